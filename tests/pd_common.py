"""Shared pieces of tests/test_pd.py (CPU tier) and tests/test_gpu_pd.py (GPU tier): the PROJECTION PD LAW on the dispersed plants
(tsat_pd_ensemble).

THE REFERENCE is ``gg_common.ensemble_loop`` with the command line ``u = Ur[k] - K[k].T @ dX`` replaced by the definition of
include/tortoise_hip.h — built from ``ol.qmult``, ``ol.qrot``, ``ol.dyn7``, ``ol.plant_noise``, ``ol.inv3`` (through
``gg_common.gg_increment``) and numpy only —, everything else operation for operation as there. With kd = kp = 0, feed-forward on
and limit_mode 0 it has to equal ``gg_common.ensemble_loop`` called with an all-zero K, max |d| = 0
(test_pd.py::test_reference_with_zero_gains_is_the_gg_reference). The clip bookkeeping is n_sure / n_maybe with
``dispersed_common.CLIP_BAND``; in limit_mode 1 the band is applied to beta - 1.

The case of both tiers is the fixture of tests/test_gpu_gg.py (``case``), with the gains KD / KP for every slew. Every parity test
first asserts its own condition on references alone with the bar of ``gg_common.moved`` (1e-7): ``differs``.

Also: the argument list of the entry point as named fields (``Call``), which the rejection tests edit one field at a time and hand
to the library's own validation function — through the emulator driver (``EmuPd.check``) on the CPU tier, through
tsat_pd_ensemble itself on the GPU tier —, and the ctypes binding of the emulated kernels (tests/emu/tsat_emu_pd.cpp)."""
import ctypes as C

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import helpers
import mpc_held_common as hc

KD = np.array([2e-5, 3e-5, 1e-5])        # N m s / rad
KP = np.array([4e-7, 2e-7, 6e-7])        # N m
BIDX = np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=np.int32)
ORBITS = ((0.0, 0.0), (40.0, 70.0))      # RAAN, true anomaly (deg) of the two tables
WIDE = hc.WIDE                           # limits +-25: no command of the case reaches them


def case(pkg, T=8, bidx=BIDX):
    """the batch and the orbit table of tests/test_gpu_gg.py's fixture: N = 20, ragged horizons, the 3U inertia, two dipole tables
    with their orbits behind a non-identity btab_idx, 16 rows under a clock that runs to row 17.3"""
    ss = pkg.slew_setup
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=T, N=20, seed=3 if T == 8 else 41))
    n_tab = 16
    b.Btab = np.ascontiguousarray(np.stack([ss.dipole_btable(n_tab, 0.2, gc.A_KM, gc.INC, ra, nu) for ra, nu in ORBITS]))
    b.n_tab, b.btab_idx = n_tab, np.ascontiguousarray(bidx[:T])
    b.tau0[:], b.dtau[:] = 0.25, 0.9
    b.n_knots = hc.RAGGED[:T].copy()
    Rtab = np.ascontiguousarray(np.stack([gc.orbit(pkg, n_tab, 0.2, ra, nu) for ra, nu in ORBITS]))
    return b, Rtab


def options(ol):
    o = ec.tv_options(ol)
    o.min_steps, o.w_tol, o.angle_tol = hc.MIN_STEPS, hc.W_TOL, hc.ANGLE_TOL
    return o


def reference_loop(ol, batch, t, Xr, Ur, kd, kp, x0, opts, gid, Rtab, gm, plant=None, lo=None, hi=None, limit_mode=0, noisy=True,
                   sign_rule=True, k_start=0, k_stop=None):
    """one closed loop of slew t under the law, on the true state: ``reference_rollout.ensemble_loop``. Returns X_sim (N, 7)
    zero-filled beyond the horizon, (n_sure, n_maybe), the commands before the limit (N-1, 3) and the beta of every knot (mode 1)."""
    import reference_rollout as rr          # here: that module is built on this one's parents
    return rr.ensemble_loop(ol, "pd", batch, t, Xr, Ur, (kd, kp), x0, opts, gid, Rtab, gm, plant, lo, hi, limit_mode, noisy,
                            sign_rule=sign_rule, k_start=k_start, k_stop=k_stop)[:4]


def reference_pairs(ol, abi, batch, x0_sim, kd, kp, opts, pairs, X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=None, limit_mode=0,
                    x0_nom=None, noise_id0=None, sign_rule=True):
    """the reference on the (t, m) pairs (n, 2); m = -1 is the noise-free MODEL plant from x0_nom[t] (default X[t, 0]). kd / kp
    (T, 3) or (3,). Returns the dict of ``reference_rollout.pairs_of``."""
    import reference_rollout as rr
    return rr.pairs_of(ol, abi, "pd", batch, x0_sim, (kd, kp), opts, pairs, X=X, U=U, Rtab=Rtab, gm=gm, plant=plant, sat=sat,
                       limit_mode=limit_mode, x0_nom=x0_nom, noise_id0=noise_id0, sign_rule=sign_rule)


def finals(r):
    return [r["X_sim"][i, n - 1] for i, n in enumerate(r["n_knots"])]


def differs(a, b, label):
    """a condition of a parity test, on two references alone: their final states differ by >= gg_common.MOVED somewhere among the
    compared pairs"""
    d = float(np.max(np.abs(np.asarray(finals(a)) - np.asarray(finals(b)))))
    print(f"{label}: the references' final states differ by {d:.2e}")
    assert d >= gc.MOVED, f"{label} does not show on this case: a kernel that ignores it would pass"
    return d


def limit_condition(ref, ref_mode0, kind, mode):
    """the condition on the limit, on references alone. Tracking WITHOUT feed-forward commands the law's dipole alone, 1e-4 .. 1e-2
    units of u_scale under the gains of the case: it never comes near +-0.6, which is asserted as such (no knot within the band of
    a limit), and there the two limit rules are the same rule. With feed-forward (the plan's own +-19 box) and in regulation the
    limits act, and a mode-1 reference has to differ from its mode-0 twin (``ref_mode0()``) by the bar of ``differs``"""
    if kind == "track":
        assert not ref["n_maybe"].any(), "tracking without feed-forward reached a limit: assert mode 1 against mode 0 here too"
        return
    assert ref["n_sure"].max() > 0, "no knot of the case clips"
    if mode == 1:
        differs(ref, ref_mode0(), "mode 1 against mode 0")
        near = min(abs(x - 1.0) for bs in ref["betas"] for x in bs)
        print(f"nearest beta to 1: {near:.2e}")
        assert near > 100 * dc.CLIP_BAND


FIELDS = ("o", "T", "n_btab", "M", "X", "U", "xf", "Btab", "btab_idx", "tau0", "dtau", "dt", "Jmat", "kd", "kp", "feedforward", "limit_mode",
          "x0_sim", "x0_nom", "noise_id0", "n_knots", "plant", "sat_lo", "sat_hi", "stats", "summary", "stats_nominal", "X_sim", "n_clipped",
          "Rtab", "gm")
_INT64, _INT32 = ("T", "n_btab"), ("M", "feedforward", "limit_mode")


class Call:
    """the arguments of tsat_pd_ensemble after the handle, by name; ``c_args()`` in the order of the C ABI. Arrays are made contiguous
    and kept alive here; outputs are allocated unless given"""

    def __init__(self, abi, batch, opts, x0_sim, kd, kp, X=None, U=None, plant=None, Rtab=None, gm=0.0, sat=None, limit_mode=0,
                 x0_nom=None, noise_id0=None, trajectories=True, nominal=True):
        self.abi = abi
        T, N, M = batch.T, batch.N, x0_sim.shape[1]
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        o = abi.TvlqrOptions.from_buffer_copy(opts)
        o.n_knots, o.n_tab = N, batch.n_tab
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        self.v = dict(
            o=o, T=T, n_btab=batch.Btab.shape[0], M=M, X=c(X), U=c(U), xf=c(batch.xf), Btab=c(batch.Btab),
            btab_idx=np.ascontiguousarray(batch.btab_idx, dtype=np.int32), tau0=c(batch.tau0), dtau=c(batch.dtau), dt=c(batch.dt),
            Jmat=c(batch.Jmat), kd=c(np.broadcast_to(kd, (T, 3))), kp=c(np.broadcast_to(kp, (T, 3))), feedforward=0 if U is None else 1,
            limit_mode=limit_mode, x0_sim=c(x0_sim), x0_nom=c(x0_nom),
            noise_id0=None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64),
            n_knots=None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32), plant=c(plant), sat_lo=lo,
            sat_hi=hi, stats=np.zeros((T, M), dtype=abi.TVLQR_STATS_DTYPE), summary=np.zeros((T, 8)),
            stats_nominal=np.zeros(T, dtype=abi.TVLQR_STATS_DTYPE) if nominal else None,
            X_sim=np.full((T, M, N, 7), np.nan) if trajectories else None, n_clipped=np.full((T, M), -1, dtype=np.int32), Rtab=c(Rtab),
            gm=float(gm))

    def edit(self, **kw):
        """a copy with the named fields replaced (float arrays made contiguous); ``o_<field>=value`` edits the options block"""
        other = type(self).__new__(type(self))
        other.abi, other.v = self.abi, dict(self.v)
        for k, val in kw.items():
            if k.startswith("o_"):
                o = self.abi.TvlqrOptions.from_buffer_copy(other.v["o"])
                setattr(o, k[2:], val)
                other.v["o"] = o
            else:
                assert k in other.v, k
                other.v[k] = np.ascontiguousarray(val, dtype=np.float64) if isinstance(val, np.ndarray) and val.dtype.kind == "f" else val
        return other

    def c_args(self, names=FIELDS):
        out = []
        for n in names:
            a = self.v[n]
            if n == "o":
                out.append(None if a is None else C.byref(a))
            elif n in _INT64:
                out.append(C.c_int64(a))
            elif n in _INT32:
                out.append(C.c_int32(a))
            elif n == "gm":
                out.append(C.c_double(a))
            elif a is None:
                out.append(None)
            elif n in ("stats", "stats_nominal"):
                out.append(a.ctypes.data_as(C.c_void_p))
            elif n == "noise_id0":
                out.append(a.ctypes.data_as(C.POINTER(C.c_int64)))
            elif a.dtype == np.int32:
                out.append(self.abi.as_ip(a))
            else:
                out.append(self.abi.as_dp(a))
        return out

    def result(self):
        v = self.v
        return dict(stats=v["stats"], summary=v["summary"], nominal=v["stats_nominal"], X_sim=v["X_sim"], n_clipped=v["n_clipped"])


def rejections(call, batch, Rtab):
    """every rejection of the issue's list as (label, edited call, words of the text); `call` is a good tracking call with
    feed-forward, plants, limits, orbit table and x0_nom"""
    T = batch.T
    bad = lambda a, idx, val: (lambda x: (x.__setitem__(idx, val), x)[1])(np.array(a, dtype=np.float64))
    kd, kp, lo, hi, plant = (call.v[k] for k in ("kd", "kp", "sat_lo", "sat_hi", "plant"))
    return [
        ("kd NULL", call.edit(kd=None), "null kd or kp"), ("kp NULL", call.edit(kp=None), "null kd or kp"),
        ("kd NaN", call.edit(kd=bad(kd, (1, 2), np.nan)), "kd and kp must be finite and >= 0 (t = 1)"),
        ("kp inf", call.edit(kp=bad(kp, (0, 0), np.inf)), "kd and kp must be finite and >= 0 (t = 0)"),
        ("kd negative", call.edit(kd=bad(kd, (T - 1, 1), -1e-9)), f"kd and kp must be finite and >= 0 (t = {T - 1})"),
        ("kp negative", call.edit(kp=bad(kp, (0, 1), -1.0)), "kd and kp must be finite"),
        ("feedforward 2", call.edit(feedforward=2), "feedforward must be 0"), ("feedforward -1", call.edit(feedforward=-1), "feedforward must be 0"),
        ("feedforward without X", call.edit(X=None), "feedforward = 1 needs the plan"),
        ("feedforward without U", call.edit(U=None), "feedforward = 1 needs the plan"),
        ("limit_mode 2", call.edit(limit_mode=2), "limit_mode must be 0"), ("limit_mode -1", call.edit(limit_mode=-1), "limit_mode must be 0"),
        ("mode 1 without limits", call.edit(limit_mode=1, sat_lo=None, sat_hi=None), "limit_mode = 1 needs sat_lo and sat_hi"),
        ("mode 1, lo = 0", call.edit(limit_mode=1, sat_lo=bad(lo, (1, 0), 0.0)), "sat_lo < 0 < sat_hi in every component (t = 1)"),
        ("mode 1, hi < 0", call.edit(limit_mode=1, sat_lo=bad(lo, (0, 2), -2.0), sat_hi=bad(hi, (0, 2), -1.0)), "sat_lo < 0 < sat_hi"),
        ("regulation, nominal without x0_nom", call.edit(X=None, U=None, feedforward=0, x0_nom=None), "stats_nominal needs x0_nom"),
        ("Rtab NULL, gm != 0", call.edit(Rtab=None, gm=gc.GM), "Rtab is NULL but gm != 0"),
        ("Rtab NULL, gm NaN", call.edit(Rtab=None, gm=float("nan")), "Rtab is NULL but gm != 0"),
        # ... and what tsat_tvlqr_ensemble_gg rejects
        ("options NULL", call.edit(o=None), "null handle or options"), ("noise_mode 0", call.edit(o_noise_mode=0), "noise_mode must be 1"),
        ("rate_as_written", call.edit(o_rate_as_written=1), "rate_as_written must be 0"), ("M = 0", call.edit(M=0), "M must be in [1, 65535]"),
        ("T = 0", call.edit(T=0), "bad batch dimensions"), ("xf NULL", call.edit(xf=None), "null array"),
        ("x0_sim NULL", call.edit(x0_sim=None), "null array"), ("stats NULL", call.edit(stats=None), "null array"),
        ("btab_idx NULL", call.edit(btab_idx=None, T=1), "btab_idx is NULL but n_btab != T"),
        ("btab_idx range", call.edit(btab_idx=np.full(T, 2, dtype=np.int32)), "btab_idx out of range"),
        ("dt = 0", call.edit(dt=np.zeros(T)), "dt must be positive"),
        ("n_knots 1", call.edit(n_knots=np.full(T, 1, dtype=np.int32)), "n_knots[t] must be in [2, N]"),
        ("one limit NULL", call.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"),
        ("lo > hi", call.edit(sat_lo=bad(lo, (1, 1), 1.0)), "sat_lo > sat_hi (or not a number) at t = 1"),
        ("plant NaN", call.edit(plant=bad(plant, (1, 2, 20), np.nan)), "non-finite plant entry at (t, m) = (1, 2)"),
        ("Jp not symmetric", call.edit(plant=bad(plant, (0, 1, 1), 1e-3)), "Jp is not symmetric at (t, m) = (0, 1)"),
        ("Rtab NaN", call.edit(Rtab=bad(Rtab, (1, 4, 2), np.nan)), "non-finite Rtab entry in row 20"),
        ("Rtab zero row", call.edit(Rtab=bad(Rtab, (1, 0), 0.0)), "row 16 has |r| = 0"), ("gm negative", call.edit(gm=-1.0), "gm must be finite"),
    ]


class EmuPd:
    """ctypes binding of tests/emu/libtsat_emu_pd.so, built here by its own make fragment"""

    def __init__(self, abi):
        self.lib = helpers.emu_library("libtsat_emu_pd.so")
        self.abi = abi

    def run(self, batch, opts, x0_sim, kd, kp, **kw):
        """emu_pd_ensemble; keyword arguments as ``Call``; the result dict of ``tracking.attitude_ensemble_pd``"""
        call = Call(self.abi, batch, opts, x0_sim, kd, kp, **kw)
        rc = self.lib.emu_pd_ensemble(*call.c_args())
        if rc != 0:
            raise RuntimeError(f"emu_pd_ensemble rc={rc}")
        return call.result()

    def check(self, call):
        text = C.create_string_buffer(256)
        names = [n for n in FIELDS if n not in ("noise_id0", "X_sim", "n_clipped")]
        rc = self.lib.emu_pd_check(*call.c_args(names), text, C.c_int32(256))
        return rc, text.value.decode()
