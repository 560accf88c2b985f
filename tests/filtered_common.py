"""Shared pieces of tests/test_filtered.py (CPU tier) and tests/test_gpu_filtered.py (GPU tier): the ensemble controllers behind a
multiplicative EKF (tsat_tvlqr_ensemble_filtered, tsat_pd_ensemble_filtered).

THE REFERENCE (``pairs_of``) is ``reference_rollout.ensemble_loop`` with the recursion of include/tortoise_hip.h (``Ekf``, behind
``reference_rollout.SixState``) between ``measure`` and the law — numpy and the oracle's primitives only (``ol.qmult``, ``ol.inv3``,
``ol.plant_noise``, ``ol.qrot``, ``ol.dyn7``). With ``filt=None`` it has to equal ``sensed_common.pairs_of`` with max |d| = 0
(test_filtered.py::test_reference_with_the_filter_off_is_the_sensed_reference); it also returns X_hat and filt_final.

The case of both tiers is ``sensed_common``'s; the filter's levels are FILT below. Every parity test first asserts its conditions on
references alone with the bar ``gg_common.MOVED`` (``conditions``).

Also, once for the four filter families (``Family``; the other three name theirs in model_filtered_common, mag_filtered_common and
mag_bias_filtered_common): the argument lists of the two entry points (``TvCall``, ``PdCall``) and the ctypes binding of the emulated
kernels (``EmuFiltered``; tests/emu/tsat_emu_filtered.cpp and its three siblings)."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np

import dispersed_common as dc
import gg_common as gc
import helpers
import pd_common as pc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = 9
# the filter of the parity tests: it assumes the sensor's own attitude noise (sensed_common.SIGMAS), a bias random walk and an initial
# bias spread of the size of sensed_common.BIAS' gyro bias, and a gyro noise of 5e-3 rad/s (near the reference's 0.38 deg/s figure;
# at the sensor's own 3e-4 rad/s the term (sigma_v h)^2 moves the final states of the 8-slew case by 6e-8 only), so that every option acts
FILT = dict(sigma_v=5e-3, sigma_u=1e-4, sigma_a=sc.SIGMAS["sigma_att"], p0_att=math.radians(1.0), p0_bias=2e-3)
# body rate added to the starts of the tests of the prediction across the delay under the PD law: the prediction turns the estimate
# by h w^, and at the case's own rates (|w| < 1e-3 rad/s) and gains that moves the final state by 5e-8 .. 3e-7, on or under the bar
FAST = np.array([0.03, -0.02, 0.025])


def dq_of(phi):
    th = math.sqrt(float(phi @ phi))
    return np.r_[math.cos(th / 2), phi * (0.5 if th == 0.0 else math.sin(th / 2) / th)]


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _sym(A):
    """the matrix the upper triangle of A stands for"""
    return np.triu(A) + np.triu(A, 1).T


class Ekf:
    """the recursion of include/tortoise_hip.h, line for line"""

    def __init__(self, ol, h, filt):
        self.ol, self.h, self.f = ol, float(h), filt

    def first(self, w_m, q_m):
        f = self.f
        self.q = q_m / math.sqrt(float(q_m @ q_m))
        self.b = np.zeros(3)
        self.w = np.array(w_m, dtype=np.float64)
        self.A, self.B, self.D = f["p0_att"] ** 2 * np.eye(3), np.zeros((3, 3)), f["p0_bias"] ** 2 * np.eye(3)

    def step(self, w_m, q_m):
        ol, h, f, I = self.ol, self.h, self.f, np.eye(3)
        d = dq_of(h * self.w)                                                          # 1.
        qm = ol.qmult(self.q, d)
        V = _skew(d[1:4])
        Phi = (I + 2 * d[0] * V + 2 * V @ V).T
        PB = Phi @ self.B                                                              # 2.
        Am = _sym(Phi @ self.A @ Phi.T - h * (PB + PB.T) + h * h * self.D + (f["sigma_v"] * h) ** 2 * I)
        Bm = PB - h * self.D
        Dm = self.D + f["sigma_u"] ** 2 * I
        e = ol.qmult(np.r_[qm[0], -qm[1:4]], q_m / math.sqrt(float(q_m @ q_m)))        # 3.
        z = 2.0 * (-1.0 if e[0] < 0 else 1.0) * e[1:4]
        S = Am + f["sigma_a"] ** 2 * I                                                 # 4.
        Si = ol.inv3(S)
        Kt, Kb = Am @ Si, Bm.T @ Si
        dth, db = Kt @ z, Kb @ z
        qp = ol.qmult(qm, np.r_[1.0, dth / 2])                                         # 5.
        self.q = qp / math.sqrt(float(qp @ qp))
        self.b = self.b + db
        self.w = w_m - self.b
        self.A = _sym(Am - Kt @ S @ Kt.T)                                              # 6.
        self.B = Bm - Kt @ S @ Kb.T
        self.D = _sym(Dm - Kb @ S @ Kb.T)

    def predicted(self):
        return self.ol.qmult(self.q, dq_of(self.h * self.w))

    def final(self):
        return np.r_[self.b, np.sqrt(np.diag(self.A)), np.sqrt(np.diag(self.D))]


def estimator(ol, batch, filt, predict=True):
    """t -> the estimator of one loop of slew t: ``Ekf`` behind ``reference_rollout.SixState``. ``filt`` None: the raw measurement;
    ``predict`` False leaves the prediction across the delay out (a condition of the tests, not a mode of the product)"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    return lambda t: rr.SixState(Ekf(ol, batch.dt[t], filt), predict)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, filt=None, predict=True, **kw):
    """``sensed_common.pairs_of`` (its keyword arguments) behind the filter: X_hat (n, N, 7) and filt_final (n, 9) are the filter's,
    Y_raw (n, N, 7) the raw (w_m, q_m) the law would have seen"""
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, est=estimator(ol, batch, filt, predict), **kw)


def conditions(ref_of, sensor, prediction=True):
    """the conditions of a parity test on references alone (bar gg_common.MOVED, through pd_common.differs). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced; the call flies sensor biases ``sensor`` with a gyro bias in them.
    Filtered against raw moves the final state; each of sigma_v, sigma_a, sigma_u and p0_bias moves it; latency 1 against 0 moves it;
    removing the prediction across the delay moves it (``prediction`` False leaves that one to the test that flies the case on which
    it shows under the PD law: starts with the body rate FAST under wide limits). Returns the reference of the call itself."""
    assert np.abs(sensor[..., 0:3]).min() > 0, "the conditions on sigma_u and p0_bias need a gyro bias"
    ref = ref_of()
    pc.differs(ref, ref_of(filt=None), "filtered against raw")
    for name in ("sigma_v", "sigma_a", "sigma_u", "p0_bias"):
        pc.differs(ref, ref_of(filt=dict(FILT, **{name: 3.0 * FILT[name]})), f"{name} against three times it")
    pc.differs(ref_of(latency=1), ref_of(latency=0), "latency 1 against 0")
    if prediction:
        pc.differs(ref_of(latency=1), ref_of(latency=1, predict=False), "prediction across the delay on against off")
    return ref


def compare_estimates(ref, got, pairs, idx=None):
    """X_hat and filt_final against the reference to 1e-9, the project's bar for these loops; X_hat zero from the last knot on"""
    idx = np.arange(len(pairs)) if idx is None else idx
    t, m = pairs[idx, 0], pairs[idx, 1]
    dH = float(np.max(np.abs(ref["X_hat"][idx] - got["X_hat"][t, m])))
    dF = float(np.max(np.abs(ref["filt_final"][idx] - got["filt_final"][t, m])))
    print(f"max|dX_hat| {dH:.2e}  max|dfilt_final| {dF:.2e} against the reference")
    assert dH < 1e-9 and dF < 1e-9
    for i, n in zip(idx, ref["n_knots"][idx]):
        assert np.all(got["X_hat"][pairs[i, 0], pairs[i, 1], n - 1:] == 0) and np.all(ref["X_hat"][i, n - 1:] == 0)
        assert np.all(np.abs(got["X_hat"][pairs[i, 0], pairs[i, 1], :n - 1, 3:7]).max(axis=1) > 0)


GYRO_BIAS = 2e-3   # rad/s, the long-horizon case


def long_case(pkg, ol, N, M):
    """T = 1, N knots, M realisations: the PD law (10 x pd_common's gains, direction-preserving limit +-0.6) regulating from the
    workload's start on the model's plant with plant noise, no gravity gradient; the reference's sensor figures (0.38 deg/s, 1 deg),
    a gyro bias of GYRO_BIAS in a drawn direction per realisation and no other bias, latency 0; the filter with the default figures
    plus a bias state (p0_bias = GYRO_BIAS). Returns the case with its reference on every realisation."""
    import mpc_held_common as hc
    tr = pkg.tracking
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=1, N=N, seed=41, rows=N))
    x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    g = np.random.default_rng(17).standard_normal((1, M, 3))
    sensor = np.zeros((1, M, 9))
    sensor[..., 0:3] = GYRO_BIAS * g / np.linalg.norm(g, axis=-1, keepdims=True)
    sens = dict(sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=0.0)
    filt = dict(sigma_v=tr.SENSOR_SIGMA_GYRO, sigma_u=0.0, sigma_a=tr.SENSOR_SIGMA_ATT, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=GYRO_BIAS)
    kw = dict(X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=hc.SAT, limit_mode=1, x0_nom=np.ascontiguousarray(b.x0),
              noise_id0=np.array([2 ** 33 + 5], dtype=np.int64), sens=sens, latency=0, sensor=sensor, filt=filt)
    o = pc.options(ol)
    pairs = dc.all_pairs(1, M)
    ref = pairs_of(ol, pkg._abi, "pd", b, x0s, (sc.KD, sc.KP), o, pairs, **kw)
    return dict(b=b, x0s=x0s, o=o, kw=kw, pairs=pairs, ref=ref, sensor=sensor)


def _angles(qa, qb):
    """rotation angle between rows of two (n, 4) quaternion arrays, neither assumed unit"""
    c = np.abs(np.sum(qa * qb, axis=1)) / (np.linalg.norm(qa, axis=1) * np.linalg.norm(qb, axis=1))
    return 2.0 * np.arccos(np.minimum(c, 1.0))


def assert_filter_works(c):
    """on the reference alone, for every realisation: the rms attitude error of X_hat over the last half of the horizon is below
    that of the raw measurement, and |b^ - bw| at the end is below |bw|"""
    ref, N = c["ref"], c["b"].N
    half = slice(N // 2, N - 1)
    est, raw, db = [], [], []
    for i, (t, m) in enumerate(c["pairs"]):
        true = ref["X_sim"][i, half, 3:7]
        est.append(math.sqrt(float(np.mean(_angles(ref["X_hat"][i, half, 3:7], true) ** 2))))
        raw.append(math.sqrt(float(np.mean(_angles(ref["Y_raw"][i, half, 3:7], true) ** 2))))
        db.append(float(np.linalg.norm(ref["filt_final"][i, 0:3] - c["sensor"][t, m, 0:3])))
    est, raw, db = np.array(est), np.array(raw), np.array(db)
    print(f"rms attitude error over the last half, deg: raw {np.degrees(raw).min():.3f} .. {np.degrees(raw).max():.3f}, "
          f"filtered {np.degrees(est).min():.3f} .. {np.degrees(est).max():.3f}; |b^ - bw| {db.min():.2e} .. {db.max():.2e} against {GYRO_BIAS:.1e}")
    assert np.all(est < raw), "the filter does not beat the raw attitude measurement"
    assert np.all(db < GYRO_BIAS), "the filter does not estimate the gyro bias"


def filter_options(abi, filt):
    return abi.FilterOptions(sigma_v=filt["sigma_v"], sigma_u=filt["sigma_u"], sigma_a=filt["sigma_a"], p0_att=filt["p0_att"],
                             p0_bias=filt["p0_bias"], reserved=0)


@dataclasses.dataclass(frozen=True)
class Family:
    """what tells the calls of one filter from those of another"""
    options: object    # (abi, filt) -> the options block of the filter
    width: int         # FILTER_W: doubles of filt_final per realisation
    levels: dict       # the filter of the parity tests
    suffix: str        # tsat_{tvlqr,pd}_ensemble_<suffix>, emu_..._<suffix>, tests/emu/libtsat_emu_<suffix>.so
    check: str         # the emulator's symbol of the library's check of the options


SIX_STATE = Family(filter_options, FILTER_W, FILT, "filtered", "emu_filter_check")
_LEVELS = object()     # the default of ``filt``: the family's own levels


def _outputs(v, abi, family, filt, fo, estimates):
    """the three filter arguments of a call: ``fo`` 0 builds the options from ``filt`` (None: f = NULL and no outputs)"""
    T, M, N = v["T"], v["M"], v["o"].n_knots
    filt = family.levels if filt is _LEVELS else filt
    v["f"] = (None if filt is None else family.options(abi, filt)) if fo == 0 else fo
    on = v["f"] is not None
    v["X_hat"] = np.full((T, M, N, 7), np.nan) if (on and estimates) else None
    v["filt_final"] = np.full((T, M, family.width), np.nan) if (on and estimates) else None


def _tail(v, abi):
    return [None if v["f"] is None else C.byref(v["f"]), abi.as_dp(v["X_hat"]), abi.as_dp(v["filt_final"])]


class TvCall(sc.TvCall):
    """sensed_common.TvCall followed by the three filter arguments of ``family``: tsat_tvlqr_ensemble_<suffix> after the handle, or —
    ``emu=True`` — emu_tvlqr_ensemble_<suffix>"""

    def __init__(self, abi, *a, family=SIX_STATE, filt=_LEVELS, fo=0, estimates=True, **kw):
        super().__init__(abi, *a, **kw)
        _outputs(self.v, abi, family, filt, fo, estimates)

    def c_args(self, emu=False):
        return super().c_args(emu) + _tail(self.v, self.abi)

    def result(self):
        return dict(super().result(), X_hat=self.v["X_hat"], filt_final=self.v["filt_final"])


class PdCall(sc.PdCall):
    """sensed_common.PdCall followed by the three filter arguments of ``family``: tsat_pd_ensemble_<suffix> after the handle, or
    emu_pd_ensemble_<suffix>"""

    def __init__(self, abi, *a, family=SIX_STATE, filt=_LEVELS, fo=0, estimates=True, **kw):
        super().__init__(abi, *a, **kw)
        _outputs(self.v, abi, family, filt, fo, estimates)

    def c_args(self, names=pc.FIELDS):
        return super().c_args(names) + _tail(self.v, self.abi)

    def result(self):
        return dict(super().result(), X_hat=self.v["X_hat"], filt_final=self.v["filt_final"])


def filter_rejections(call):
    """what check_filter and the entry points reject of the filter arguments, as (label, edited call, words of the text)"""
    abi, f = call.abi, call.v["f"]

    def fo(**kw):
        o = abi.FilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), "must be finite and >= 0"),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), "must be finite and >= 0"),
        ("sigma_a negative", call.edit(f=fo(sigma_a=-1e-3)), "must be finite and >= 0"),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), "must be finite and >= 0"),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), "must be finite and >= 0"),
        ("sigma_a zero", call.edit(f=fo(sigma_a=0.0)), "sigma_a must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
    ]


class EmuFiltered:
    """ctypes binding of tests/emu/libtsat_emu_<suffix>.so (the four emulated kernels of a family), built by the emulator's pattern rule"""

    def __init__(self, abi, family=SIX_STATE):
        self.lib = helpers.emu_library(f"libtsat_emu_{family.suffix}.so")
        self.abi, self.family = abi, family

    def _run(self, law, call, *a):
        name = f"emu_{law}_ensemble_{self.family.suffix}"
        rc = getattr(self.lib, name)(*call.c_args(*a))
        if rc != 0:
            raise RuntimeError(f"{name} rc={rc}")
        return call.result()

    def tv(self, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K, **kw):
        """emu_tvlqr_ensemble_<suffix>; keyword arguments as ``TvCall``; the result dict of ``tracking.attitude_ensemble_<suffix>``"""
        return self._run("tvlqr", TvCall(self.abi, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K=K, family=self.family, **kw), True)

    def pd(self, batch, opts, x0_sim, kd, kp, **kw):
        """emu_pd_ensemble_<suffix>; keyword arguments as ``PdCall``; the result dict of ``tracking.attitude_ensemble_pd_<suffix>``"""
        return self._run("pd", PdCall(self.abi, batch, opts, x0_sim, kd, kp, family=self.family, **kw))

    def check(self, call):
        """the library's check of the family's filter options on those of a call"""
        text = C.create_string_buffer(256)
        f = call.v["f"]
        rc = getattr(self.lib, self.family.check)(None if f is None else C.byref(f), text, C.c_int32(256))
        return rc, text.value.decode()


def bindings(family):
    """TvCall, PdCall and EmuFiltered of a family, for the module that names it"""
    return (functools.partial(TvCall, family=family), functools.partial(PdCall, family=family), functools.partial(EmuFiltered, family=family))
