"""Shared pieces of tests/test_sensed.py (CPU tier) and tests/test_gpu_sensed.py (GPU tier): the ensemble controllers FED
MEASUREMENTS (tsat_tvlqr_ensemble_sensed, tsat_pd_ensemble_sensed).

THE REFERENCES are ``gg_common.ensemble_loop`` (``law="tv"``) and ``pd_common.reference_loop`` (``law="pd"``) with the three
measurement lines of include/tortoise_hip.h (``measure``) and the latency rule inserted — built from ``ol.plant_noise``,
``ol.qmult``, ``ol.qrot``, ``ol.dyn7``, ``ol.inv3`` (through ``gg_common.gg_increment``) and numpy only —, everything else operation
for operation as there. With no biases, zero sigmas and latency 0 each has to equal its parent with max |d| = 0
(test_sensed.py::test_references_with_the_ideal_sensor_are_their_parents).

The case of both tiers is ``pd_common.case`` with two changes that make a sensor error visible at all: the TVLQR weights are
``tvlqr_weights(T, r=R_LQR)`` with R_LQR = 0.5e-6 (|K| up to 4.8e3; at the parity tests' usual r = 0.5e3 the gains move the final
state by 2e-13) and the PD gains are 10 x pd_common.KD / KP. Every parity test first asserts its conditions on references alone
with the bar ``gg_common.MOVED`` (``conditions``): sensor noise, gyro bias, attitude bias, magnetometer bias (PD) and latency 1
against 0 each move the final state by at least the bar.

Also: the ctypes binding of the emulated kernels (tests/emu/tsat_emu_sensed.cpp, built on demand by its own make fragment), and the
argument lists of the two entry points for the GPU tier."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import helpers
import pd_common as pc

R_LQR = 0.5e-6
KD, KP = 10.0 * pc.KD, 10.0 * pc.KP
# the levels of the parity tests
SIGMAS = dict(sigma_gyro=3e-4, sigma_att=math.radians(0.3), sigma_mag=5e-7)
BIAS = dict(gyro_bias=1.5e-3, att_bias_deg=0.7, mag_bias=1.5e-6)
IDEAL = dict(sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0)


def biases(pkg, T, M):
    return pkg.tracking.disperse_sensor(T, M, np.random.default_rng(11), **BIAS)


def measure(ol, batch, t, k, x, opts, gid, sens, bias, noisy):
    """y_k = (w_m, q_m, b_m) of the true state x at knot k; ``sens`` holds the three sigmas, ``bias`` (9,) or None"""
    bw, ba, bm = (np.zeros(3),) * 3 if bias is None else (bias[0:3], bias[3:6], bias[6:9])
    if noisy:
        n = ol.plant_noise(int(opts.noise_seed), int(gid), k, 4, sens["sigma_gyro"], sens["sigma_att"], 0.0)
        n_w, n_a = n[0:3], n[3:6]
        n_m = ol.plant_noise(int(opts.noise_seed), int(gid), k, 5, sens["sigma_mag"], 0.0, 0.0)[0:3]
    else:
        n_w = n_a = n_m = np.zeros(3)
    w_m = x[:3] + bw + n_w
    phi = ba + n_a
    th = math.sqrt(float(phi @ phi))
    dq = np.r_[math.cos(th / 2), phi * (0.5 if th == 0.0 else math.sin(th / 2) / th)]
    q_m = ol.qmult(x[3:7], dq)
    b_m = ol.qrot(x[3:7] / math.sqrt(float(x[3:7] @ x[3:7])), dc._row(batch, t, k, 0.0)) + bm + n_m
    return w_m, q_m, b_m


def loop(ol, law, batch, t, Xr, Ur, gains, x0, opts, gid, Rtab, gm, plant=None, lo=None, hi=None, limit_mode=0, noisy=True, sens=None,
         latency=0, bias=None, k_start=0, k_stop=None, x_before=None):
    """one closed loop of slew t fed measurements: ``reference_rollout.ensemble_loop`` with no filter. Returns X_sim (N, 7)
    zero-filled beyond the horizon, (n_sure, n_maybe), the commands before the limit (N-1, 3)."""
    import reference_rollout as rr          # here: that module is built on this one
    return rr.ensemble_loop(ol, law, batch, t, Xr, Ur, gains, x0, opts, gid, Rtab, gm, plant, lo, hi, limit_mode, noisy, sens, latency,
                            bias, k_start=k_start, k_stop=k_stop, x_before=x_before)[:3]


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=None, limit_mode=0,
             x0_nom=None, noise_id0=None, sens=None, latency=0, sensor=None):
    """``reference_rollout.pairs_of`` with no filter"""
    import reference_rollout as rr
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, X, U, Rtab, gm, plant, sat, limit_mode, x0_nom, noise_id0, sens,
                       latency, sensor)


def conditions(ref_of, law, sensor):
    """the conditions of a parity test on references alone (bar gg_common.MOVED, through pd_common.differs). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced. Sensor noise, gyro bias, attitude bias and — under the PD law —
    magnetometer bias each move the final state, and so does latency 1 against 0. Returns the reference of the call itself."""
    ref = ref_of()
    pc.differs(ref, ref_of(sens=IDEAL), "sensor noise on against off")
    for name, sl in (("gyro", slice(0, 3)), ("attitude", slice(3, 6))) + ((("magnetometer", slice(6, 9)),) if law == "pd" else ()):
        z = sensor.copy()
        z[..., sl] = 0.0
        pc.differs(ref, ref_of(sensor=z), f"{name} bias on against zero")
    pc.differs(ref_of(latency=1), ref_of(latency=0), "latency 1 against 0")
    return ref


def sensor_options(abi, sens, latency):
    return abi.SensorOptions(sigma_gyro=sens["sigma_gyro"], sigma_att=sens["sigma_att"], sigma_mag=sens["sigma_mag"], latency=int(latency),
                             reserved=0)


def _dc(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class TvCall:
    """the arguments of tsat_tvlqr_ensemble_sensed after the handle (``c_args()``), or — ``emu=True`` — of emu_tvlqr_ensemble_sensed,
    which takes K as an input before ``stats`` and returns none; arrays are kept alive here"""

    def __init__(self, abi, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K=None, plant=None, Rtab=None, gm=0.0, sat=None, noise_id0=None,
                 sens=IDEAL, latency=0, sensor=None, trajectories=True, so=0):
        self.abi = abi
        T, N, M = batch.T, batch.N, x0_sim.shape[1]
        o = abi.TvlqrOptions.from_buffer_copy(opts)
        o.n_knots, o.n_tab = N, batch.n_tab
        lo, hi = (None, None) if sat is None else (_dc(np.broadcast_to(sat[0], (T, 3))), _dc(np.broadcast_to(sat[1], (T, 3))))
        self.v = dict(o=o, T=T, n_btab=batch.Btab.shape[0], M=M, X=_dc(X), U=_dc(U), xf=_dc(batch.xf), Btab=_dc(batch.Btab),
                      btab_idx=np.ascontiguousarray(batch.btab_idx, dtype=np.int32), tau0=_dc(batch.tau0), dtau=_dc(batch.dtau),
                      dt=_dc(batch.dt), Jmat=_dc(batch.Jmat), Qd=_dc(Qd), Qfd=_dc(Qfd), Rd=_dc(Rd), x0_sim=_dc(x0_sim),
                      noise_id0=None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64),
                      n_knots=None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32), plant=_dc(plant),
                      sat_lo=lo, sat_hi=hi, K=_dc(K), stats=np.zeros((T, M), dtype=abi.TVLQR_STATS_DTYPE), summary=np.zeros((T, 8)),
                      stats_nominal=np.zeros(T, dtype=abi.TVLQR_STATS_DTYPE), X_sim=np.full((T, M, N, 7), np.nan) if trajectories else None,
                      n_clipped=np.full((T, M), -1, dtype=np.int32), Rtab=_dc(Rtab), gm=float(gm),
                      s=sensor_options(abi, sens, latency) if so == 0 else so, sensor=_dc(sensor))

    def edit(self, **kw):
        other = type(self).__new__(type(self))
        other.abi, other.v = self.abi, dict(self.v)
        for k, val in kw.items():
            assert k in other.v, k
            other.v[k] = _dc(val) if isinstance(val, np.ndarray) and val.dtype.kind == "f" else val
        return other

    def c_args(self, emu=False):
        v, d, ip = self.v, self.abi.as_dp, self.abi.as_ip
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        head = [None if v["o"] is None else C.byref(v["o"]), C.c_int64(v["T"]), C.c_int64(v["n_btab"]), C.c_int32(v["M"]), d(v["X"]), d(v["U"]),
                d(v["xf"]), d(v["Btab"]), ip(v["btab_idx"]), d(v["tau0"]), d(v["dtau"]), d(v["dt"]), d(v["Jmat"]), d(v["Qd"]), d(v["Qfd"]),
                d(v["Rd"]), d(v["x0_sim"]), None if v["noise_id0"] is None else v["noise_id0"].ctypes.data_as(C.POINTER(C.c_int64)),
                ip(v["n_knots"]), d(v["plant"]), d(v["sat_lo"]), d(v["sat_hi"])]
        mid = [d(v["K"]), vp(v["stats"]), d(v["summary"]), vp(v["stats_nominal"]), d(v["X_sim"])] if emu else \
              [vp(v["stats"]), d(v["summary"]), vp(v["stats_nominal"]), None, d(v["X_sim"])]
        return head + mid + [ip(v["n_clipped"]), d(v["Rtab"]), C.c_double(v["gm"]), None if v["s"] is None else C.byref(v["s"]), d(v["sensor"])]

    def parent_args(self, gravity):
        """the arguments of the emulated parents out of the call's own: emu_tvlqr_ensemble_dispersed, or — ``gravity`` —
        emu_tvlqr_ensemble_gg, which end before the sensor's"""
        return self.c_args(emu=True)[:30 if gravity else 28]

    def result(self):
        v = self.v
        return dict(stats=v["stats"], summary=v["summary"], nominal=v["stats_nominal"], X_sim=v["X_sim"], n_clipped=v["n_clipped"])


def smallest_tv_call(pkg, opts):
    """the smallest valid TVLQR call — T = 1, N = 4, M = 1, zero gains, with a plant, limits and an orbit table — for the tests of
    what the emulated drivers reject"""
    import gg_common as gc
    import mpc_held_common as hc
    b = hc.mpc_batch(pkg, T=1, N=4, rows=4)
    X, U, K = np.repeat(b.x0[:, None], 4, axis=1), np.zeros((1, 3, 3)), np.zeros((1, 3, 6, 3))
    return TvCall(pkg._abi, b, opts, X, U, *pkg.tracking.tvlqr_weights(1, r=0.5e3), b.x0[:, None], K=K, plant=hc.plants(pkg, b, 1),
                  Rtab=gc.orbit(pkg, 4, 0.2)[None], gm=gc.GM, sat=hc.SAT)


class PdCall(pc.Call):
    """pd_common.Call followed by the two sensor arguments: tsat_pd_ensemble_sensed after the handle, or emu_pd_ensemble_sensed"""

    def __init__(self, abi, batch, opts, x0_sim, kd, kp, sens=IDEAL, latency=0, sensor=None, so=0, **kw):
        super().__init__(abi, batch, opts, x0_sim, kd, kp, **kw)
        self.v["s"] = sensor_options(abi, sens, latency) if so == 0 else so
        self.v["sensor"] = _dc(sensor)

    def c_args(self, names=pc.FIELDS):
        s = self.v["s"]
        return super().c_args(names) + [None if s is None else C.byref(s), self.abi.as_dp(self.v["sensor"])]


def sensor_rejections(call):
    """what check_sensor rejects, as (label, edited call, words of the text); ``call`` a good sensed call with a sensor array"""
    abi, s, sensor = call.abi, call.v["s"], call.v["sensor"]

    def so(**kw):
        o = abi.SensorOptions.from_buffer_copy(s)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def bad(idx, val):
        z = sensor.copy()
        z[idx] = val
        return z

    T, M = sensor.shape[:2]
    return [
        ("s NULL", call.edit(s=None), "null sensor options"),
        ("sigma_gyro NaN", call.edit(s=so(sigma_gyro=float("nan"))), "must be finite and >= 0"),
        ("sigma_att inf", call.edit(s=so(sigma_att=float("inf"))), "must be finite and >= 0"),
        ("sigma_mag negative", call.edit(s=so(sigma_mag=-1e-9)), "must be finite and >= 0"),
        ("sigma_gyro negative", call.edit(s=so(sigma_gyro=-1.0)), "must be finite and >= 0"),
        ("latency 2", call.edit(s=so(latency=2)), "latency must be 0"),
        ("latency -1", call.edit(s=so(latency=-1)), "latency must be 0"),
        ("sensor NaN", call.edit(sensor=bad((1, 2, 4), np.nan)), "non-finite sensor entry at (t, m) = (1, 2)"),
        ("sensor inf", call.edit(sensor=bad((T - 1, M - 1, 8), np.inf)), f"non-finite sensor entry at (t, m) = ({T - 1}, {M - 1})"),
        ("sensor -inf", call.edit(sensor=bad((0, 0, 0), -np.inf)), "non-finite sensor entry at (t, m) = (0, 0)"),
    ]


class EmuSensed:
    """ctypes binding of tests/emu/libtsat_emu_sensed.so (the four emulated kernels), built here by its own make fragment"""

    def __init__(self, abi):
        self.lib = helpers.emu_library("libtsat_emu_sensed.so")
        self.abi = abi

    def tv(self, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K, **kw):
        """emu_tvlqr_ensemble_sensed; keyword arguments as ``TvCall``; the result dict of ``tracking.attitude_ensemble_sensed``"""
        call = TvCall(self.abi, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K=K, **kw)
        rc = self.lib.emu_tvlqr_ensemble_sensed(*call.c_args(emu=True))
        if rc != 0:
            raise RuntimeError(f"emu_tvlqr_ensemble_sensed rc={rc}")
        return call.result()

    def pd(self, batch, opts, x0_sim, kd, kp, **kw):
        """emu_pd_ensemble_sensed; keyword arguments as ``PdCall``; the result dict of ``tracking.attitude_ensemble_pd_sensed``"""
        call = PdCall(self.abi, batch, opts, x0_sim, kd, kp, **kw)
        rc = self.lib.emu_pd_ensemble_sensed(*call.c_args())
        if rc != 0:
            raise RuntimeError(f"emu_pd_ensemble_sensed rc={rc}")
        return call.result()

    def check(self, call):
        """check_sensor on the sensor arguments of a call"""
        text = C.create_string_buffer(256)
        s, sensor = call.v["s"], call.v["sensor"]
        rc = self.lib.emu_sensed_check(None if s is None else C.byref(s), self.abi.as_dp(sensor), C.c_int64(call.v["T"]), C.c_int32(call.v["M"]),
                                       text, C.c_int32(256))
        return rc, text.value.decode()
