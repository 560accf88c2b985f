"""Shared pieces of tests/test_mag_filtered.py (CPU tier) and tests/test_gpu_mag_filtered.py (GPU tier): the ensemble controllers
behind the MAGNETOMETER-updated attitude filter (tsat_tvlqr_ensemble_mag_filtered, tsat_pd_ensemble_mag_filtered).

THE REFERENCE (``pairs_of``) is ``reference_rollout.ensemble_loop`` with the recursion of include/tortoise_hip.h (``MagEkf``, behind
``reference_rollout.MagState``) between ``measure`` and the law — numpy and the oracle's primitives only (``ol.qmult``, ``ol.qrot``,
``ol.inv3``, ``ol.dyn7``, ``ol.plant_noise``). The delayed ROW goes with the delayed sample: at latency 1 the sample that arrives at
knot k is knot k - 1's and is updated against r_{k-1}. The PD law reads the b_m that ``measure`` returned, the very reading the filter
used. With ``filt=None`` it has to equal ``sensed_common.pairs_of`` with max |d| = 0
(test_mag_filtered.py::test_reference_with_the_filter_off_is_the_sensed_reference).

The case of both tiers is ``sensed_common``'s; the filter's levels are MFILT below. Every parity test first asserts its conditions on
references alone with the bar ``gg_common.MOVED`` (``conditions``).

Also: the filter as a ``filtered_common.Family``, which gives the argument lists of the two entry points (``TvCall``, ``PdCall``) and
the ctypes binding of the emulated kernels (``EmuMagFiltered``; tests/emu/tsat_emu_mag_filtered.cpp)."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import filtered_common as fc
import gg_common as gc
import pd_common as pc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = fc.FILTER_W
# the filter of the parity tests: filtered_common.FILT with the magnetometer's own noise level (sensed_common.SIGMAS) in the place of
# the attitude sensor's
MFILT = dict(sigma_v=5e-3, sigma_u=1e-4, sigma_m=sc.SIGMAS["sigma_mag"], p0_att=math.radians(1.0), p0_bias=2e-3)
FAST = fc.FAST
GYRO_BIAS = fc.GYRO_BIAS


def cmat(n):
    """C(n) = I + 2 n0 [v]x + 2 [v]x^2, v = n[1:4]: qrot(n, r) = C(n) r for a unit n"""
    V = fc._skew(n[1:4])
    return np.eye(3) + 2.0 * n[0] * V + 2.0 * V @ V


def h_matrix(n, r):
    """H = -C(n) [r]x: the derivative of qrot(n (x) [1; dtheta / 2], r) in dtheta at 0"""
    return -cmat(n) @ fc._skew(r)


class MagEkf(fc.Ekf):
    """the recursion of include/tortoise_hip.h, line for line; ``first`` is the six-state filter's. ``update`` False: gyro dead
    reckoning from the first fix (K = 0: steps 1, 2, 5 and 6 alone), a condition of the tests, not a mode of the product"""

    def __init__(self, ol, h, filt, update=True):
        super().__init__(ol, h, filt)
        self.update = update

    def step(self, w_m, b_m, r):
        ol, h, f, I = self.ol, self.h, self.f, np.eye(3)
        d = fc.dq_of(h * self.w)                                                       # 1.
        qm = ol.qmult(self.q, d)
        V = fc._skew(d[1:4])
        Phi = (I + 2 * d[0] * V + 2 * V @ V).T
        PB = Phi @ self.B                                                              # 2.
        Am = fc._sym(Phi @ self.A @ Phi.T - h * (PB + PB.T) + h * h * self.D + (f["sigma_v"] * h) ** 2 * I)
        Bm = PB - h * self.D
        Dm = self.D + f["sigma_u"] ** 2 * I
        n = qm / math.sqrt(float(qm @ qm))                                             # 3.
        z = b_m - ol.qrot(n, r)
        H = h_matrix(n, r)
        G, Gb = Am @ H.T, Bm.T @ H.T                                                   # 4.
        S = fc._sym(H @ G) + f["sigma_m"] ** 2 * I
        Si = ol.inv3(S)
        Kt, Kb = G @ Si, Gb @ Si
        if not self.update:
            Kt, Kb = np.zeros((3, 3)), np.zeros((3, 3))
        dth, db = Kt @ z, Kb @ z
        qp = ol.qmult(qm, np.r_[1.0, dth / 2])                                         # 5.
        self.q = qp / math.sqrt(float(qp @ qp))
        self.b = self.b + db
        self.w = w_m - self.b
        self.A = fc._sym(Am - Kt @ S @ Kt.T)                                           # 6.
        self.B = Bm - Kt @ S @ Kb.T
        self.D = fc._sym(Dm - Kb @ S @ Kb.T)
        self.prior = (qm, Am, Bm, Dm)


def estimator(ol, batch, filt, predict=True, update=True, pair_own_row=True):
    """t -> the estimator of one loop of slew t: ``MagEkf`` behind ``reference_rollout.MagState``. ``filt`` None: the raw
    measurement. Conditions of the tests, not modes of the product: ``predict`` False leaves the prediction across the delay out,
    ``update`` False the magnetometer update (gyro dead reckoning from the first fix), ``pair_own_row`` False updates the delayed
    sample against r_k in the place of r_{k-1}"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    return lambda t: rr.MagState(MagEkf(ol, batch.dt[t], filt, update), predict, pair_own_row)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, filt=None, predict=True, update=True, pair_own_row=True, **kw):
    """``filtered_common.pairs_of`` behind this filter"""
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, est=estimator(ol, batch, filt, predict, update, pair_own_row), **kw)


def conditions(ref_of, sensor, prediction=True, pairing=True):
    """the conditions of a parity test on references alone (bar gg_common.MOVED, through pd_common.differs). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced; the call flies sensor biases ``sensor`` with a gyro and a
    magnetometer bias in them. This filter against gyro dead reckoning from the same first fix moves the final state; each of
    sigma_v, sigma_m, sigma_u and p0_bias against three times it moves it; the magnetometer bias against none moves it; latency 1
    against 0 moves it; removing the prediction across the delay moves it (``prediction`` False leaves that one to the test that
    flies the case on which it shows under the PD law: the starts with the body rate FAST under wide limits); at latency 1, pairing
    the delayed sample with r_k in the place of r_{k-1} moves it (``pairing`` False leaves that one to the test that flies the table
    on which it shows, ``fast_table``). Returns the reference of the call itself."""
    assert np.abs(sensor[..., 0:3]).min() > 0 and np.abs(sensor[..., 6:9]).min() > 0, "the conditions need a gyro and a magnetometer bias"
    ref = ref_of()
    pc.differs(ref, ref_of(update=False), "this filter against gyro dead reckoning from the same first fix")
    for name in ("sigma_v", "sigma_m", "sigma_u", "p0_bias"):
        pc.differs(ref, ref_of(filt=dict(MFILT, **{name: 3.0 * MFILT[name]})), f"{name} against three times it")
    z = sensor.copy()
    z[..., 6:9] = 0.0
    pc.differs(ref, ref_of(sensor=z), "magnetometer bias on against zero")
    pc.differs(ref_of(latency=1), ref_of(latency=0), "latency 1 against 0")
    if prediction:
        pc.differs(ref_of(latency=1), ref_of(latency=1, predict=False), "prediction across the delay on against off")
    if pairing:
        pc.differs(ref_of(latency=1), ref_of(latency=1, pair_own_row=False), "the delayed sample against r_{k-1}, not r_k")
    return ref


compare_estimates = fc.compare_estimates


def mag_filter_options(abi, filt):
    return abi.MagFilterOptions(sigma_v=filt["sigma_v"], sigma_u=filt["sigma_u"], sigma_m=filt["sigma_m"], p0_att=filt["p0_att"],
                                p0_bias=filt["p0_bias"], reserved=0)


FAMILY = fc.Family(mag_filter_options, FILTER_W, MFILT, "mag_filtered", "emu_mag_filter_check")
TvCall, PdCall, EmuMagFiltered = fc.bindings(FAMILY)


def filter_rejections(call):
    """what check_mag_filter rejects of the filter options, as (label, edited call, words of the text)"""
    abi, f = call.abi, call.v["f"]

    def fo(**kw):
        o = abi.MagFilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    default = abi.MagFilterOptions()
    abi.load().tsat_mag_filter_default_options(C.byref(default))
    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), "must be finite and >= 0"),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), "must be finite and >= 0"),
        ("sigma_m negative", call.edit(f=fo(sigma_m=-1e-9)), "must be finite and >= 0"),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), "must be finite and >= 0"),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), "must be finite and >= 0"),
        ("sigma_m zero", call.edit(f=fo(sigma_m=0.0)), "sigma_m must be > 0"),
        ("the default options as they are", call.edit(f=default), "sigma_m must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
    ]


def fast_table(batch, turn_deg=25.0):
    """the batch with field tables whose rows turn faster from knot to knot: row i of every table rotated by i * ``turn_deg`` about an
    axis fixed per table. At the case's own tables two neighbouring rows differ by 4.5e-4 of the field, and the row a delayed sample is
    paired with moves the final state by 4e-8 (TVLQR) and 8e-9 (PD), under the bar of 1e-7; here they differ by about 40 % of the
    field. The level raised is the table's turning rate alone; the law, the plants, the sensor and the filter are the case's."""
    import dataclasses
    B = np.array(batch.Btab, dtype=np.float64)
    for i in range(B.shape[0]):
        ax = np.array([1.0, 2.0, -1.5 + i]) / np.linalg.norm([1.0, 2.0, -1.5 + i])
        K = fc._skew(ax)
        for j in range(B.shape[1]):
            a = math.radians(turn_deg) * j
            B[i, j] = (np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * K @ K) @ B[i, j]
    return dataclasses.replace(batch, Btab=np.ascontiguousarray(B))


def long_case(pkg, ol, N, M):
    """``filtered_common.long_case`` behind this filter: the same batch, starts, generator ids, gains, limits and gyro figures, with
    sigma_mag = sensed_common.SIGMAS["sigma_mag"] in sensor and filter, no magnetometer bias and p0_bias = GYRO_BIAS. Returns the case
    with its reference on every realisation (``ref``) and the reference of gyro dead reckoning from the same first fix (``dead``).
    Only the batch and the starts are taken from ``filtered_common.long_case``'s recipe; its own reference is not computed."""
    import mpc_held_common as hc
    tr = pkg.tracking
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=1, N=N, seed=41, rows=N))
    x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    g = np.random.default_rng(17).standard_normal((1, M, 3))
    sensor = np.zeros((1, M, 9))
    sensor[..., 0:3] = GYRO_BIAS * g / np.linalg.norm(g, axis=-1, keepdims=True)
    smag = sc.SIGMAS["sigma_mag"]
    sens = dict(sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=smag)
    filt = dict(sigma_v=tr.SENSOR_SIGMA_GYRO, sigma_u=0.0, sigma_m=smag, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=GYRO_BIAS)
    kw = dict(X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=hc.SAT, limit_mode=1, x0_nom=np.ascontiguousarray(b.x0),
              noise_id0=np.array([2 ** 33 + 5], dtype=np.int64), sens=sens, latency=0, sensor=sensor, filt=filt)
    o = pc.options(ol)
    pairs = dc.all_pairs(1, M)
    ref = pairs_of(ol, pkg._abi, "pd", b, x0s, (sc.KD, sc.KP), o, pairs, **kw)
    dead = pairs_of(ol, pkg._abi, "pd", b, x0s, (sc.KD, sc.KP), o, pairs, update=False, **kw)
    return dict(b=b, x0s=x0s, o=o, kw=kw, pairs=pairs, ref=ref, dead=dead, sensor=sensor)


def rms_attitude_error(ref, N):
    """per realisation, the rms over the last half of the horizon of the angle between X_hat and the true attitude (rad)"""
    half = slice(N // 2, N - 1)
    return np.array([math.sqrt(float(np.mean(fc._angles(ref["X_hat"][i, half, 3:7], ref["X_sim"][i, half, 3:7]) ** 2)))
                     for i in range(len(ref["X_sim"]))])


def assert_filter_works(c):
    """on the references alone: the mean over the realisations of the rms attitude error of X_hat over the last half is below that of
    gyro dead reckoning from the same first fix; it is below it individually on all but at most one realisation; |b^ - bw| at the
    end is below GYRO_BIAS on every realisation"""
    N, n = c["b"].N, len(c["pairs"])
    est, dead = rms_attitude_error(c["ref"], N), rms_attitude_error(c["dead"], N)
    db = np.array([float(np.linalg.norm(c["ref"]["filt_final"][i, 0:3] - c["sensor"][t, m, 0:3])) for i, (t, m) in enumerate(c["pairs"])])
    print(f"rms attitude error over the last half, deg: this filter {np.degrees(est).min():.2f} .. {np.degrees(est).max():.2f} (mean "
          f"{np.degrees(est).mean():.2f}), dead reckoning {np.degrees(dead).min():.2f} .. {np.degrees(dead).max():.2f} (mean "
          f"{np.degrees(dead).mean():.2f}); better on {int(np.count_nonzero(est < dead))} of {n}, worst ratio {float((est / dead).max()):.2f}; "
          f"|b^ - bw| {db.min():.2e} .. {db.max():.2e} against {GYRO_BIAS:.1e}")
    assert est.mean() < dead.mean(), "the filter does not beat gyro dead reckoning on average"
    assert np.count_nonzero(est < dead) >= n - 1, "the filter loses to gyro dead reckoning on more than one realisation"
    assert np.all(db < GYRO_BIAS), "the filter does not estimate the gyro bias"
