"""Shared pieces of tests/test_mag_bias_filtered.py (CPU tier) and tests/test_gpu_mag_bias_filtered.py (GPU tier): the ensemble
controllers behind the magnetometer-updated filter that ESTIMATES THE MAGNETOMETER BIAS (tsat_tvlqr_ensemble_mag_bias_filtered,
tsat_pd_ensemble_mag_bias_filtered).

THE REFERENCE (``pairs_of``) is ``reference_rollout.ensemble_loop`` with the recursion of include/tortoise_hip.h (``MagBiasEkf``,
behind ``MagBiasState``) between ``measure`` and the law — numpy and the oracle's primitives only (``ol.qmult``, ``ol.qrot``,
``ol.inv3``, ``ol.dyn7``, ``ol.plant_noise``). Sequencing, the delayed row and the PD law's raw b_m are ``reference_rollout.MagState``'s.
With ``filt=None`` it has to equal ``sensed_common.pairs_of`` with max |d| = 0; ``bias_state=False`` flies the six-state mag filter
(``mag_filtered_common.MagEkf``) on the same options, a condition of the tests.

The case of both tiers is ``sensed_common``'s; the filter's levels are MBFILT below. Every parity test first asserts its conditions on
references alone with the bar ``gg_common.MOVED`` (``conditions``).

Also: the filter as a ``filtered_common.Family``, which gives the argument lists of the two entry points (``TvCall``, ``PdCall``) and
the ctypes binding of the emulated kernels (``EmuMagBiasFiltered``; tests/emu/tsat_emu_mag_bias_filtered.cpp)."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import filtered_common as fc
import gg_common as gc
import mag_filtered_common as mc
import pd_common as pc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = 15
# the filter of the parity tests: the mag filter's levels, an initial magnetometer-bias spread of the size of sensed_common.BIAS'
# magnetometer bias and a random walk that keeps the state alive over the 20 knots
MBFILT = dict(mc.MFILT, p0_mag=1.5e-6, sigma_c=1e-7)
LEVELS = ("p0_mag", "sigma_c", "sigma_m", "sigma_v", "sigma_u", "p0_bias")
FAST = fc.FAST
GYRO_BIAS = fc.GYRO_BIAS
MAG_BIAS = 3e-6    # T, the long-horizon case

_IU = np.triu_indices(3)


class MagBiasEkf(mc.MagEkf):
    """the recursion of include/tortoise_hip.h by blocks, line for line: A, D, M symmetric (their upper triangles stand for them),
    B (theta b), E (theta c), F (b c)"""

    def __init__(self, ol, h, filt):
        super().__init__(ol, h, filt)

    def first(self, w_m, q_m):
        super().first(w_m, q_m)
        self.c = np.zeros(3)
        self.M, self.E, self.F = self.f["p0_mag"] ** 2 * np.eye(3), np.zeros((3, 3)), np.zeros((3, 3))

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
        Em = Phi @ self.E - h * self.F
        Fm = self.F
        Mm = self.M + f["sigma_c"] ** 2 * I
        n = qm / math.sqrt(float(qm @ qm))                                             # 3.
        z = b_m - self.c - ol.qrot(n, r)
        H = mc.h_matrix(n, r)
        Gt, Gb, Gc = Am @ H.T + Em, Bm.T @ H.T + Fm, Em.T @ H.T + Mm                   # 4.
        S = fc._sym(H @ Gt + Gc + f["sigma_m"] ** 2 * I)
        Si = ol.inv3(S)
        Kt, Kb, Kc = Gt @ Si, Gb @ Si, Gc @ Si
        dth, db, dcc = Kt @ z, Kb @ z, Kc @ z
        qp = ol.qmult(qm, np.r_[1.0, dth / 2])                                         # 5.
        self.q = qp / math.sqrt(float(qp @ qp))
        self.b = self.b + db
        self.w = w_m - self.b
        self.c = self.c + dcc
        Wt, Wb, Wc = Kt @ S, Kb @ S, Kc @ S                                            # 6.
        self.A = fc._sym(Am - Wt @ Kt.T)
        self.D = fc._sym(Dm - Wb @ Kb.T)
        self.M = fc._sym(Mm - Wc @ Kc.T)
        self.B = Bm - Wt @ Kb.T
        self.E = Em - Wt @ Kc.T
        self.F = Fm - Wb @ Kc.T
        self.prior = (qm, Am, Bm, Dm, Em, Fm, Mm)

    def final(self):
        return np.r_[self.b, np.sqrt(np.diag(self.A)), np.sqrt(np.diag(self.D)), self.c, np.sqrt(np.diag(self.M))]


class MagBiasState(rr.MagState):
    """``reference_rollout.MagState`` around a ``MagBiasEkf``: the sequencing, the delayed row (``_step``) and ``final`` (the
    filter's own, 15 wide) are inherited as they stand; the flat record is the 58 values of include/tortoise_hip.h —
    q^ 4, b^ 3, w^ 3, c^ 3, A 6, D 6, M 6 (upper triangles), B 9, E 9, F 9 (row-major)"""

    def record(self):
        e = self.ekf
        return np.r_[e.q, e.b, e.w, e.c, e.A[_IU], e.D[_IU], e.M[_IU], e.B.reshape(9), e.E.reshape(9), e.F.reshape(9)]


def estimator(ol, batch, filt, predict=True, pair_own_row=True, bias_state=True):
    """t -> the estimator of one loop of slew t. ``filt`` None: the raw measurement. Conditions of the tests, not modes of the
    product: ``predict`` and ``pair_own_row`` as ``mag_filtered_common.estimator``; ``bias_state`` False flies the six-state mag
    filter on the same levels (its filt_final padded to this one's width)"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    if not bias_state:
        class Padded(rr.MagState):
            def final(self):
                return np.r_[self.ekf.final(), np.zeros(FILTER_W - mc.FILTER_W)]
        return lambda t: Padded(mc.MagEkf(ol, batch.dt[t], filt), predict, pair_own_row)
    return lambda t: MagBiasState(MagBiasEkf(ol, batch.dt[t], filt), predict, pair_own_row)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, filt=None, predict=True, pair_own_row=True, bias_state=True, **kw):
    """``mag_filtered_common.pairs_of`` behind this filter"""
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs,
                       est=estimator(ol, batch, filt, predict, pair_own_row, bias_state), **kw)


def conditions(ref_of, sensor, filt=None, prediction=True, pairing=True, skip=()):
    """the conditions of a parity test on references alone (bar gg_common.MOVED, through pd_common.differs). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced; the call flies sensor biases ``sensor`` with a gyro and a
    magnetometer bias in them and the filter levels ``filt`` (default MBFILT). This filter against the six-state mag filter moves
    the final state; each of p0_mag, sigma_c, sigma_m, sigma_v, sigma_u and p0_bias against three times it moves it; the magnetometer
    bias against none moves it; latency 1 against 0 moves it; ``prediction`` and ``pairing`` as ``mag_filtered_common.conditions``.
    ``skip`` names levels whose condition the caller flies on a case of its own, where the level it needs is raised. Returns the
    reference of the call itself."""
    filt = MBFILT if filt is None else filt
    assert np.abs(sensor[..., 0:3]).min() > 0 and np.abs(sensor[..., 6:9]).min() > 0, "the conditions need a gyro and a magnetometer bias"
    ref = ref_of()
    pc.differs(ref, ref_of(bias_state=False), "this filter against the six-state mag filter")
    for name in LEVELS:
        if name not in skip:
            pc.differs(ref, ref_of(filt=dict(filt, **{name: 3.0 * filt[name]})), f"{name} against three times it")
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


def mag_bias_filter_options(abi, filt):
    return abi.MagBiasFilterOptions(sigma_v=filt["sigma_v"], sigma_u=filt["sigma_u"], sigma_m=filt["sigma_m"], sigma_c=filt["sigma_c"],
                                    p0_att=filt["p0_att"], p0_bias=filt["p0_bias"], p0_mag=filt["p0_mag"], reserved=0)


FAMILY = fc.Family(mag_bias_filter_options, FILTER_W, MBFILT, "mag_bias_filtered", "emu_mag_bias_filter_check")
TvCall, PdCall, EmuMagBiasFiltered = fc.bindings(FAMILY)


def filter_rejections(call):
    """what check_mag_bias_filter rejects of the filter options, as (label, edited call, words of the text)"""
    abi, f = call.abi, call.v["f"]

    def fo(**kw):
        o = abi.MagBiasFilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    default = abi.MagBiasFilterOptions()
    abi.load().tsat_mag_bias_filter_default_options(C.byref(default))
    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), "must be finite and >= 0"),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), "must be finite and >= 0"),
        ("sigma_m negative", call.edit(f=fo(sigma_m=-1e-9)), "must be finite and >= 0"),
        ("sigma_c negative", call.edit(f=fo(sigma_c=-1e-9)), "must be finite and >= 0"),
        ("sigma_c NaN", call.edit(f=fo(sigma_c=float("nan"))), "must be finite and >= 0"),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), "must be finite and >= 0"),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), "must be finite and >= 0"),
        ("p0_mag inf", call.edit(f=fo(p0_mag=float("inf"))), "must be finite and >= 0"),
        ("p0_mag negative", call.edit(f=fo(p0_mag=-1e-6)), "must be finite and >= 0"),
        ("sigma_m zero", call.edit(f=fo(sigma_m=0.0)), "sigma_m must be > 0"),
        ("the default options as they are", call.edit(f=default), "sigma_m must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
    ]


fast_table = mc.fast_table


def long_case(pkg, ol, N, M, mag_bias=MAG_BIAS):
    """``mag_filtered_common.long_case``'s batch, starts, generator ids and gyro figures, with a magnetometer bias of ``mag_bias``
    along np.random.default_rng(18).standard_normal((1, M, 3)), normalised, and the filter at p0_mag = ``mag_bias``, sigma_c = 0.
    Returns the case with its reference on every realisation (``ref``) and the reference of the six-state mag filter on the same
    samples (``mag``). Only the recipe is taken from the parents' long cases; their own references are not computed."""
    import mpc_held_common as hc
    tr = pkg.tracking
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=1, N=N, seed=41, rows=N))
    x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    g = np.random.default_rng(17).standard_normal((1, M, 3))
    gm = np.random.default_rng(18).standard_normal((1, M, 3))
    sensor = np.zeros((1, M, 9))
    sensor[..., 0:3] = GYRO_BIAS * g / np.linalg.norm(g, axis=-1, keepdims=True)
    sensor[..., 6:9] = mag_bias * gm / np.linalg.norm(gm, axis=-1, keepdims=True)
    smag = sc.SIGMAS["sigma_mag"]
    sens = dict(sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=smag)
    filt = dict(sigma_v=tr.SENSOR_SIGMA_GYRO, sigma_u=0.0, sigma_m=smag, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=GYRO_BIAS,
                p0_mag=mag_bias, sigma_c=0.0)
    kw = dict(X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=hc.SAT, limit_mode=1, x0_nom=np.ascontiguousarray(b.x0),
              noise_id0=np.array([2 ** 33 + 5], dtype=np.int64), sens=sens, latency=0, sensor=sensor, filt=filt)
    o = pc.options(ol)
    pairs = dc.all_pairs(1, M)
    ref = pairs_of(ol, pkg._abi, "pd", b, x0s, (sc.KD, sc.KP), o, pairs, **kw)
    mag = pairs_of(ol, pkg._abi, "pd", b, x0s, (sc.KD, sc.KP), o, pairs, bias_state=False, **kw)
    return dict(b=b, x0s=x0s, o=o, kw=kw, pairs=pairs, ref=ref, mag=mag, sensor=sensor)


rms_attitude_error = mc.rms_attitude_error


def assert_filter_works(c):
    """on the references alone: the mean over the realisations of the rms attitude error of X_hat over the last half is below the
    six-state mag filter's on the same samples; it is below it individually on at least 6 of 8; |c^ - c| at the end is below
    0.5 |c| on every realisation. Returns the figures"""
    N, n = c["b"].N, len(c["pairs"])
    est, mag = rms_attitude_error(c["ref"], N), rms_attitude_error(c["mag"], N)
    cm = np.array([c["sensor"][t, m, 6:9] for t, m in c["pairs"]])
    rel = np.linalg.norm(c["ref"]["filt_final"][:, 9:12] - cm, axis=1) / np.linalg.norm(cm, axis=1)
    better, worst = int(np.count_nonzero(est < mag)), float((est / mag).max())
    print(f"rms attitude error over the last half, deg: this filter mean {np.degrees(est).mean():.2f}, the six-state mag filter mean "
          f"{np.degrees(mag).mean():.2f}; better on {better} of {n}, worst ratio {worst:.2f}; |c^ - c| / |c| {rel.min():.2f} .. {rel.max():.2f}")
    assert est.mean() < mag.mean(), "estimating the magnetometer bias does not pay on average"
    assert better >= 6 * n // 8, "estimating the magnetometer bias loses on more than 2 of 8 realisations"
    assert np.all(rel < 0.5), "the filter does not estimate the magnetometer bias"
    return dict(est=float(np.degrees(est).mean()), mag=float(np.degrees(mag).mean()), better=better, worst=worst, rel=float(rel.max()))
