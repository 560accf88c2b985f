"""Shared pieces of tests/test_model_mag_filtered.py (CPU tier) and tests/test_gpu_model_mag_filtered.py (GPU tier): the ensemble
controllers behind the model-based rate filter UPDATED BY THE MAGNETOMETER (tsat_tvlqr_ensemble_model_mag_filtered,
tsat_pd_ensemble_model_mag_filtered).

THE REFERENCE (``pairs_of``) is ``reference_rollout.ensemble_loop`` with the recursion of include/tortoise_hip.h between ``measure``
and the law: ``ModelMagEkf`` — ``model_filtered_common.ModelEkf`` with update a. replaced by ``_mag``, which uses
``mag_filtered_common.h_matrix``, ``ol.qrot`` and the parent's ``_apply`` — behind ``ModelMagState``, the parent's sequencing handing
over b_m and the row it was formed with. Numpy and the oracle's primitives only. With ``filt=None`` it has to equal
``sensed_common.pairs_of`` with max |d| = 0.

The case of both tiers is ``sensed_common``'s; the filter's levels are FILT below. Every parity test first asserts its conditions on
references alone with the bar ``gg_common.MOVED`` (``conditions``): terms of the recursion are switched off through ``variant`` and
``pair_own_row``, which are devices of the tests, not modes of the product. A label that a test leaves to the case on which it shows
is printed with its figure.

Both tiers compare the same realisations in the same way (``parity``): the tier hands over how it runs a call (the emulated kernels,
or the library through ``tracking``)."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import filtered_common as fc
import gg_common as gc
import mag_filtered_common as gfc
import model_filtered_common as mfc
import mpc_held_common as hc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = 12
# the filter of the parity tests. At model_filtered_common.FILT's levels (1e-3, 3e-4, 1e-4) sigma_v, sigma_w and sigma_u move the
# final states of the case by 4e-8 .. 9e-8 behind this filter, under the bar: without an attitude sensor the covariance is larger and
# those terms are a smaller part of it. At these each of the seven moves them by 8.5e-7 .. 8.2e-6 against three times itself.
FILT = dict(sigma_v=5e-3, sigma_w=3e-3, sigma_u=5e-4, sigma_g=5e-3, sigma_m=sc.SIGMAS["sigma_mag"], p0_att=math.radians(1.0), p0_bias=2e-3)
LEVELS = ("sigma_v", "sigma_w", "sigma_u", "sigma_g", "sigma_m", "p0_att", "p0_bias")
FAST = fc.FAST
GYRO_BIAS = fc.GYRO_BIAS
# the sensor and filter on which the ORDER of the two updates shows: model_filtered_common's loud gyro, and a magnetometer as loud
# against the field (2.5e-5 T) as that case's attitude sensor is: 3 deg of it, 1.3e-6 T. The order acts only through the second-order
# term of the quaternion correction, so both corrections have to be large.
LOUD_MAG = 2.5e-5 * math.radians(3.0)
LOUD_SENS = dict(mfc.LOUD_SENS, sigma_mag=LOUD_MAG)
LOUD_FILT = dict(sigma_v=1e-3, sigma_w=3e-4, sigma_u=1e-4, sigma_g=2e-2, sigma_m=LOUD_MAG, p0_att=math.radians(3.0), p0_bias=2e-3)
VARIANT = dict(mfc.VARIANT, mag=True)          # ``mag`` False leaves the magnetometer update out


class ModelMagEkf(mfc.ModelEkf):
    """the recursion of include/tortoise_hip.h: the parent's ``first``, ``predict``, ``_apply`` and ``_gyro``, with ``_mag`` in
    the place of ``_attitude``"""

    def __init__(self, ol, h, J, us, filt, variant=VARIANT):
        super().__init__(ol, h, J, us, filt, variant)

    def _mag(self, b_m, r):
        if not self.v["mag"]:
            return
        ol, f, P = self.ol, self.f, self.P
        n = self.q / math.sqrt(float(self.q @ self.q))
        z = b_m - ol.qrot(n, r)
        Hm = gfc.h_matrix(n, r)
        PH = P[:, 0:3] @ Hm.T
        S = mfc._sym(Hm @ PH[0:3]) + f["sigma_m"] ** 2 * np.eye(3)
        self._apply(PH, S, z)

    def update(self, w_m, b_m, r):
        if self.v["order"] == "ab":
            self._mag(b_m, r)
            self._gyro(w_m)
        else:
            self._gyro(w_m)
            self._mag(b_m, r)


class ModelMagState(rr.ModelState):
    """``reference_rollout.ModelState``'s sequencing, each update against the sample's b_m and the row it was formed with (``row_m``:
    r_{k-1} for the delayed sample of latency 1). ``pair_own_row`` False pairs it with r_k: a condition of the tests"""

    def __init__(self, ekf, predict=True, pair_own_row=True):
        super().__init__(ekf, predict)
        self.pair_own_row = pair_own_row

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev):
        e = self.ekf
        r = row_m if self.pair_own_row else rows[0]
        if k == 0:
            e.first(w_m, q_m)
            e.u = np.zeros(3)
            self.fin, post = e.final(), (e.w, e.q)
        elif latency:
            if k > 1:                                       # m_0 handed over a second time: no update
                e.update(w_m, b_m, r)
            self.fin, post = e.final(), (e.w, e.q)
            self._predict(u_prev, rows_prev)
        else:
            self._predict(u_prev, rows_prev)
            e.update(w_m, b_m, r)
            self.fin, post = e.final(), (e.w, e.q)
        return (e.w, e.q) if self.predict else post


def estimator(ol, batch, opts, filt, variant=VARIANT, pair_own_row=True):
    """t -> the estimator of one loop of slew t: ``ModelMagEkf`` on the MODEL's inertia behind ``ModelMagState``. ``filt`` None: the
    raw measurement"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    return lambda t: ModelMagState(ModelMagEkf(ol, float(batch.dt[t]), np.asarray(batch.Jmat[t]).reshape(3, 3).T, float(opts.u_scale), filt,
                                               variant), variant["predict"], pair_own_row)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, filt=None, variant=VARIANT, pair_own_row=True, **kw):
    """``filtered_common.pairs_of`` behind this filter: its dict with filt_final (n, 12)"""
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, est=estimator(ol, batch, opts, filt, variant, pair_own_row), **kw)


COMMAND, GYROSCOPIC, ORDER = mfc.COMMAND, mfc.GYROSCOPIC, "the update order a, b against b, a"
PAIRING = "the delayed sample against r_{k-1}, not r_k"
DELAY = mfc.DELAY[0]
MAG = "the magnetometer update on against off"
# the labels that do not show on the case's own starts, sensor and tables (their figures there: the command 8e-8 .. 9e-8, the
# gyroscopic term 4e-9 .. 5e-9, the order 3e-10, the pairing 5e-8, the prediction across the delay 7e-8): each is asserted by the
# test that flies the case on which it shows
LEFT = (COMMAND, GYROSCOPIC, ORDER, PAIRING, DELAY)


moved = mfc.moved


def conditions(ref_of, sensor, latency, skip=LEFT, filt=FILT):
    """the conditions of a parity test on references alone (bar gg_common.MOVED on the final states). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced; the call flies sensor biases ``sensor`` with a gyro and a
    magnetometer bias in them. Each of the seven levels against three times itself moves the final state; so do the magnetometer
    update against none, the magnetometer bias against zero, latency 1 against 0, the command in predict, the gyroscopic term, the
    update order and, at latency 1, the row the delayed sample is paired with and the prediction across the delay. ``skip`` names the
    labels left to the test that flies the case on which they show: their figures are printed. Returns the reference of the call."""
    assert np.abs(sensor[..., 0:3]).min() > 0 and np.abs(sensor[..., 6:9]).min() > 0, "the conditions need a gyro and a magnetometer bias"
    ref = ref_of()
    z = sensor.copy()
    z[..., 6:9] = 0.0
    terms = [(f"{n} against three times it", ref, dict(filt=dict(filt, **{n: 3.0 * filt[n]}))) for n in LEVELS]
    terms += [(MAG, ref, dict(variant=dict(VARIANT, mag=False))),
              ("magnetometer bias on against zero", ref, dict(sensor=z)),
              ("latency 1 against 0", ref, dict(latency=1 - latency)),
              (COMMAND, ref, dict(variant=dict(VARIANT, command=False))),
              (GYROSCOPIC, ref, dict(variant=dict(VARIANT, gyroscopic=False))),
              (ORDER, ref, dict(variant=dict(VARIANT, order="ba")))]
    if latency:
        terms += [(PAIRING, ref, dict(pair_own_row=False)), (DELAY, ref, dict(variant=dict(VARIANT, predict=False)))]
    short = []
    for label, base, over in terms:
        d = moved(base, ref_of(**over))
        print(f"  condition: {label}: max|d final state| {d:.2e}" + ("  (left to the case that shows it)" if label in skip else ""))
        if label not in skip and not d >= gc.MOVED:
            short.append(f"{label} moves the final state by {d:.2e} only")
    assert not short, short
    return ref


def compare_estimates(ref, got, pairs, idx=None):
    """X_hat and filt_final against the reference to 1e-9; X_hat zero from the last knot on"""
    assert got["filt_final"].shape[-1] == FILTER_W
    fc.compare_estimates(ref, got, pairs, idx)


def filter_options(abi, filt):
    return abi.ModelMagFilterOptions(sigma_v=filt["sigma_v"], sigma_w=filt["sigma_w"], sigma_u=filt["sigma_u"], sigma_g=filt["sigma_g"],
                                     sigma_m=filt["sigma_m"], p0_att=filt["p0_att"], p0_bias=filt["p0_bias"], reserved=0)


first_record = mfc.first_record          # filt_final when no update was made: ``first`` is the parent's


FAMILY = fc.Family(filter_options, FILTER_W, FILT, "model_mag_filtered", "emu_model_mag_filter_check")
TvCall, PdCall, EmuModelMagFiltered = fc.bindings(FAMILY)


def filter_rejections(call):
    """what check_model_mag_filter rejects of the filter options, as (label, edited call, words of the text)"""
    abi, f = call.abi, call.v["f"]

    def fo(**kw):
        o = abi.ModelMagFilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    default = abi.ModelMagFilterOptions()
    abi.load().tsat_model_mag_filter_default_options(C.byref(default))
    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), "must be finite and >= 0"),
        ("sigma_w negative", call.edit(f=fo(sigma_w=-1e-6)), "must be finite and >= 0"),
        ("sigma_w inf", call.edit(f=fo(sigma_w=float("inf"))), "must be finite and >= 0"),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), "must be finite and >= 0"),
        ("sigma_g NaN", call.edit(f=fo(sigma_g=float("nan"))), "must be finite and >= 0"),
        ("sigma_m negative", call.edit(f=fo(sigma_m=-1e-9)), "must be finite and >= 0"),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), "must be finite and >= 0"),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), "must be finite and >= 0"),
        ("sigma_g zero", call.edit(f=fo(sigma_g=0.0)), "sigma_g must be > 0"),
        ("sigma_m zero", call.edit(f=fo(sigma_m=0.0)), "sigma_m must be > 0"),
        ("the default options as they are", call.edit(f=default), "sigma_m must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
    ]


# ---- the calls of both tiers --------------------------------------------------------------------------------------------------

KINDS = ("track", "track_ff", "regulate")
N_COND = 4          # compared pairs the conditions are evaluated on: shown on a part of them, they hold on all


def cut(a, M):
    return None if a is None else np.ascontiguousarray(a[:, :M])


def tv_kw(e, M, sat=hc.SAT, **over):
    """the keyword arguments that the reference, the emulator's driver and (``sens`` spread, ``filt`` as ``filter``) the wrapper take"""
    kw = dict(Rtab=e["Rtab"], gm=gc.GM, plant=cut(e["plant"], M), sat=sat, sens=sc.SIGMAS, latency=0, sensor=cut(e["sensor"], M), filt=FILT)
    kw.update(over)
    return kw


def pd_kw(e, kind, mode, M, **over):
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"], gm=gc.GM,
              plant=cut(e["plant"], M), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"], sens=sc.SIGMAS, latency=0, sensor=cut(e["sensor"], M),
              filt=FILT)
    kw.update(over)
    return kw


def ref_of(pkg, ol, e, M, law, pairs, kw, batch=None):
    if law == "tv":
        return pairs_of(ol, pkg._abi, "tv", batch or e["b"], e["x0s"][:, :M], e["K"], e["o"], pairs, X=e["X"], U=e["U"], **kw)
    return pairs_of(ol, pkg._abi, "pd", batch or e["b"], e["x0s"][:, :M], (sc.KD, sc.KP), e["o"], pairs, **kw)


def nomp(b):
    return np.array([(t, -1) for t in range(b.T)])


def cond_pairs(e, ref, pairs, keep):
    cp = pairs[keep[ref["n_knots"][keep] == e["b"].N][:N_COND]]
    assert len(cp) == N_COND
    return cp


def parity(pkg, ol, run, e, M, law, kw, skip=LEFT, only=None, batch=None):
    """34 seeded (t, m) drawn, the first 32 off the statistic's thresholds compared; at most 2 are replaced, which is a condition on
    the reference alone and asserted (``gg_common.kept``). X_sim, stats, n_clipped, X_hat and filt_final; the summary, the zero fill
    and stats_nominal with them. The conditions are asserted first, on references alone, over the first N_COND compared pairs of
    full horizon; ``skip`` None asserts none (a second run of a case whose conditions another run asserts), ``only`` names the labels
    to assert alone. ``run(law, e, M, kw, batch)`` is the tier's call. Returns (ref, got, keep)."""
    b = batch or e["b"]
    pairs = dc.sampled_pairs(b.T, M)
    ref = ref_of(pkg, ol, e, M, law, pairs, kw, batch)
    keep = gc.kept(ref, e["o"])
    if skip is not None:
        cp = cond_pairs(dict(e, b=b), ref, pairs, keep)
        every = (MAG, "magnetometer bias on against zero", "latency 1 against 0") + LEFT + tuple(f"{n} against three times it" for n in LEVELS)
        sk = tuple(l for l in every if l not in only) if only is not None else skip
        conditions(lambda **o: ref_of(pkg, ol, e, M, law, cp, dict(kw, **o), batch), kw["sensor"], kw["latency"], skip=sk, filt=kw["filt"])
    got = run(law, e, M, kw, batch)
    dc.compare(ref, got, pairs, keep)
    compare_estimates(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
    ec.same_stats(ref_of(pkg, ol, e, M, law, nomp(b), kw, batch)["stats"], got["nominal"])
    return ref, got, keep


def zero_row_batch(b0):
    """row 5 of field table 0 set to zero: under the case's clock (row floor(0.25 + 0.9 k)) it is the stage-0 row of knot 6 of every
    slew on that table whose horizon reaches it"""
    import dataclasses
    B = b0.Btab.copy()
    B[0, 5] = 0.0
    b = dataclasses.replace(b0, Btab=np.ascontiguousarray(B))
    assert any(np.array_equal(dc._row(b, t, 6, 0.0), np.zeros(3)) and b.n_knots[t] > 8 for t in range(b.T))
    return b


def tiny_batch(b0):
    """n_knots = 2, 3 and 4 among the slews, two of each"""
    import dataclasses
    nk = b0.n_knots.copy()
    nk[[0, 5]], nk[[1, 7]], nk[[2, 6]] = 2, 3, 4
    return dataclasses.replace(b0, n_knots=nk)


def check_tiny(pkg, ol, run, e, M, b):
    """latency 1 on ``tiny_batch``: with 2 knots ``first`` only and filt_final is ``first_record``; with 3, k = 1 makes no update
    (filt_final still ``first_record``, y_1 the model's prediction from the first sample); with 4, one update, at k = 2"""
    pairs = dc.sampled_pairs(b.T, M)
    for law, kw in (("tv", tv_kw(e, M, latency=1)), ("pd", pd_kw(e, "track_ff", 0, M, latency=1)), ("pd", pd_kw(e, "regulate", 1, M, latency=1))):
        ref = ref_of(pkg, ol, e, M, law, pairs, kw, b)
        tiny = np.flatnonzero(ref["n_knots"] <= 4)
        assert set(ref["n_knots"][tiny]) == {2, 3, 4}, "the sample must hold the three tiny horizons"
        got = run(law, e, M, kw, b)
        # a horizon of 2 or 3 knots has no sample past min_steps: nothing of it can sit on a threshold, and the margin is taken on
        # the others
        none = np.flatnonzero(ref["n_knots"] <= 3)
        big = np.flatnonzero(ref["n_knots"] > 3)
        o = e["o"]
        ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], o.min_steps, o.w_tol, o.angle_tol)
                       > dc.MARGIN for i in big])
        assert np.count_nonzero(~ok) <= dc.N_DRAWN - dc.N_KEPT, "more than 2 of the sampled realisations sit on a threshold"
        idx = np.concatenate([none, big[ok]])
        assert np.isin(tiny, idx).all(), "a tiny horizon sits on a threshold"
        dc.compare(ref, got, pairs, idx)
        compare_estimates(ref, got, pairs, idx)
        assert np.all(got["stats"]["failed"][pairs[none, 0], pairs[none, 1]] == 1)
        ec.same_stats(ref_of(pkg, ol, e, M, law, nomp(b), kw, b)["stats"], got["nominal"])
        for s, n in enumerate(b.n_knots):
            assert np.all(got["X_sim"][s, :, n:] == 0) and np.all(got["X_hat"][s, :, n - 1:] == 0)
        np.testing.assert_allclose(got["filt_final"][pairs[none, 0], pairs[none, 1]],
                                   np.broadcast_to(first_record(kw["filt"]), (len(none), FILTER_W)), rtol=1e-15, atol=0)
        four = tiny[ref["n_knots"][tiny] == 4]
        assert np.all(got["filt_final"][pairs[four, 0], pairs[four, 1], 3:6] < kw["filt"]["p0_att"]), "the update at k = 2 was not made"
        # y_0 is the first sample whatever the latency; y_1 of a 3-knot slew is the model's prediction from it, rate included
        r0 = ref_of(pkg, ol, e, M, law, pairs, dict(kw, latency=0), b)
        assert np.array_equal(ref["X_hat"][:, 0], r0["X_hat"][:, 0])
        three = tiny[ref["n_knots"][tiny] == 3]
        assert np.all(np.any(ref["X_hat"][three, 1, 0:3] != ref["X_hat"][three, 0, 0:3], axis=1))


# ---- the long horizon ---------------------------------------------------------------------------------------------------------

LONG_SIGMA_W = 1e-4


def long_case(pkg, ol, N, M):
    """``mag_filtered_common.long_case``'s recipe (T = 1, the PD law regulating on the model's plant with plant noise, 0.38 deg/s
    gyro noise, 5e-7 T magnetometer noise, a gyro bias of GYRO_BIAS in a drawn direction, latency 0) behind this filter: sigma_w =
    LONG_SIGMA_W, sigma_v = sigma_u = 0, sigma_g the sensor's, p0_att = 1 deg, p0_bias = GYRO_BIAS. Returns the case with its
    reference (``ref``), the mag filter's on the same draws (``mag``) and gyro dead reckoning's (``dead``)"""
    c = gfc.long_case(pkg, ol, N, M)
    tr = pkg.tracking
    filt = dict(sigma_v=0.0, sigma_w=LONG_SIGMA_W, sigma_u=0.0, sigma_g=tr.SENSOR_SIGMA_GYRO, sigma_m=sc.SIGMAS["sigma_mag"],
                p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=GYRO_BIAS)
    kw = dict(c["kw"], filt=filt)
    ref = pairs_of(ol, pkg._abi, "pd", c["b"], c["x0s"], (sc.KD, sc.KP), c["o"], c["pairs"], **kw)
    return dict(c, kw=kw, ref=ref, mag=c["ref"])


def assert_filter_works(c):
    """on the references alone, rms over the last half of the horizon: the rate error of the estimate is below 0.25 x the raw
    sample's (the model filter's own bar); the attitude error is below gyro dead reckoning's on every realisation; its mean is no
    worse than 1.10 x the mag filter's on the same draws; |b^ - b_w| at the end is below GYRO_BIAS on every realisation"""
    ref, N = c["ref"], c["b"].N
    half = slice(N // 2, N - 1)
    we, wr = [], []
    for i in range(len(c["pairs"])):
        true = ref["X_sim"][i, half]
        we.append(np.mean(np.sum((ref["X_hat"][i, half, 0:3] - true[:, 0:3]) ** 2, axis=1)))
        wr.append(np.mean(np.sum((ref["Y_raw"][i, half, 0:3] - true[:, 0:3]) ** 2, axis=1)))
    we, wr = math.sqrt(float(np.mean(we))), math.sqrt(float(np.mean(wr)))
    est, mag, dead = (gfc.rms_attitude_error(c[k], N) for k in ("ref", "mag", "dead"))
    db = np.array([float(np.linalg.norm(ref["filt_final"][i, 0:3] - c["sensor"][t, m, 0:3])) for i, (t, m) in enumerate(c["pairs"])])
    deg = np.degrees
    print(f"rms over the last half: rate error of the estimate {we:.2e} rad/s against the raw sample's {wr:.2e}: ratio {we / wr:.3f}; "
          f"attitude error, deg: this filter {deg(est).min():.2f} .. {deg(est).max():.2f} (mean {deg(est).mean():.2f}), the mag filter "
          f"{deg(mag).min():.2f} .. {deg(mag).max():.2f} (mean {deg(mag).mean():.2f}), dead reckoning {deg(dead).min():.2f} .. "
          f"{deg(dead).max():.2f} (mean {deg(dead).mean():.2f}); |b^ - bw| {db.min():.2e} .. {db.max():.2e} against {GYRO_BIAS:.1e}")
    assert np.isfinite(ref["X_hat"]).all() and np.isfinite(ref["filt_final"]).all()
    assert we < 0.25 * wr, "the filter does not smooth the gyro noise"
    assert np.all(est < dead), "the filter loses to gyro dead reckoning on a realisation"
    assert est.mean() <= 1.10 * mag.mean(), "the attitude estimate is worse than the mag filter's"
    assert np.all(db < GYRO_BIAS), "the filter does not estimate the gyro bias"
