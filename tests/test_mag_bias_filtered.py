"""CPU tier of the ensemble controllers behind the magnetometer-updated filter that estimates the magnetometer bias
(tsat_tvlqr_ensemble_mag_bias_filtered, tsat_pd_ensemble_mag_bias_filtered): the block recursion of the reference against the same
step with a full 9 x 9 covariance, the reference of tests/mag_bias_filtered_common.py pinned to the sensed reference with the filter
off, a zero field row, the kernel source of tortoisesat.jl_amd/csrc/tsat_mag_bias_filtered.hpp under the lane emulator against the
reference (X_sim, X_hat, filt_final to 1e-9; stats, n_clipped, summary as tests/test_sensed.py compares them), its reduction to the
emulated mag-filtered parents at p0_mag = sigma_c = 0, f = NULL against the emulated sensed parents, what the calls reject (the
library's own check_mag_bias_filter) and the host layers.

The case is tests/test_mag_filtered.py's: ``pd_common.case`` (8 slews, N = 20, ragged horizons) at M = 5, all five plant dispersions,
plant noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels sensed_common.SIGMAS / BIAS,
filter levels mag_bias_filtered_common.MBFILT."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import filtered_common as fc
import gg_common as gc
import mag_bias_filtered_common as mb
import mag_filtered_common as mc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

M = 5
KINDS = ("track", "track_ff", "regulate")
N_COND = 4


@pytest.fixture(scope="module")
def emu(pkg):
    return mb.EmuMagBiasFiltered(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the 8 slews, their plan and gains from the oracle, M = 5 realisations; computed once and left unchanged"""
    b, Rtab = pc.case(pkg)
    r = ol.solve_batch(b, hc.solve_options(ol))
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    pairs = dc.all_pairs(b.T, M)
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=(Qd, Qfd, Rd), K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, M),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, M), pairs=pairs)


def _tv_kw(cs, sat=hc.SAT, **over):
    kw = dict(Rtab=cs["Rtab"], gm=gc.GM, plant=cs["plant"], sat=sat, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"], filt=mb.MBFILT)
    kw.update(over)
    return kw


def _pd_kw(cs, kind, mode, **over):
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"], gm=gc.GM,
              plant=cs["plant"], sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], sens=sc.SIGMAS, latency=0, sensor=cs["sensor"],
              filt=mb.MBFILT)
    kw.update(over)
    return kw


def _tv_ref(pkg, ol, cs, pairs, kw):
    return mb.pairs_of(ol, pkg._abi, "tv", cs["b"], cs["x0s"], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **kw)


def _pd_ref(pkg, ol, cs, pairs, kw):
    return mb.pairs_of(ol, pkg._abi, "pd", cs["b"], cs["x0s"], (sc.KD, sc.KP), cs["o"], pairs, **kw)


def _tv_emu(emu, cs, kw):
    return emu.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **kw)


def _pd_emu(emu, cs, kw):
    return emu.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **kw)


def _nomp(b):
    return np.array([(t, -1) for t in range(b.T)])


def _cond_pairs(cs):
    """the first N_COND pairs of full horizon: the conditions are shown on a part of the pairs, they hold on all"""
    full = cs["pairs"][ec.horizons(cs["b"])[cs["pairs"][:, 0]] == cs["b"].N]
    return full[:: max(1, len(full) // N_COND)][:N_COND]


def _record(rng, ol, filt):
    """a filter one step after its first sample, then every block overwritten by a consistent random covariance: P = L L^T"""
    e = mb.MagBiasEkf(ol, 0.2, filt)
    q0 = rng.standard_normal(4)
    e.first(0.02 * rng.standard_normal(3), q0)
    s = np.r_[np.full(3, 2e-2), np.full(3, 2e-3), np.full(3, 1.5e-6)]
    L = np.tril(rng.standard_normal((9, 9))) * s[:, None]
    P = L @ L.T
    e.A, e.B, e.E = fc._sym(P[0:3, 0:3]), P[0:3, 3:6].copy(), P[0:3, 6:9].copy()
    e.D, e.F, e.M = fc._sym(P[3:6, 3:6]), P[3:6, 6:9].copy(), fc._sym(P[6:9, 6:9])
    e.b, e.c = 1e-3 * rng.standard_normal(3), 1e-6 * rng.standard_normal(3)
    return e


def _full_P(e):
    return np.block([[e.A, e.B, e.E], [e.B.T, e.D, e.F], [e.E.T, e.F.T, e.M]])


def test_block_recursion_is_the_full_nine_state_step(ol):
    """one step of ``MagBiasEkf`` against the same step written with a full 9 x 9 P: F = [[Phi, -hI, 0], [0, I, 0], [0, 0, I]],
    P- = F P F^T + Q, Hf = [H 0 I], K = P- Hf^T S^-1, x += K z, P = P- - K S K^T. Bar: 1e-14 relative — the states to their own
    largest entry, a covariance block to the largest entry of its PRIOR (the two differ in the order of a few dozen sums and in the
    3 x 3 inverse: units of 2^-53 = 1.1e-16 per operand, and the operands of P- - K S K^T are of the prior's size)"""
    ol.load()
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(10):
        e = _record(rng, ol, mb.MBFILT)
        w1, bm, r = 0.02 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3)
        f, h, I, Z = e.f, e.h, np.eye(3), np.zeros((3, 3))
        P, q, b, c, w = _full_P(e), e.q.copy(), e.b.copy(), e.c.copy(), e.w.copy()
        d = fc.dq_of(h * w)
        qm = ol.qmult(q, d)
        V = fc._skew(d[1:4])
        Phi = (I + 2 * d[0] * V + 2 * V @ V).T
        Fm = np.block([[Phi, -h * I, Z], [Z, I, Z], [Z, Z, I]])
        Q = np.diag(np.r_[np.full(3, (f["sigma_v"] * h) ** 2), np.full(3, f["sigma_u"] ** 2), np.full(3, f["sigma_c"] ** 2)])
        Pm = Fm @ P @ Fm.T + Q
        n = qm / math.sqrt(float(qm @ qm))
        Hf = np.hstack([mc.h_matrix(n, r), Z, I])
        z = bm - c - ol.qrot(n, r)
        S = Hf @ Pm @ Hf.T + f["sigma_m"] ** 2 * I
        K = Pm @ Hf.T @ np.linalg.inv(S)
        dx = K @ z
        Pp = Pm - K @ S @ K.T
        qp = ol.qmult(qm, np.r_[1.0, dx[0:3] / 2])
        e.step(w1, bm, r)
        want = dict(q=qp / np.linalg.norm(qp), b=b + dx[3:6], c=c + dx[6:9], w=w1 - (b + dx[3:6]), A=Pp[0:3, 0:3], B=Pp[0:3, 3:6],
                    E=Pp[0:3, 6:9], D=Pp[3:6, 3:6], F=Pp[3:6, 6:9], M=Pp[6:9, 6:9])
        prior = dict(A=Pm[0:3, 0:3], B=Pm[0:3, 3:6], E=Pm[0:3, 6:9], D=Pm[3:6, 3:6], F=Pm[3:6, 6:9], M=Pm[6:9, 6:9])
        for k, v in want.items():
            # a covariance block is P- - K S K^T, the difference of two matrices of the prior's size that each carry their own
            # rounding: the difference is held to 1e-14 of the prior block, the size of what was rounded
            rel = float(np.max(np.abs(getattr(e, k) - v)) / np.max(np.abs(prior.get(k, v))))
            worst = max(worst, rel)
            assert rel < 1e-14, (k, rel)
    print(f"block recursion against the full 9 x 9 step: worst relative difference {worst:.1e}")


def test_reference_with_the_filter_off_is_the_sensed_reference(pkg, ol, cs):
    """the anchor: ``mag_bias_filtered_common.pairs_of`` with filt = None is ``sensed_common.pairs_of``, max |d| = 0, both laws and
    both latencies, the nominal slot included"""
    b = cs["b"]
    pairs = np.concatenate([cs["pairs"][::7], _nomp(b)[:2]])
    for latency in (0, 1):
        kw = _tv_kw(cs, latency=latency, filt=None)
        skw = {k: v for k, v in kw.items() if k != "filt"}
        old = sc.pairs_of(ol, pkg._abi, "tv", b, cs["x0s"], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **skw)
        new = _tv_ref(pkg, ol, cs, pairs, kw)
        d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
        print(f"TVLQR reference with the filter off against sensed_common.pairs_of, latency {latency}: max|d| {d:.1e}")
        assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
        assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
        assert not new["X_hat"].any() and not new["filt_final"].any() and new["filt_final"].shape[1] == 15
        for kind, mode in (("track_ff", 0), ("regulate", 1), ("track", 0)):
            kw = _pd_kw(cs, kind, mode, latency=latency, filt=None)
            skw = {k: v for k, v in kw.items() if k != "filt"}
            old = sc.pairs_of(ol, pkg._abi, "pd", b, cs["x0s"], (sc.KD, sc.KP), cs["o"], pairs, **skw)
            new = _pd_ref(pkg, ol, cs, pairs, kw)
            d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
            print(f"PD reference ({kind}, mode {mode}) with the filter off against sensed_common.pairs_of, latency {latency}: max|d| {d:.1e}")
            assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])


def test_reference_without_a_bias_state_is_the_mag_filter(ol):
    """p0_mag = sigma_c = 0 in the reference: c^, E, F and M stay exactly zero and the step is ``MagEkf``'s to 1e-15 relative"""
    ol.load()
    rng = np.random.default_rng(4)
    filt = dict(mb.MBFILT, p0_mag=0.0, sigma_c=0.0)
    a, p = mb.MagBiasEkf(ol, 0.2, filt), mc.MagEkf(ol, 0.2, mc.MFILT)
    w0, q0 = 0.02 * rng.standard_normal(3), rng.standard_normal(4)
    a.first(w0, q0)
    p.first(w0, q0)
    for _ in range(5):
        w1, bm, r = 0.02 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3)
        a.step(w1, bm, r)
        p.step(w1, bm, r)
        assert not a.c.any() and not a.E.any() and not a.F.any() and not a.M.any()
        for k in ("q", "b", "w", "A", "B", "D"):
            assert np.max(np.abs(getattr(a, k) - getattr(p, k))) <= 1e-15 * np.max(np.abs(getattr(p, k))), k


def test_a_zero_row_observes_the_magnetometer_bias(ol):
    """a step against r = 0: H = 0, so the attitude block of the gain is E- S^-1 alone and z = b_m - c^ observes c directly — no
    longer a no-op. With E = F = 0 besides (a fresh filter) the attitude and the gyro bias stay at the propagated ones while c^
    moves towards b_m by M- (M- + sigma_m^2 I)^-1 and M shrinks; everything stays finite"""
    ol.load()
    rng = np.random.default_rng(9)
    w0, q0 = 0.02 * rng.standard_normal(3), rng.standard_normal(4)
    w1, bm = 0.02 * rng.standard_normal(3), 2.5e-6 * rng.standard_normal(3)
    e = mb.MagBiasEkf(ol, 0.2, mb.MBFILT)
    e.first(w0, q0)
    e.step(w1, bm, np.zeros(3))
    qm, Am, Bm, Dm, Em, Fm, Mm = e.prior
    assert np.array_equal(e.q, qm / math.sqrt(float(qm @ qm))) and not e.b.any() and np.array_equal(e.w, w1)
    assert np.array_equal(e.A, fc._sym(Am)) and np.array_equal(e.B, Bm) and np.array_equal(e.D, fc._sym(Dm))
    m, s = mb.MBFILT["p0_mag"] ** 2 + mb.MBFILT["sigma_c"] ** 2, mb.MBFILT["sigma_m"] ** 2
    np.testing.assert_allclose(e.c, bm * m / (m + s), rtol=1e-13)
    np.testing.assert_allclose(np.diag(e.M), np.full(3, m - m * m / (m + s)), rtol=1e-12)
    assert np.max(np.abs(e.c)) > 1e-7, "the zero row must move c^, or the test shows nothing"
    # with every block at work the zero row moves the attitude too, through E-
    e2 = _record(np.random.default_rng(2), ol, mb.MBFILT)
    q_before = e2.q.copy()
    e2.step(w1, bm, np.zeros(3))
    qm = e2.prior[0]
    assert np.max(np.abs(e2.q - qm / math.sqrt(float(qm @ qm)))) > 1e-9 and np.isfinite(e2.final()).all() and np.isfinite(q_before).all()


def _check_against(pkg, ol, cs, ref, got, pairs, keep, nom_ref):
    b = cs["b"]
    dc.compare(ref, got, pairs, keep)
    mb.compare_estimates(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
    ec.same_stats(nom_ref["stats"], got["nominal"])


def _parity(pkg, ol, emu, cs, law, kw, with_conditions=True, prediction=None, skip=()):
    """every pair of 8 x 5 that is off the thresholds (at most 2 may sit on one), and stats_nominal; the conditions first, on
    references alone, over N_COND pairs of full horizon"""
    b, pairs = cs["b"], cs["pairs"]
    ref_of, run = (_tv_ref, _tv_emu) if law == "tv" else (_pd_ref, _pd_emu)
    ref = ref_of(pkg, ol, cs, pairs, kw)
    o = cs["o"]
    ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], o.min_steps, o.w_tol, o.angle_tol) > dc.MARGIN
                   for i in range(len(pairs))])
    assert np.count_nonzero(~ok) <= 2, "more than 2 of the 40 realisations sit on a threshold"
    keep = np.flatnonzero(ok)
    if with_conditions:
        cp = _cond_pairs(cs)
        mb.conditions(lambda **o_: ref_of(pkg, ol, cs, cp, dict(kw, **o_)), kw["sensor"], filt=kw["filt"],
                      prediction=(law == "tv") if prediction is None else prediction, pairing=False, skip=skip)
    got = run(emu, cs, kw)
    _check_against(pkg, ol, cs, ref, got, pairs, keep, ref_of(pkg, ol, cs, _nomp(b), kw))
    return ref, got, keep


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
def test_emulated_tvlqr_matches_reference(pkg, ol, emu, cs, limits, latency):
    """8 slews x M = 5, limits +-0.6 and +-25, latency 0 and 1"""
    kw = _tv_kw(cs, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = _parity(pkg, ol, emu, cs, "tv", kw)
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_pd_matches_reference(pkg, ol, emu, cs, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation under +-0.6 sits
    on its limits at every knot (tests/test_sensed.py): it is compared under +-0.6 AND under +-25, and asserts its conditions there"""
    kw = _pd_kw(cs, kind, mode, latency=latency)
    if kind == "regulate":
        ref, _, keep = _parity(pkg, ol, emu, cs, "pd", kw, with_conditions=False)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    _parity(pkg, ol, emu, cs, "pd", kw)


@pytest.mark.parametrize("kind", ["track_ff", "regulate"])
def test_emulated_pd_prediction_across_the_delay(pkg, ol, emu, cs, kind):
    """the PD law at latency 1 with the body rate FAST added to the starts, limits +-25: the case on which the prediction across the
    delay shows under this law; every condition, then parity"""
    c2 = dict(cs, x0s=cs["x0s"] + np.r_[mb.FAST, np.zeros(4)])
    _parity(pkg, ol, emu, c2, "pd", _pd_kw(c2, kind, 0, latency=1, sat=pc.WIDE), prediction=True)


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_delayed_sample_is_paired_with_its_own_row(pkg, ol, emu, cs, law):
    """latency 1 on ``mag_filtered_common.fast_table``, tables whose rows turn 25 deg from one to the next: there the row the delayed
    sample is updated against moves the final state; the condition on references alone, then parity"""
    c2 = dict(cs, b=mb.fast_table(cs["b"]))
    kw = _tv_kw(c2, latency=1, sat=pc.WIDE) if law == "tv" else _pd_kw(c2, "track_ff", 0, latency=1, sat=pc.WIDE)
    ref_of = _tv_ref if law == "tv" else _pd_ref
    cp = _cond_pairs(c2)
    pc.differs(ref_of(pkg, ol, c2, cp, kw), ref_of(pkg, ol, c2, cp, dict(kw, pair_own_row=False)), "the delayed sample against r_{k-1}, not r_k")
    _parity(pkg, ol, emu, c2, law, kw, with_conditions=False)


def test_emulated_reduction_to_the_mag_filter(pkg, emu, cs):
    """p0_mag = sigma_c = 0: the emulated call equals the emulated mag-filtered call on X_sim, X_hat and filt_final[0:9] to 1e-12
    (byte equality is not demanded: contraction may differ), and filt_final[9:15] is exactly 0. Both laws, both latencies"""
    parent = mc.EmuMagFiltered(pkg._abi)
    off = dict(mb.MBFILT, p0_mag=0.0, sigma_c=0.0)
    worst = 0.0
    for latency in (0, 1):
        for new, old in ((_tv_emu(emu, cs, _tv_kw(cs, latency=latency, filt=off)),
                          parent.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **_tv_kw(cs, latency=latency, filt=mc.MFILT))),
                         (_pd_emu(emu, cs, _pd_kw(cs, "track_ff", 1, latency=latency, filt=off)),
                          parent.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **_pd_kw(cs, "track_ff", 1, latency=latency, filt=mc.MFILT)))):
            d = max(float(np.max(np.abs(new["X_sim"] - old["X_sim"]))), float(np.max(np.abs(new["X_hat"] - old["X_hat"]))),
                    float(np.max(np.abs(new["filt_final"][..., 0:9] - old["filt_final"]))))
            worst = max(worst, d)
            assert np.all(new["filt_final"][..., 9:15] == 0.0)
    print(f"reduction to the emulated mag-filtered calls at p0_mag = sigma_c = 0: max difference {worst:.1e}")
    assert worst < 1e-12
    # with the bias state on the run is another one: the reduction is not vacuous
    on = _tv_emu(emu, cs, _tv_kw(cs))
    assert np.max(np.abs(on["X_sim"] - _tv_emu(emu, cs, _tv_kw(cs, filt=off))["X_sim"])) >= gc.MOVED


def _same(a, c, keys=("X_sim", "stats", "summary", "nominal", "n_clipped")):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_null_filter_is_byte_equal_to_the_emulated_sensed_parents(pkg, emu, cs):
    """f = NULL dispatches to the sensed call: byte for byte its outputs, both laws, both latencies, with and without gravity rows"""
    old = sc.EmuSensed(pkg._abi)
    for latency in (0, 1):
        for rt, gm in ((cs["Rtab"], gc.GM), (None, 0.0)):
            kw = _tv_kw(cs, latency=latency, Rtab=rt, gm=gm, filt=None)
            skw = {k: v for k, v in kw.items() if k != "filt"}
            new = _tv_emu(emu, cs, kw)
            _same(old.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **skw), new)
            assert new["X_hat"] is None and new["filt_final"] is None
            assert np.max(np.abs(new["X_sim"] - _tv_emu(emu, cs, dict(kw, filt=mb.MBFILT))["X_sim"])) >= gc.MOVED
            for kind, mode in (("track_ff", 0), ("regulate", 1)):
                kw = _pd_kw(cs, kind, mode, latency=latency, Rtab=rt, gm=gm, filt=None)
                skw = {k: v for k, v in kw.items() if k != "filt"}
                _same(old.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **skw), _pd_emu(emu, cs, kw))


def test_estimates_requested_or_not_do_not_change_the_run(pkg, emu, cs):
    for latency in (0, 1):
        kw = _tv_kw(cs, latency=latency)
        _same(_tv_emu(emu, cs, kw), _tv_emu(emu, cs, dict(kw, estimates=False)))
        kw = _pd_kw(cs, "track_ff", 1, latency=latency)
        _same(_pd_emu(emu, cs, kw), _pd_emu(emu, cs, dict(kw, estimates=False)))


def test_rejected_arguments(pkg, emu, cs):
    """check_mag_bias_filter, the validation function both entry points add to their sensed parents', through the emulator driver;
    the drivers refuse what it refuses and what the parents refuse; f = NULL with an output asked for is refused by the entry points
    before anything else, with its text"""
    b = cs["b"]
    good = mb.PdCall(pkg._abi, b, cs["o"], cs["x0s"], sc.KD, sc.KP, **_pd_kw(cs, "track_ff", 0))
    tv = mb.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], K=cs["K"], **_tv_kw(cs))
    pd_fn, tv_fn = emu.lib.emu_pd_ensemble_mag_bias_filtered, emu.lib.emu_tvlqr_ensemble_mag_bias_filtered
    assert emu.check(good) == (0, "")
    assert emu.check(good.edit(f=None)) == (-1, "null filter options")
    assert pd_fn(*good.c_args()) == 0 and tv_fn(*tv.c_args(emu=True)) == 0
    for label, call, words in mb.filter_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert pd_fn(*call.c_args()) == -1, label
    for label, call, words in mb.filter_rejections(tv):
        assert tv_fn(*call.c_args(emu=True)) == -1, label
    # what the sensed parents reject is still rejected
    for label, call, words in sc.sensor_rejections(good):
        assert pd_fn(*call.c_args()) == -1, label
    for label, call, words in sc.sensor_rejections(tv):
        assert tv_fn(*call.c_args(emu=True)) == -1, label
    assert pd_fn(*good.edit(limit_mode=3).c_args()) == -1
    assert tv_fn(*tv.edit(Rtab=None).c_args(emu=True)) == -1          # gm != 0 needs the table
    # f = NULL with X_hat or filt_final
    for call, fn, kw in ((good, pd_fn, {}), (tv, tv_fn, dict(emu=True))):
        assert fn(*call.edit(f=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None, filt_final=None).c_args(**kw)) == 0
    # the entry points: a code and a text, not a crash
    lib = pkg._abi.load()
    for fn, call in ((lib.tsat_pd_ensemble_mag_bias_filtered, good), (lib.tsat_tvlqr_ensemble_mag_bias_filtered, tv)):
        assert fn(None, *call.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, filt_final=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, X_hat=None, filt_final=None).c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_mag_bias_filter_options_and_host_layers(pkg):
    """the header, ``_abi``, the wrappers and this tier's constants agree"""
    tr, abi = pkg.tracking, pkg._abi
    lib = abi.load()
    deg = math.pi / 180.0
    names = ["sigma_v", "sigma_u", "sigma_m", "sigma_c", "p0_att", "p0_bias", "p0_mag"]
    assert C.sizeof(abi.MagBiasFilterOptions) == 64
    assert [(n, C.sizeof(t)) for n, t in abi.MagBiasFilterOptions._fields_] == [(n, 8) for n in names] + [("reserved", 4)]
    fo = abi.MagBiasFilterOptions(9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 7)
    lib.tsat_mag_bias_filter_default_options(C.byref(fo))
    # the mag filter's defaults, sigma_m left 0, no bias state
    ref = abi.MagFilterOptions()
    lib.tsat_mag_filter_default_options(C.byref(ref))
    assert (fo.sigma_v, fo.sigma_u, fo.sigma_m, fo.p0_att, fo.p0_bias) == (ref.sigma_v, ref.sigma_u, 0.0, ref.p0_att, ref.p0_bias)
    assert (fo.sigma_c, fo.p0_mag, fo.reserved) == (0.0, 0.0, 0) and (fo.sigma_v, fo.p0_att) == (tr.SENSOR_SIGMA_GYRO, deg)
    lib.tsat_mag_bias_filter_default_options(None)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    body = re.search(r"struct tsat_mag_bias_filter_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", n) for n in names] + [("int32_t", "reserved")]
    assert re.search(r"#define TSAT_MAG_BIAS_FILTER_W 15\b", hdr) and tr.MAG_BIAS_FILTER_W == 15 == mb.FILTER_W
    for name in ("tsat_mag_bias_filter_default_options", "tsat_tvlqr_ensemble_mag_bias_filtered", "tsat_pd_ensemble_mag_bias_filtered"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
    # the prototypes are the mag-filtered parents' with the options struct exchanged
    for law in ("tvlqr", "pd"):
        p, f = abi.PROTOTYPES[f"tsat_{law}_ensemble_mag_filtered"], abi.PROTOTYPES[f"tsat_{law}_ensemble_mag_bias_filtered"]
        assert f[0] is p[0] and len(f[1]) == len(p[1]) and f[1][:-3] == p[1][:-3] and f[1][-2:] == p[1][-2:]
        assert f[1][-3]._type_ is abi.MagBiasFilterOptions
    # the statements the headers have to make
    for text in (hdr, open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_mag_bias_filtered.hpp")).read()):
        assert "[H 0 I]" in text and "r_{k-1}" in text and "NO LONGER A NO-OP" in text and "E- = Phi E - h F" in text
    # mag_bias_filter_options
    fo = tr.mag_bias_filter_options(1e-3, 5e-7)
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [1e-3, 0.0, 5e-7, 0.0, deg, 0.0, 0.0, 0]
    fo = tr.mag_bias_filter_options(1e-3, 5e-7, sigma_u=3e-5, sigma_c=2e-8, p0_att=4e-2, p0_bias=5e-3, p0_mag=1.5e-6)
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [1e-3, 3e-5, 5e-7, 2e-8, 4e-2, 5e-3, 1.5e-6, 0]
    assert isinstance(fo, abi.MagBiasFilterOptions)
    assert list(inspect.signature(tr.mag_bias_filter_options).parameters) == ["sigma_v", "sigma_m", "sigma_u", "sigma_c", "p0_att", "p0_bias",
                                                                             "p0_mag"]
    for bad in (dict(sigma_v=-1.0, sigma_m=1.0), dict(sigma_v=1.0, sigma_m=0.0), dict(sigma_v=1.0, sigma_m=1.0, sigma_u=-1.0),
                dict(sigma_v=1.0, sigma_m=1.0, sigma_c=-1.0), dict(sigma_v=1.0, sigma_m=1.0, p0_att=-1.0),
                dict(sigma_v=1.0, sigma_m=1.0, p0_bias=-1.0), dict(sigma_v=1.0, sigma_m=1.0, p0_mag=-1.0),
                dict(sigma_v=1.0, sigma_m=1.0, p0_mag=float("inf")), dict(sigma_v=1.0, sigma_m=float("nan"))):
        with pytest.raises(ValueError):
            tr.mag_bias_filter_options(**bad)
    # the two calls take the arguments of the mag-filtered wrappers
    for new, old in ((tr.attitude_ensemble_mag_bias_filtered, tr.attitude_ensemble_mag_filtered),
                     (tr.attitude_ensemble_pd_mag_bias_filtered, tr.attitude_ensemble_pd_mag_filtered)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
        assert inspect.signature(new).parameters["want_estimates"].default is False
    fo, Xh, ff = tr._mag_bias_filtering(2, 3, 5, fo, True)
    assert Xh.shape == (2, 3, 5, 7) and ff.shape == (2, 3, 15)
    assert tr._mag_bias_filtering(2, 3, 5, fo, False)[1] is None
    for bad in (None, tr.mag_filter_options(1e-3, 5e-7)):       # sigma_m has no default; another filter's options are not these
        with pytest.raises(ValueError):
            tr._mag_bias_filtering(2, 3, 5, bad, False)
