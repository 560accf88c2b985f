"""CPU tier of the ensemble controllers behind the magnetometer-updated model filter with a sun sensor that eclipse blinds
(tsat_tvlqr_ensemble_model_mag_sun_filtered, tsat_pd_ensemble_model_mag_sun_filtered): the restated reference loop of
tests/model_mag_sun_filtered_common.py pinned to ``model_mag_filtered_common.pairs_of`` with the sun table None or all zero (max |d|
= 0) and one update a, b, c by blocks pinned to a full 9 x 9 update; the kernel source of
tortoisesat.jl_amd/csrc/tsat_model_mag_sun_filtered.hpp under the lane emulator against the reference (X_sim, X_hat, filt_final to
1e-9; stats, n_clipped, summary as tests/test_sensed.py compares them); tiny horizons at latency 1; a table dark throughout, Stab =
None and f = None against the emulated parents (difference 0, equal bytes); the pairing of the delayed sun sample; realisations that
do not depend on M; two wavefronts with every realisation compared; what the calls reject (the library's own check functions) and
the host layers.

The case, its sun tables and what each slew's updates see are described in tests/model_mag_sun_filtered_common.py. Every parity test
prints every figure of its conditions (bar gg_common.MOVED on the final states, on references alone) before the kernels run."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mag_filtered_common as gfc
import model_filtered_common as mfc
import model_mag_filtered_common as mc
import model_mag_sun_filtered_common as uc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

MS = (63, 64)


@pytest.fixture(scope="module")
def emu(pkg):
    return uc.EmuModelMagSunFiltered(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the 8 slews, their plan and gains from the oracle, 70 realisations, the sun tables; computed once and left unchanged"""
    b, Rtab = pc.case(pkg)
    r = ol.solve_batch(b, hc.solve_options(ol))
    W = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], *W, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 70, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=W, K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 70),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, 70), Stab=uc.sun_table(b))


@pytest.fixture(scope="module")
def run(emu):
    """the tier's call: the emulated kernels"""
    def call(law, e, M, kw, batch=None, **more):
        b = batch or e["b"]
        if law == "tv":
            return emu.tv(b, e["o"], e["X"], e["U"], *e["W"], uc.cut(e["x0s"], M), e["K"], **kw, **more)
        return emu.pd(b, e["o"], uc.cut(e["x0s"], M), sc.KD, sc.KP, **kw, **more)
    return call


@pytest.fixture(scope="module")
def run_parent(pkg):
    """the emulated model-mag-filtered kernels, on this family's keyword arguments less the sun's"""
    old = mc.EmuModelMagFiltered(pkg._abi)

    def call(law, e, M, kw, batch=None):
        b, kw = batch or e["b"], uc.parent_kw(kw)
        if law == "tv":
            return old.tv(b, e["o"], e["X"], e["U"], *e["W"], uc.cut(e["x0s"], M), e["K"], **kw)
        return old.pd(b, e["o"], uc.cut(e["x0s"], M), sc.KD, sc.KP, **kw)
    return call


def _laws(cs, M, latency, **over):
    return (("tv", uc.tv_kw(cs, M, latency=latency, **over)), ("pd", uc.pd_kw(cs, "track_ff", 0, M, latency=latency, **over)),
            ("pd", uc.pd_kw(cs, "regulate", 1, M, latency=latency, **over)), ("pd", uc.pd_kw(cs, "track", 0, M, latency=latency, **over)))


def test_the_inputs_of_the_case(cs):
    """every sun direction is at least 20 deg from every field row of its table; rows are exactly zero or exactly the direction;
    the two eclipse windows are in different places; every compared slew that makes six updates has three lit and three dark"""
    b, S = cs["b"], cs["Stab"]
    assert S.shape == (b.Btab.shape[0], b.n_tab, 3)
    s = uc.sun_directions(b)
    for i in range(S.shape[0]):
        a = uc.angle_to_rows(s[i], b.Btab[i, :b.n_tab])
        print(f"table {i}: the sun direction is {math.degrees(a):.1f} deg from the nearest field row")
        assert a >= uc.MIN_ANGLE and abs(np.linalg.norm(s[i]) - 1.0) < 1e-15
        dark = ~np.any(S[i] != 0, axis=1)
        assert np.array_equal(S[i][~dark], np.broadcast_to(s[i], (int(np.count_nonzero(~dark)), 3)))
        assert list(np.flatnonzero(dark)) == list(range(uc.DARK_ROWS[i][0], uc.DARK_ROWS[i][1] + 1))
    assert uc.DARK_ROWS[0] != uc.DARK_ROWS[1]
    for latency in (0, 1):
        uc.assert_lit_and_dark(b, S, dc.sampled_pairs(b.T, 64)[:, 0], latency)
    assert [uc.updates_of(b, S, t, 0)[1] for t in (0, 4)] == [6, 4]      # knots 6 .. 11 of table 0's slews, 2 .. 5 of table 1's


def test_reference_without_a_sun_table_is_the_parents_reference(pkg, ol, cs):
    """the anchor: the restated loop with the sun table None, and with it all zero, is ``model_mag_filtered_common.pairs_of``, max
    |d| = 0 on every output: both laws, both latencies, the nominal slot included; and with filt = None the sensed reference"""
    b, M = cs["b"], 5
    pairs = np.concatenate([dc.all_pairs(b.T, M)[::7], uc.nomp(b)[:2]])
    zero = np.zeros_like(cs["Stab"])
    for latency in (0, 1):
        for law, kw in _laws(cs, M, latency):
            old = mc.ref_of(pkg, ol, cs, M, law, pairs, uc.parent_kw(kw))
            for label, over in (("None", dict(Stab=None, sigma_sun=0.0)), ("all zero", dict(Stab=zero))):
                new = uc.ref_of(pkg, ol, cs, M, law, pairs, dict(kw, **over))
                d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_sim", "X_hat", "filt_final", "U_cmd", "Y_raw"))
                print(f"{law} reference with the sun table {label} against the parent's, latency {latency}: max|d| {d:.1e}")
                assert d == 0.0 and np.array_equal(old["stats"], new["stats"])
                assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
            assert uc.moved(old, uc.ref_of(pkg, ol, cs, M, law, pairs, kw)) >= gc.MOVED, "the sun table must move the case"
        law, kw = _laws(cs, M, latency, filt=None)[0]
        raw = uc.ref_of(pkg, ol, cs, M, law, pairs, kw)
        skw = {k: v for k, v in kw.items() if k not in ("filt", "Stab", "sigma_sun")}
        old = sc.pairs_of(ol, pkg._abi, "tv", b, cs["x0s"][:, :M], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **skw)
        assert float(np.max(np.abs(old["X_sim"] - raw["X_sim"]))) == 0.0 and not raw["X_hat"].any()


def _worked_record(ol, rng):
    """a ModelMagSunEkf whose every block is at work: ``first`` and a dense symmetric positive definite P"""
    J = np.diag([0.04, 0.05, 0.02]) + 1e-3 * np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0.0]])
    e = uc.ModelMagSunEkf(ol, 0.2, J, 1e-2, uc.FILT)
    e.first(0.02 * rng.standard_normal(3), rng.standard_normal(4))
    e.b = 1e-3 * rng.standard_normal(3)
    L = np.diag([2e-2, 2e-2, 2e-2, 5e-3, 5e-3, 5e-3, 2e-3, 2e-3, 2e-3]) @ (np.eye(9) + 0.3 * np.tril(rng.standard_normal((9, 9)), -1))
    e.P = mfc._sym(L @ L.T)
    return e


def test_one_update_by_blocks_is_a_full_nine_state_update(ol):
    """``_mag``, ``_gyro`` and ``_sun`` in this order equal three full 9 x 9 updates without the Joseph form, K = P H^T (H P H^T +
    R)^-1, P <- P - K S K^T, with H = [Hm 0 0], [0 I I] and [Hs 0 0]; the difference is measured and printed, the bar is the
    parent's for the same comparison (1e-14 on the state and relative to each block's size on P). A zero sun row leaves the parent's
    posterior exactly."""
    ol.load()
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(10):
        e = _worked_record(ol, rng)
        r, w_m = 2.5e-5 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)
        s = rng.standard_normal(3)
        s /= np.linalg.norm(s)
        b_m = ol.qrot(e.q, r) + 5e-7 * rng.standard_normal(3)
        s_m = ol.qrot(e.q, s) + uc.SIGMA_SUN * rng.standard_normal(3)
        q, w, b, P = e.q.copy(), e.w.copy(), e.b.copy(), e.P.copy()
        par = mc.ModelMagEkf(ol, 0.2, e.J, 1e-2, mc.FILT)
        par.q, par.w, par.b, par.P = q.copy(), w.copy(), b.copy(), P.copy()
        dark = uc.ModelMagSunEkf(ol, 0.2, e.J, 1e-2, uc.FILT)
        dark.q, dark.w, dark.b, dark.P = q.copy(), w.copy(), b.copy(), P.copy()
        e.update(w_m, b_m, r, s_m, s)
        par.update(w_m, b_m, r)
        dark.update(w_m, b_m, r, None, np.zeros(3))
        for a, c in ((dark.q, par.q), (dark.w, par.w), (dark.b, par.b), (dark.P, par.P)):
            assert np.array_equal(a, c)
        assert np.max(np.abs(e.q - par.q)) > 1e-6, "the sun update must move the estimate, or the test shows nothing"
        Z, I = np.zeros((3, 3)), np.eye(3)
        for H, R, z_of in ((lambda q_: np.hstack([gfc.h_matrix(q_, r), Z, Z]), uc.FILT["sigma_m"] ** 2, lambda q_, w_, b_: b_m - ol.qrot(q_, r)),
                           (lambda q_: np.hstack([Z, I, I]), uc.FILT["sigma_g"] ** 2, lambda q_, w_, b_: w_m - (w_ + b_)),
                           (lambda q_: np.hstack([gfc.h_matrix(q_, s), Z, Z]), uc.FILT["sigma_s"] ** 2, lambda q_, w_, b_: s_m - ol.qrot(q_, s))):
            Hf = H(q)
            S = Hf @ P @ Hf.T + R * I
            K = P @ Hf.T @ np.linalg.inv(S)
            dl = K @ z_of(q, w, b)
            qp = ol.qmult(q, np.r_[1.0, dl[0:3] / 2])
            q, w, b = qp / np.linalg.norm(qp), w + dl[3:6], b + dl[6:9]
            P = P - K @ S @ K.T
        scale = np.sqrt(np.outer(np.diag(P), np.diag(P)))
        d = max(float(np.max(np.abs(e.q - q))), float(np.max(np.abs(e.w - w))), float(np.max(np.abs(e.b - b))), float(np.max(np.abs(e.P - P) / scale)))
        worst = max(worst, d)
    print(f"block update a, b, c against the full 9 x 9 update: max difference {worst:.1e}")
    assert worst < 1e-14


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
@pytest.mark.parametrize("M", MS)
def test_emulated_tvlqr_matches_reference(pkg, ol, run, cs, M, limits, latency):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront"""
    kw = uc.tv_kw(cs, M, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = uc.parity(pkg, ol, run, cs, M, "tv", kw)
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", uc.KINDS)
@pytest.mark.parametrize("M", MS)
def test_emulated_pd_matches_reference(pkg, ol, run, cs, M, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation under +-0.6 sits
    on its limits at every knot (tests/test_sensed.py): it is compared under +-0.6 AND under +-25, and asserts its conditions there"""
    kw = uc.pd_kw(cs, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = uc.parity(pkg, ol, run, cs, M, "pd", kw, skip=None)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    uc.parity(pkg, ol, run, cs, M, "pd", kw)


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_delayed_sun_sample_is_paired_with_its_own_row(pkg, ol, run, cs, law):
    """latency 1 on ``pairing_table`` (sun rows alternately lit and dark), M = 64: at one knot row k - 1 is lit and row k dark, at
    the next the other way round, so a wrong pairing drops an update or feeds in a sample that never existed; that condition on
    the references, then parity"""
    b, S = cs["b"], uc.pairing_table(cs["b"])
    flips = [(bool(np.any(uc.sun_row(b, S, 0, k - 1) != 0)), bool(np.any(uc.sun_row(b, S, 0, k) != 0))) for k in range(2, 18)]
    assert (True, False) in flips and (False, True) in flips
    kw = uc.tv_kw(cs, 64, latency=1, Stab=S) if law == "tv" else uc.pd_kw(cs, "track_ff", 0, 64, latency=1, Stab=S)
    pairs = dc.sampled_pairs(b.T, 64)
    ref = uc.ref_of(pkg, ol, cs, 64, law, pairs, kw)
    keep = gc.kept(ref, cs["o"])
    cp = mc.cond_pairs(cs, ref, pairs, keep)
    d = uc.moved(uc.ref_of(pkg, ol, cs, 64, law, cp, kw), uc.ref_of(pkg, ol, cs, 64, law, cp, dict(kw, sun_own_row=False)))
    print(f"  condition: {uc.SUN_PAIRING}: max|d final state| {d:.2e}")
    assert d >= gc.MOVED
    got = run(law, cs, 64, kw)
    dc.compare(ref, got, pairs, keep)
    uc.compare_estimates(ref, got, pairs, keep)


def test_tiny_horizons_at_latency_1(pkg, ol, run, cs):
    """n_knots = 2, 3 and 4 among the slews at latency 1, M = 64 (model_mag_sun_filtered_common.check_tiny)"""
    b = mc.tiny_batch(cs["b"])
    c2 = dict(cs, K=ol.tvlqr_batch(b, cs["X"], cs["U"], *cs["W"], cs["X"][:, 0])["K"])      # the gains of the shortened horizons
    uc.check_tiny(pkg, ol, run, c2, 64, b)


def test_dark_table_and_null_table_are_the_emulated_parent(pkg, run, run_parent, cs):
    """a table dark throughout, and Stab = None, against the emulated model-mag-filtered kernels: difference 0 and equal bytes on
    every output, both laws, both latencies, with and without gravity rows; a lit table differs"""
    M, zero = 64, np.zeros_like(cs["Stab"])
    for latency in (0, 1):
        for rt, gm in ((cs["Rtab"], gc.GM), (None, 0.0)):
            for law, kw in _laws(cs, M, latency, Rtab=rt, gm=gm)[:3]:
                old = run_parent(law, cs, M, kw)
                uc.same_bytes(old, run(law, cs, M, dict(kw, Stab=zero)))
                uc.same_bytes(old, run(law, cs, M, dict(kw, Stab=zero, sigma_sun=0.0, filt=dict(uc.FILT, sigma_s=7.0))))
                uc.same_bytes(old, run(law, cs, M, dict(kw, Stab=None, sigma_sun=0.0)))
                uc.same_bytes(old, run(law, cs, M, dict(kw, Stab=None, sigma_sun=0.0, filt=dict(uc.FILT, sigma_s=0.0))))      # not looked at
                assert np.max(np.abs(old["X_hat"] - run(law, cs, M, kw)["X_hat"])) >= gc.MOVED


def test_null_filter_is_byte_equal_to_the_emulated_sensed_parents(pkg, run, cs):
    """f = None (with Stab = None, sigma_sun = 0) dispatches to the sensed call: byte for byte its outputs"""
    old, M = sc.EmuSensed(pkg._abi), 64
    keys = ("X_sim", "stats", "summary", "nominal", "n_clipped")
    for latency in (0, 1):
        for rt, gm in ((cs["Rtab"], gc.GM), (None, 0.0)):
            over = dict(latency=latency, Rtab=rt, gm=gm, filt=None, Stab=None, sigma_sun=0.0)
            kw = uc.tv_kw(cs, M, **over)
            skw = {k: v for k, v in kw.items() if k not in ("filt", "Stab", "sigma_sun")}
            new = run("tv", cs, M, kw)
            uc.same_bytes(old.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], uc.cut(cs["x0s"], M), cs["K"], **skw), new, keys)
            assert new["X_hat"] is None and new["filt_final"] is None
            for kind, mode in (("track_ff", 0), ("regulate", 1)):
                kw = uc.pd_kw(cs, kind, mode, M, **over)
                skw = {k: v for k, v in kw.items() if k not in ("filt", "Stab", "sigma_sun")}
                uc.same_bytes(old.pd(cs["b"], cs["o"], uc.cut(cs["x0s"], M), sc.KD, sc.KP, **skw), run("pd", cs, M, kw), keys)


def test_repeated_and_unrequested_estimates_do_not_change_the_run(pkg, run, cs):
    """``load`` zeroes the record and the sample memory, so a second call is not affected by the first; X_hat / filt_final
    requested or not does not change the run"""
    for latency in (0, 1):
        for law, kw in (("tv", uc.tv_kw(cs, 64, latency=latency)), ("pd", uc.pd_kw(cs, "track_ff", 1, 64, latency=latency))):
            a = run(law, cs, 64, kw)
            other = run(law, cs, 64, dict(kw, sigma_sun=3.0 * uc.SIGMA_SUN, latency=1 - latency))      # a different record in between
            assert other["X_hat"].tobytes() != a["X_hat"].tobytes()
            uc.same_bytes(a, run(law, cs, 64, kw))
            uc.same_bytes(a, run(law, cs, 64, kw, estimates=False), ("X_sim", "stats", "summary", "nominal", "n_clipped"))


def test_realisations_do_not_depend_on_m(pkg, run, cs):
    """with explicit generator ids, realisations 0 .. 62 of the M = 64 run are the M = 63 run, byte for byte"""
    id0 = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
    for law, k63, k64 in (("tv", uc.tv_kw(cs, 63, latency=1, noise_id0=id0), uc.tv_kw(cs, 64, latency=1, noise_id0=id0)),
                          ("pd", uc.pd_kw(cs, "regulate", 1, 63, latency=1, noise_id0=id0), uc.pd_kw(cs, "regulate", 1, 64, latency=1, noise_id0=id0)),
                          ("pd", uc.pd_kw(cs, "track_ff", 0, 63, noise_id0=id0), uc.pd_kw(cs, "track_ff", 0, 64, noise_id0=id0))):
        a, c = run(law, cs, 63, k63), run(law, cs, 64, k64)
        for k in ("stats", "X_sim", "n_clipped", "X_hat", "filt_final"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_two_wavefronts_every_realisation(pkg, ol, run, cs, law):
    """M = 70 (lanes 0 .. 5 of a second wavefront and the model slot in it): every realisation of every slew compared, latency 1;
    at most N_DRAWN - N_KEPT of them may sit on a threshold of the statistic, on the reference alone"""
    M = 70
    kw = uc.tv_kw(cs, M, latency=1) if law == "tv" else uc.pd_kw(cs, "track_ff", 1, M, latency=1)
    ref, got, keep = uc.parity(pkg, ol, run, cs, M, law, kw, skip=None, pairs=dc.all_pairs(cs["b"].T, M))
    assert len(keep) >= 8 * M - (dc.N_DRAWN - dc.N_KEPT)


def test_rejected_arguments(pkg, emu, cs):
    """check_sun_arguments and check_model_mag_sun_filter, the validation the entry points add to their sensed parents', through the
    emulator driver, each rejection with its text; the drivers refuse what they refuse and what the parents refuse"""
    b, M = cs["b"], 5
    good = uc.PdCall(pkg._abi, b, cs["o"], cs["x0s"][:, :M], sc.KD, sc.KP, **uc.pd_kw(cs, "track_ff", 0, M))
    tv = uc.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"][:, :M], K=cs["K"], **uc.tv_kw(cs, M))
    pd_fn, tv_fn = emu.lib.emu_pd_ensemble_model_mag_sun_filtered, emu.lib.emu_tvlqr_ensemble_model_mag_sun_filtered
    assert emu.check(good) == (0, "")
    assert emu.check(good.edit(Stab=None, sigma_sun=0.0)) == (0, "")
    assert emu.check(good.edit(Stab=None, sigma_sun=0.0, f=None)) == (-1, "null filter options")
    assert pd_fn(*good.c_args()) == 0 and tv_fn(*tv.c_args(emu=True)) == 0
    for label, call, words in uc.filter_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert pd_fn(*call.c_args()) == -1, label
    for label, call, words in uc.filter_rejections(tv):
        assert tv_fn(*call.c_args(emu=True)) == -1, label
    # what the sensed parents reject is still rejected
    for label, call, words in sc.sensor_rejections(good):
        assert pd_fn(*call.c_args()) == -1, label
    for label, call, words in sc.sensor_rejections(tv):
        assert tv_fn(*call.c_args(emu=True)) == -1, label
    assert pd_fn(*good.edit(limit_mode=3).c_args()) == -1
    assert tv_fn(*tv.edit(Rtab=None).c_args(emu=True)) == -1          # gm != 0 needs the table
    # f = NULL: no outputs, no table, no sigma_sun
    for call, fn, kw in ((good, pd_fn, {}), (tv, tv_fn, dict(emu=True))):
        none = call.edit(f=None, Stab=None, sigma_sun=0.0)
        assert fn(*none.c_args(**kw)) == -1
        assert fn(*none.edit(X_hat=None).c_args(**kw)) == -1
        assert fn(*none.edit(X_hat=None, filt_final=None).c_args(**kw)) == 0
        assert fn(*none.edit(X_hat=None, filt_final=None, sigma_sun=1e-3).c_args(**kw)) == -1
    # the entry points: a code and a text, not a crash
    lib = pkg._abi.load()
    for fn, call in ((lib.tsat_pd_ensemble_model_mag_sun_filtered, good), (lib.tsat_tvlqr_ensemble_model_mag_sun_filtered, tv)):
        assert fn(None, *call.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, X_hat=None, filt_final=None).c_args()) == -1
        assert b"Stab must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(Stab=None).c_args()) == -1 and b"sigma_sun must be 0" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, Stab=None, sigma_sun=0.0).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(Stab=None, sigma_sun=0.0).c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_entry_points_are_declared(pkg):
    """the header, ``_abi``, the Julia shim, the wrappers and this tier's constants agree"""
    tr, abi = pkg.tracking, pkg._abi
    lib = abi.load()
    deg = math.pi / 180.0
    names = list(uc.LEVELS)
    assert C.sizeof(abi.ModelMagSunFilterOptions) == 72
    assert [(n, C.sizeof(t)) for n, t in abi.ModelMagSunFilterOptions._fields_] == [(n, 8) for n in names] + [("reserved", 4)]
    fo = abi.ModelMagSunFilterOptions(9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 7)
    lib.tsat_model_mag_sun_filter_default_options(C.byref(fo))
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 0.0, 0.0, 0.38 * math.pi / 180.0, 0.0, 0.0, deg, 0.0, 0]
    lib.tsat_model_mag_sun_filter_default_options(None)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    src = open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_model_mag_sun_filtered.hpp")).read()
    body = re.search(r"struct tsat_model_mag_sun_filter_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", n) for n in names] + [("int32_t", "reserved")]
    assert tr.MODEL_MAG_FILTER_W == 12 == uc.FILTER_W
    for name in ("tsat_model_mag_sun_filter_default_options", "tsat_tvlqr_ensemble_model_mag_sun_filtered",
                 "tsat_pd_ensemble_model_mag_sun_filtered"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
        assert hasattr(lib, name)
    # the prototypes are the parent's with the new options struct, then the sun table and sigma_sun
    for law in ("tvlqr", "pd"):
        s, f = abi.PROTOTYPES[f"tsat_{law}_ensemble_model_mag_filtered"], abi.PROTOTYPES[f"tsat_{law}_ensemble_model_mag_sun_filtered"]
        assert f[0] is s[0] and len(f[1]) == len(s[1]) + 2 and f[1][:len(s[1]) - 3] == s[1][:-3] and f[1][-4:-2] == s[1][-2:]
        assert f[1][-5]._type_ is abi.ModelMagSunFilterOptions and f[1][-2] is s[1][-1] and f[1][-1] is C.c_double
    # the statements the headers have to make
    for text in (hdr, src):
        assert "Hs = -C(n) [s_j]x" in text and "s_{k-1}" in text and "S = Hs A Hs^T + sigma_s^2 I" in text
        assert re.search(r"NO per-realisation sun-sensor bias|NO PER-REALISATION SUN-SENSOR BIAS", text)
    assert "ModelMagFiltered<real> mm;" in src and not re.search(r"struct \w*State\b", src) and "24u" in src
    # no other draw of the library uses a counter above 20
    csrc = os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hpp", ".hip")) and fn != "tsat_model_mag_sun_filtered.hpp":
            for m in re.finditer(r"philox4x32_10\([^;]*?(\d+)u,\s*\w+\);", open(os.path.join(csrc, fn)).read()):
                assert int(m.group(1)) <= 20, (fn, m.group(0))
    # model_mag_sun_filter_options: sigma_w, sigma_g, sigma_m and sigma_s are required
    sig = inspect.signature(tr.model_mag_sun_filter_options)
    assert list(sig.parameters) == ["sigma_w", "sigma_g", "sigma_m", "sigma_s", "sigma_v", "sigma_u", "p0_att", "p0_bias"]
    assert all(sig.parameters[n].default is inspect.Parameter.empty for n in ("sigma_w", "sigma_g", "sigma_m", "sigma_s"))
    fo = tr.model_mag_sun_filter_options(1e-4, 1e-3, 5e-7, 8e-3)
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 1e-4, 0.0, 1e-3, 5e-7, 8e-3, deg, 0.0, 0]
    fo = tr.model_mag_sun_filter_options(1e-4, 1e-3, 5e-7, 8e-3, sigma_v=6e-4, sigma_u=3e-5, p0_att=4e-2, p0_bias=5e-3)
    assert [getattr(fo, n) for n in names] == [6e-4, 1e-4, 3e-5, 1e-3, 5e-7, 8e-3, 4e-2, 5e-3]
    for bad in (dict(sigma_w=-1.0, sigma_g=1.0, sigma_m=1.0, sigma_s=1.0), dict(sigma_w=1.0, sigma_g=1.0, sigma_m=0.0, sigma_s=1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_m=1.0, sigma_s=0.0), dict(sigma_w=1.0, sigma_g=1.0, sigma_m=1.0, sigma_s=float("nan")),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_m=1.0, sigma_s=-1.0)):
        with pytest.raises(ValueError):
            tr.model_mag_sun_filter_options(**bad)
    # the two calls take the parent wrappers' signatures, then Stab and sigma_sun
    for new, old in ((tr.attitude_ensemble_model_mag_sun_filtered, tr.attitude_ensemble_model_mag_filtered),
                     (tr.attitude_ensemble_pd_model_mag_sun_filtered, tr.attitude_ensemble_pd_model_mag_filtered)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters) + ["Stab", "sigma_sun"]
        assert inspect.signature(new).parameters["Stab"].default is None and inspect.signature(new).parameters["sigma_sun"].default == 0.0
    fo, Xh, ff = tr._model_mag_sun_filtering(2, 3, 5, fo, True)
    assert Xh.shape == (2, 3, 5, 7) and ff.shape == (2, 3, 12)
    for bad in (None, tr.model_mag_filter_options(1e-4, 1e-3, 5e-7)):      # another filter's options are not these
        with pytest.raises(ValueError):
            tr._model_mag_sun_filtering(2, 3, 5, bad, False)
    b = pc.case(pkg)[0]
    S = np.zeros((b.Btab.shape[0], b.n_tab, 3))
    assert tr._sun(b, None, 0.0) == (None, 0.0) and tr._sun(b, S, 1e-3)[1] == 1e-3 and tr._sun(b, S, 0.0)[0].flags.c_contiguous
    for bad in ((None, 1e-3), (S[:, :-1], 0.0), (S[0], 0.0), (S, -1.0), (S, float("nan"))):
        with pytest.raises(ValueError):
            tr._sun(b, *bad)
