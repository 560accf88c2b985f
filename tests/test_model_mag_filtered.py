"""CPU tier of the ensemble controllers behind the model-based rate filter updated by the magnetometer
(tsat_tvlqr_ensemble_model_mag_filtered, tsat_pd_ensemble_model_mag_filtered): the reference of tests/model_mag_filtered_common.py
pinned to the sensed reference with the filter off and to a full 9 x 9 update, the kernel source of
tortoisesat.jl_amd/csrc/tsat_model_mag_filtered.hpp under the lane emulator against it (X_sim, X_hat, filt_final to 1e-9; stats,
n_clipped, summary as tests/test_sensed.py compares them), tiny horizons at latency 1, a zero field row inside the horizon, a long
horizon, f = NULL against the emulated sensed parents, what the calls reject (the library's own check_model_mag_filter) and the host
layers.

The case is the GPU tier's: ``pd_common.case`` (8 slews, N = 20, ragged horizons), M = 63 and 64 realisations (M + 1 fills one
wavefront exactly, or the model slot is alone in a second one), the sampled pairs of ``dispersed_common.sampled_pairs`` compared, all
five plant dispersions, plant noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels
sensed_common.SIGMAS / BIAS, filter levels model_mag_filtered_common.FILT.

Which case shows which term (bar gg_common.MOVED on the final states; every parity test prints every figure). On the case's own
starts, sensor and tables the seven levels, the magnetometer update, the magnetometer bias and the latency show. Left to their own
cases (model_mag_filtered_common.LEFT):
  - the command in predict, the gyroscopic term of Phi_ww and the prediction across the delay: the body rate filtered_common.FAST
    under limits +-25 (test_emulated_fast_starts);
  - the order of the two updates: the sensor and filter levels LOUD_SENS / LOUD_FILT (test_emulated_loud_sensor_shows_the_update_order);
  - the row a delayed sample is paired with: ``mag_filtered_common.fast_table``
    (test_emulated_delayed_sample_is_paired_with_its_own_row)."""
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
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

MS = (63, 64)


@pytest.fixture(scope="module")
def emu(pkg):
    return mc.EmuModelMagFiltered(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the 8 slews, their plan and gains from the oracle, 64 realisations; computed once and left unchanged"""
    b, Rtab = pc.case(pkg)
    r = ol.solve_batch(b, hc.solve_options(ol))
    W = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], *W, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 64, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=W, K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 64),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, 64))


@pytest.fixture(scope="module")
def run(emu):
    """the tier's call: the emulated kernels"""
    def call(law, e, M, kw, batch=None, **more):
        b = batch or e["b"]
        if law == "tv":
            return emu.tv(b, e["o"], e["X"], e["U"], *e["W"], mc.cut(e["x0s"], M), e["K"], **kw, **more)
        return emu.pd(b, e["o"], mc.cut(e["x0s"], M), sc.KD, sc.KP, **kw, **more)
    return call


def test_reference_with_the_filter_off_is_the_sensed_reference(pkg, ol, cs):
    """the anchor: ``model_mag_filtered_common.pairs_of`` with filt = None is ``sensed_common.pairs_of``, max |d| = 0, both laws and
    both latencies, the nominal slot included"""
    b, M = cs["b"], 5
    pairs = np.concatenate([dc.all_pairs(b.T, M)[::7], mc.nomp(b)[:2]])
    for latency in (0, 1):
        for law, kw in (("tv", mc.tv_kw(cs, M, latency=latency, filt=None)), ("pd", mc.pd_kw(cs, "track_ff", 0, M, latency=latency, filt=None)),
                        ("pd", mc.pd_kw(cs, "regulate", 1, M, latency=latency, filt=None)), ("pd", mc.pd_kw(cs, "track", 0, M, latency=latency, filt=None))):
            skw = {k: v for k, v in kw.items() if k != "filt"}
            if law == "tv":
                old = sc.pairs_of(ol, pkg._abi, "tv", b, cs["x0s"][:, :M], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **skw)
            else:
                old = sc.pairs_of(ol, pkg._abi, "pd", b, cs["x0s"][:, :M], (sc.KD, sc.KP), cs["o"], pairs, **skw)
            new = mc.ref_of(pkg, ol, cs, M, law, pairs, kw)
            d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
            print(f"{law} reference with the filter off against sensed_common.pairs_of, latency {latency}: max|d| {d:.1e}")
            assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
            assert not new["X_hat"].any() and not new["filt_final"].any()


def _worked_record(ol, rng):
    """a ModelMagEkf whose every block is at work: ``first``, one predict, and a dense symmetric positive definite P"""
    J = np.diag([0.04, 0.05, 0.02]) + 1e-3 * np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0.0]])
    e = mc.ModelMagEkf(ol, 0.2, J, 1e-2, mc.FILT)
    e.first(0.02 * rng.standard_normal(3), rng.standard_normal(4))
    e.b = 1e-3 * rng.standard_normal(3)
    L = np.diag([2e-2, 2e-2, 2e-2, 5e-3, 5e-3, 5e-3, 2e-3, 2e-3, 2e-3]) @ (np.eye(9) + 0.3 * np.tril(rng.standard_normal((9, 9)), -1))
    e.P = mfc._sym(L @ L.T)
    return e


def test_one_update_by_blocks_is_a_full_nine_state_update(ol):
    """``_mag`` followed by ``_gyro`` equals two full 9 x 9 updates without the Joseph form, K = P H^T (H P H^T + R)^-1,
    P <- P - K S K^T, with H = [Hm 0 0] and H = [0 I I], to 1e-14 on the state and relative to each block's size on P"""
    ol.load()
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(10):
        e = _worked_record(ol, rng)
        r, w_m = 2.5e-5 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)
        b_m = ol.qrot(e.q, r) + 5e-7 * rng.standard_normal(3)
        q, w, b, P = e.q.copy(), e.w.copy(), e.b.copy(), e.P.copy()
        e.update(w_m, b_m, r)
        Z, I = np.zeros((3, 3)), np.eye(3)
        for H, R, z_of in ((lambda q_: np.hstack([gfc.h_matrix(q_, r), Z, Z]), mc.FILT["sigma_m"] ** 2, lambda q_, w_, b_: b_m - ol.qrot(q_, r)),
                           (lambda q_: np.hstack([Z, I, I]), mc.FILT["sigma_g"] ** 2, lambda q_, w_, b_: w_m - (w_ + b_))):
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
    print(f"block update against the full 9 x 9 update: max difference {worst:.1e}")
    assert worst < 1e-14


def test_a_zero_row_leaves_the_gyro_only_posterior(ol):
    """``update`` against r = 0: Hm = 0 and K = 0 in a., so the record after it is the one the gyro update alone leaves — P at that
    knot is the gyro-only posterior — and everything stays finite; a non-zero row moves it"""
    ol.load()
    rng = np.random.default_rng(11)
    e0 = _worked_record(ol, rng)
    w_m, b_m, r1 = 0.02 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3)

    def updated(r, mag=True):
        e = mc.ModelMagEkf(ol, 0.2, e0.J, 1e-2, mc.FILT, dict(mc.VARIANT, mag=mag))
        e.q, e.w, e.b, e.P = e0.q.copy(), e0.w.copy(), e0.b.copy(), e0.P.copy()
        e.update(w_m, b_m, r)
        return e

    z, off, moved = updated(np.zeros(3)), updated(np.zeros(3), mag=False), updated(r1)
    assert np.max(np.abs(moved.q - z.q)) > 1e-6, "a non-zero row must move the estimate, or the test shows nothing"
    for a, c in ((z.w, off.w), (z.b, off.b), (z.P, off.P)):
        assert np.array_equal(a, c)
    assert np.max(np.abs(z.q - off.q)) < 1e-16                 # q^ (x) [1; 0], normalised
    assert np.isfinite(z.final()).all() and np.isfinite(z.q).all()


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
@pytest.mark.parametrize("M", MS)
def test_emulated_tvlqr_matches_reference(pkg, ol, run, cs, M, limits, latency):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront. LEFT is left to the
    tests named in the module's text"""
    kw = mc.tv_kw(cs, M, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = mc.parity(pkg, ol, run, cs, M, "tv", kw)
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("M", MS)
def test_emulated_pd_matches_reference(pkg, ol, run, cs, M, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation under +-0.6 sits
    on its limits at every knot (tests/test_sensed.py): it is compared under +-0.6 AND under +-25, and asserts its conditions there.
    LEFT is left to the tests named in the module's text"""
    kw = mc.pd_kw(cs, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = mc.parity(pkg, ol, run, cs, M, "pd", kw, skip=None)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    mc.parity(pkg, ol, run, cs, M, "pd", kw)


def _law(c2, law, M, **over):
    if law == "tv":
        return "tv", mc.tv_kw(c2, M, **over)
    return "pd", mc.pd_kw(c2, "regulate" if law == "pd_regulate" else "track_ff", 1 if law == "pd_regulate" else 0, M, **over)


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd", "pd_regulate"])
def test_emulated_fast_starts(pkg, ol, run, cs, law, latency):
    """the body rate filtered_common.FAST added to the starts, limits +-25, M = 64: the case that carries the command in predict,
    the gyroscopic term of Phi_ww and, at latency 1, the prediction across the delay; those conditions, then parity"""
    c2 = dict(cs, x0s=cs["x0s"] + np.r_[mc.FAST, np.zeros(4)])
    law, kw = _law(c2, law, 64, latency=latency, sat=pc.WIDE)
    mc.parity(pkg, ol, run, c2, 64, law, kw, only=(mc.COMMAND, mc.GYROSCOPIC) + ((mc.DELAY,) if latency else ()))


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_loud_sensor_shows_the_update_order(pkg, ol, run, cs, law, latency):
    """the sensor and filter levels LOUD_SENS / LOUD_FILT, limits +-25, M = 64: the case that carries the order of the two updates;
    that condition, then parity"""
    law, kw = _law(cs, law, 64, latency=latency, sat=pc.WIDE, sens=mc.LOUD_SENS, filt=mc.LOUD_FILT)
    mc.parity(pkg, ol, run, cs, 64, law, kw, only=(mc.ORDER,))


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_delayed_sample_is_paired_with_its_own_row(pkg, ol, run, cs, law):
    """latency 1 on ``mag_filtered_common.fast_table`` (rows that turn 25 deg from one to the next), limits +-25, M = 64: the case
    that carries the row the delayed sample is updated against; that condition, then parity"""
    b = gfc.fast_table(cs["b"])
    c2 = dict(cs, b=b, K=ol.tvlqr_batch(b, cs["X"], cs["U"], *cs["W"], cs["X"][:, 0])["K"])      # the gains on these tables
    law, kw = _law(c2, law, 64, latency=1, sat=pc.WIDE)
    mc.parity(pkg, ol, run, c2, 64, law, kw, only=(mc.PAIRING,))


def test_tiny_horizons_at_latency_1(pkg, ol, run, cs):
    """n_knots = 2, 3 and 4 among the slews at latency 1, M = 64 (model_mag_filtered_common.check_tiny)"""
    b = mc.tiny_batch(cs["b"])
    c2 = dict(cs, K=ol.tvlqr_batch(b, cs["X"], cs["U"], *cs["W"], cs["X"][:, 0])["K"])      # the gains of the shortened horizons
    mc.check_tiny(pkg, ol, run, c2, 64, b)


@pytest.mark.parametrize("latency", [0, 1])
def test_zero_row_inside_the_horizon(pkg, ol, run, cs, latency):
    """row 5 of field table 0 set to zero (model_mag_filtered_common.zero_row_batch): the filter makes an update against r = 0
    (Hm = 0, K = 0) at knot 6, at both latencies, and the plant flies a stage without a field. The estimate stays finite and parity
    holds under both laws"""
    b = mc.zero_row_batch(cs["b"])
    e = dict(cs, b=b, K=ol.tvlqr_batch(b, cs["X"], cs["U"], *cs["W"], cs["X"][:, 0])["K"])      # the gains on this table
    for law, kw in (("tv", mc.tv_kw(e, 64, latency=latency, sat=pc.WIDE)), ("pd", mc.pd_kw(e, "track_ff", 1, 64, latency=latency))):
        ref, got, keep = mc.parity(pkg, ol, run, e, 64, law, kw, skip=None)
        assert np.isfinite(got["X_hat"]).all() and np.isfinite(got["filt_final"]).all() and np.isfinite(ref["X_hat"]).all()


def _same(a, c, keys=("X_sim", "stats", "summary", "nominal", "n_clipped")):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_null_filter_is_byte_equal_to_the_emulated_sensed_parents(pkg, run, cs):
    """f = NULL dispatches to the sensed call: byte for byte its outputs, both laws, both latencies, with and without gravity rows"""
    old, M = sc.EmuSensed(pkg._abi), 64
    for latency in (0, 1):
        for rt, gm in ((cs["Rtab"], gc.GM), (None, 0.0)):
            kw = mc.tv_kw(cs, M, latency=latency, Rtab=rt, gm=gm, filt=None)
            skw = {k: v for k, v in kw.items() if k != "filt"}
            new = run("tv", cs, M, kw)
            _same(old.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **skw), new)
            assert new["X_hat"] is None and new["filt_final"] is None
            assert np.max(np.abs(new["X_sim"] - run("tv", cs, M, dict(kw, filt=mc.FILT))["X_sim"])) >= gc.MOVED
            for kind, mode in (("track_ff", 0), ("regulate", 1)):
                kw = mc.pd_kw(cs, kind, mode, M, latency=latency, Rtab=rt, gm=gm, filt=None)
                skw = {k: v for k, v in kw.items() if k != "filt"}
                _same(old.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **skw), run("pd", cs, M, kw))


def test_repeated_and_unrequested_estimates_do_not_change_the_run(pkg, run, cs):
    """``load`` zeroes the record, so a second call is not affected by the first: equal bytes on a repeat, X_hat and filt_final
    included; X_hat / filt_final requested or not does not change the run"""
    for latency in (0, 1):
        for law, kw in (("tv", mc.tv_kw(cs, 64, latency=latency)), ("pd", mc.pd_kw(cs, "track_ff", 1, 64, latency=latency))):
            a = run(law, cs, 64, kw)
            other = run(law, cs, 64, dict(kw, filt=dict(mc.FILT, sigma_w=1e-2), latency=1 - latency))      # a different record in between
            assert other["X_hat"].tobytes() != a["X_hat"].tobytes()
            _same(a, run(law, cs, 64, kw), keys=("X_sim", "stats", "summary", "nominal", "n_clipped", "X_hat", "filt_final"))
            _same(a, run(law, cs, 64, kw, estimates=False))


def test_realisations_do_not_depend_on_m(pkg, run, cs):
    """with explicit generator ids, realisations 0 .. 62 of the M = 64 run are the M = 63 run, byte for byte"""
    id0 = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
    for law, k63, k64 in (("tv", mc.tv_kw(cs, 63, latency=1, noise_id0=id0), mc.tv_kw(cs, 64, latency=1, noise_id0=id0)),
                          ("pd", mc.pd_kw(cs, "regulate", 1, 63, latency=1, noise_id0=id0), mc.pd_kw(cs, "regulate", 1, 64, latency=1, noise_id0=id0)),
                          ("pd", mc.pd_kw(cs, "track_ff", 0, 63, noise_id0=id0), mc.pd_kw(cs, "track_ff", 0, 64, noise_id0=id0))):
        a, c = run(law, cs, 63, k63), run(law, cs, 64, k64)
        for k in ("stats", "X_sim", "n_clipped", "X_hat", "filt_final"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


@pytest.fixture(scope="module")
def long_case(pkg, ol):
    """T = 1, N = 400, M = 8 (model_mag_filtered_common.long_case): the references of this filter, of the mag filter and of gyro
    dead reckoning, once"""
    return mc.long_case(pkg, ol, N=400, M=8)


def test_filter_on_a_long_horizon(pkg, ol, emu, long_case):
    """on the references first (model_mag_filtered_common.assert_filter_works; measured: rate error 9.2e-4 rad/s against the raw
    sample's 1.17e-2, ratio 0.08; attitude 2.77 deg mean, 1.56 .. 4.19, against the mag filter's 3.01 and dead reckoning's 6.10 ..
    9.14; |b^ - b_w| at most 1.2e-3 against 2e-3); then the emulator against the reference to 1e-9"""
    c = long_case
    assert len(c["pairs"]) == 8
    mc.assert_filter_works(c)
    got = emu.pd(c["b"], c["o"], c["x0s"], sc.KD, sc.KP, **c["kw"])
    dc.compare(c["ref"], got, c["pairs"])
    mc.compare_estimates(c["ref"], got, c["pairs"])


def test_rejected_arguments(pkg, emu, cs):
    """check_model_mag_filter, the validation function both entry points add to their sensed parents', through the emulator driver,
    each rejection with its text; the drivers refuse what it refuses and what the parents refuse; f = NULL with an output asked for is
    refused by the entry points before anything else, with its text"""
    b, M = cs["b"], 5
    good = mc.PdCall(pkg._abi, b, cs["o"], cs["x0s"][:, :M], sc.KD, sc.KP, **mc.pd_kw(cs, "track_ff", 0, M))
    tv = mc.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"][:, :M], K=cs["K"], **mc.tv_kw(cs, M))
    pd_fn, tv_fn = emu.lib.emu_pd_ensemble_model_mag_filtered, emu.lib.emu_tvlqr_ensemble_model_mag_filtered
    assert emu.check(good) == (0, "")
    assert emu.check(good.edit(f=None)) == (-1, "null filter options")
    assert pd_fn(*good.c_args()) == 0 and tv_fn(*tv.c_args(emu=True)) == 0
    for label, call, words in mc.filter_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert pd_fn(*call.c_args()) == -1, label
    for label, call, words in mc.filter_rejections(tv):
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
    for fn, call in ((lib.tsat_pd_ensemble_model_mag_filtered, good), (lib.tsat_tvlqr_ensemble_model_mag_filtered, tv)):
        assert fn(None, *call.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, filt_final=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, X_hat=None, filt_final=None).c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_model_mag_entry_points_are_declared(pkg):
    """the header, ``_abi``, the Julia shim, the wrappers and this tier's constants agree"""
    tr, abi = pkg.tracking, pkg._abi
    lib = abi.load()
    deg = math.pi / 180.0
    names = list(mc.LEVELS)
    assert C.sizeof(abi.ModelMagFilterOptions) == 64
    assert [(n, C.sizeof(t)) for n, t in abi.ModelMagFilterOptions._fields_] == [(n, 8) for n in names] + [("reserved", 4)]
    fo = abi.ModelMagFilterOptions(9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 7)
    lib.tsat_model_mag_filter_default_options(C.byref(fo))
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 0.0, 0.0, 0.38 * math.pi / 180.0, 0.0, deg, 0.0, 0]
    assert fo.sigma_g == tr.SENSOR_SIGMA_GYRO
    lib.tsat_model_mag_filter_default_options(None)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    body = re.search(r"struct tsat_model_mag_filter_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", n) for n in names] + [("int32_t", "reserved")]
    assert re.search(r"#define TSAT_MODEL_FILTER_W 12\b", hdr) and tr.MODEL_MAG_FILTER_W == 12 == mc.FILTER_W
    for name in ("tsat_model_mag_filter_default_options", "tsat_tvlqr_ensemble_model_mag_filtered", "tsat_pd_ensemble_model_mag_filtered"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
        assert hasattr(lib, name)
    # the prototypes are the model-filtered pair's with the new options struct
    for law in ("tvlqr", "pd"):
        s, f = abi.PROTOTYPES[f"tsat_{law}_ensemble_model_filtered"], abi.PROTOTYPES[f"tsat_{law}_ensemble_model_mag_filtered"]
        assert f[0] is s[0] and len(f[1]) == len(s[1]) and f[1][:-3] == s[1][:-3] and f[1][-2:] == s[1][-2:]
        assert f[1][-3]._type_ is abi.ModelMagFilterOptions
    # the statements the headers have to make
    for text in (hdr, open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_model_mag_filtered.hpp")).read()):
        assert "Hm = -C(n) [r_j]x" in text and "against r_{k-1}" in text and "S = Hm A Hm^T + sigma_m^2 I" in text
    # the record is the parent's: the held loop's slot can carry it
    src = open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_model_mag_filtered.hpp")).read()
    assert "ModelFiltered<real> mf;" in src and "ModelFilterState" in src and not re.search(r"struct \w*State\b", src)
    # model_mag_filter_options: sigma_w, sigma_g and sigma_m are required
    sig = inspect.signature(tr.model_mag_filter_options)
    assert list(sig.parameters) == ["sigma_w", "sigma_g", "sigma_m", "sigma_v", "sigma_u", "p0_att", "p0_bias"]
    assert all(sig.parameters[n].default is inspect.Parameter.empty for n in ("sigma_w", "sigma_g", "sigma_m"))
    assert (sig.parameters["sigma_v"].default, sig.parameters["sigma_u"].default, sig.parameters["p0_att"].default,
            sig.parameters["p0_bias"].default) == (0.0, 0.0, None, 0.0)
    fo = tr.model_mag_filter_options(1e-4, 1e-3, 5e-7)
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 1e-4, 0.0, 1e-3, 5e-7, deg, 0.0, 0]
    fo = tr.model_mag_filter_options(1e-4, 1e-3, 5e-7, sigma_v=6e-4, sigma_u=3e-5, p0_att=4e-2, p0_bias=5e-3)
    assert [getattr(fo, n) for n in names] == [6e-4, 1e-4, 3e-5, 1e-3, 5e-7, 4e-2, 5e-3] and isinstance(fo, abi.ModelMagFilterOptions)
    for bad in (dict(sigma_w=-1.0, sigma_g=1.0, sigma_m=1.0), dict(sigma_w=1.0, sigma_g=0.0, sigma_m=1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_m=0.0), dict(sigma_w=1.0, sigma_g=1.0, sigma_m=1.0, sigma_u=-1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_m=1.0, p0_bias=-1.0), dict(sigma_w=float("nan"), sigma_g=1.0, sigma_m=1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_m=float("inf"))):
        with pytest.raises(ValueError):
            tr.model_mag_filter_options(**bad)
    # the two calls take the model-filtered wrappers' signatures
    for new, old in ((tr.attitude_ensemble_model_mag_filtered, tr.attitude_ensemble_model_filtered),
                     (tr.attitude_ensemble_pd_model_mag_filtered, tr.attitude_ensemble_pd_model_filtered)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
        assert inspect.signature(new).parameters["want_estimates"].default is False
    fo, Xh, ff = tr._model_mag_filtering(2, 3, 5, fo, True)
    assert Xh.shape == (2, 3, 5, 7) and ff.shape == (2, 3, 12)
    assert tr._model_mag_filtering(2, 3, 5, fo, False)[1] is None
    for bad in (None, tr.model_filter_options(1e-4, 1e-3, 2e-3), tr.mag_filter_options(1e-3, 5e-7)):      # another filter's options are not these
        with pytest.raises(ValueError):
            tr._model_mag_filtering(2, 3, 5, bad, False)
