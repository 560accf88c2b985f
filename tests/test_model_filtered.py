"""CPU tier of the ensemble controllers behind the model-based rate filter (tsat_tvlqr_ensemble_model_filtered,
tsat_pd_ensemble_model_filtered): the reference of tests/model_filtered_common.py pinned to the sensed reference with the filter off,
its conditions, the kernel source of tortoisesat.jl_amd/csrc/tsat_model_filtered.hpp under the lane emulator against it (X_sim, X_hat,
filt_final to 1e-9; stats, n_clipped, summary as tests/test_sensed.py compares them), tiny horizons at latency 1, a long horizon on
which the filter has to smooth the gyro noise, f = NULL against the emulated sensed parents, what the calls reject (the library's own
check_model_filter) and the host layers.

The case is tests/test_filtered.py's: slews 0 and 1 of ``pd_common.case`` (horizons 20 and 13), M = 3, every pair, all five plant
dispersions, plant noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels
sensed_common.SIGMAS / BIAS, filter levels model_filtered_common.FILT.

Which case shows which term (bar gg_common.MOVED on the final states; every parity test prints every figure): on the case's own
starts and levels every term of ``model_filtered_common.terms_of`` and, at latency 1, the prediction across the delay shows under
both laws, except
  - the gyroscopic term of Phi_ww, which is of size h |w| (J_i - J_j) / J_k: it needs the body rate filtered_common.FAST
    (test_emulated_fast_starts: both laws, regulation included, both latencies);
  - the command in predict under the PD law when it regulates or flies the direction-preserving limit, 1e-7 .. 2e-6 on the own
    starts: asserted on the FAST starts (regulation under that limit included), where it moves the final state by 1e-5 .. 1e-4;
  - the prediction across the delay under the PD law, 1e-7 .. 2e-7 at the case's own rates (7e-8 on the GPU tier's 8-slew case), as
    with the six-state filter: asserted on the FAST starts;
  - the order of the two updates, which acts only through the second-order term of the quaternion correction: it needs the sensor
    levels model_filtered_common.LOUD_SENS (test_emulated_loud_sensor_shows_the_update_order: both laws, both latencies)."""
import ctypes as C
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import model_filtered_common as mc
import pd_common as pc
import sensed_common as sc

IDS = np.array([7, 2 ** 33 + 1], dtype=np.int64)
M = 3
KINDS = ("track", "track_ff", "regulate")
LEFT = (mc.GYROSCOPIC, mc.ORDER)


@pytest.fixture(scope="module")
def emu(pkg):
    return mc.EmuModelFiltered(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the pair, its plan and gains from the oracle, M = 3 realisations; computed once and left unchanged"""
    b8, Rtab = pc.case(pkg)
    b = b8.slice(0, 2)
    r = ol.solve_batch(b, hc.solve_options(ol))
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=(Qd, Qfd, Rd), K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, M),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, M))


def _tv_kw(cs, sat=hc.SAT, **over):
    kw = dict(Rtab=cs["Rtab"], gm=gc.GM, plant=cs["plant"], sat=sat, noise_id0=IDS, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"],
              filt=mc.FILT)
    kw.update(over)
    return kw


def _pd_kw(cs, kind, mode, **over):
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"], gm=gc.GM,
              plant=cs["plant"], sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], noise_id0=IDS, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"],
              filt=mc.FILT)
    kw.update(over)
    return kw


def _tv_ref(pkg, ol, cs, pairs, kw):
    return mc.pairs_of(ol, pkg._abi, "tv", cs["b"], cs["x0s"], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **kw)


def _pd_ref(pkg, ol, cs, pairs, kw):
    return mc.pairs_of(ol, pkg._abi, "pd", cs["b"], cs["x0s"], (sc.KD, sc.KP), cs["o"], pairs, **kw)


def _tv_emu(emu, cs, kw):
    return emu.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **kw)


def _pd_emu(emu, cs, kw):
    return emu.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **kw)


def _nomp(b):
    return np.array([(t, -1) for t in range(b.T)])


def test_reference_with_the_filter_off_is_the_sensed_reference(pkg, ol, cs):
    """the anchor: ``model_filtered_common.pairs_of`` with filt = None is ``sensed_common.pairs_of``, max |d| = 0, both laws and both
    latencies, the nominal slot included"""
    b = cs["b"]
    pairs = np.concatenate([dc.all_pairs(b.T, M), _nomp(b)])
    for latency in (0, 1):
        kw = _tv_kw(cs, latency=latency, filt=None)
        skw = {k: v for k, v in kw.items() if k != "filt"}
        old = sc.pairs_of(ol, pkg._abi, "tv", b, cs["x0s"], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **skw)
        new = _tv_ref(pkg, ol, cs, pairs, kw)
        d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
        print(f"TVLQR reference with the filter off against sensed_common.pairs_of, latency {latency}: max|d| {d:.1e}")
        assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
        assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
        assert not new["X_hat"].any() and not new["filt_final"].any()
        for kind, mode in (("track_ff", 0), ("regulate", 1), ("track", 0)):
            kw = _pd_kw(cs, kind, mode, latency=latency, filt=None)
            skw = {k: v for k, v in kw.items() if k != "filt"}
            old = sc.pairs_of(ol, pkg._abi, "pd", b, cs["x0s"], (sc.KD, sc.KP), cs["o"], pairs, **skw)
            new = _pd_ref(pkg, ol, cs, pairs, kw)
            d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
            print(f"PD reference ({kind}, mode {mode}) with the filter off against sensed_common.pairs_of, latency {latency}: max|d| {d:.1e}")
            assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])


def test_reference_filter_keeps_its_invariants(pkg, ol, cs):
    """on the reference alone: q^ stays unit, the covariance keeps a positive diagonal, the noise-free realisation flown on the
    model's plant without gravity gradient is predicted by the filter's model to rounding (the mean of predict is the plant's own
    step), and with p0_bias = sigma_u = 0 the bias estimate stays exactly zero"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    ref = _tv_ref(pkg, ol, cs, pairs, _tv_kw(cs))
    for i, n in enumerate(ref["n_knots"]):
        nq = np.linalg.norm(ref["X_hat"][i, :n - 1, 3:7], axis=1)
        assert np.max(np.abs(nq - 1.0)) < 1e-14
    assert np.all(ref["filt_final"][:, 3:] > 0) and np.all(ref["filt_final"][:, :3] != 0)
    nobias = _tv_ref(pkg, ol, cs, pairs, _tv_kw(cs, filt=dict(mc.FILT, sigma_u=0.0, p0_bias=0.0)))
    assert not nobias["filt_final"][:, 0:3].any() and not nobias["filt_final"][:, 9:12].any()
    nom = _tv_ref(pkg, ol, cs, _nomp(b), _tv_kw(cs, Rtab=None, gm=0.0, sat=pc.WIDE))
    for i, n in enumerate(nom["n_knots"]):
        qs = nom["X_sim"][i, :n - 1, 3:7]
        d = np.abs(np.c_[nom["X_hat"][i, :n - 1, 0:3] - nom["X_sim"][i, :n - 1, 0:3],
                         nom["X_hat"][i, :n - 1, 3:7] - qs / np.linalg.norm(qs, axis=1, keepdims=True)])
        print(f"noise-free realisation on the model's plant: max |X_hat - X_sim| {float(d.max()):.1e}")
        assert d.max() < 1e-13


def _check_against(pkg, ol, cs, ref, got, pairs, nom_ref):
    b = cs["b"]
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], cs["o"].min_steps, cs["o"].w_tol, cs["o"].angle_tol)
    print(f"margin on the reference {m:.2e}; clipped knots sure {ref['n_sure'].tolist()} maybe {ref['n_maybe'].tolist()}")
    assert m > dc.MARGIN
    dc.compare(ref, got, pairs)
    mc.compare_estimates(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    ec.same_stats(nom_ref["stats"], got["nominal"])


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
def test_emulated_tvlqr_matches_reference(pkg, ol, emu, cs, limits, latency):
    """every pair of T = 2 x M = 3 and stats_nominal, limits +-0.6 and +-25, latency 0 and 1"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw = _tv_kw(cs, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref = mc.conditions(lambda **o: _tv_ref(pkg, ol, cs, pairs, dict(kw, **o)), cs["sensor"], latency, skip=LEFT)
    got = _tv_emu(emu, cs, kw)
    _check_against(pkg, ol, cs, ref, got, pairs, _tv_ref(pkg, ol, cs, _nomp(b), kw))
    if limits == "0.6":
        assert ref["n_sure"].max() > 0, "no knot of the case clips"
    else:
        assert not got["n_clipped"].any()


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_pd_matches_reference(pkg, ol, emu, cs, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation under +-0.6 sits
    on its limits at every knot (tests/test_sensed.py): it is compared under +-0.6 AND under +-25, and asserts its conditions there"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw = _pd_kw(cs, kind, mode, latency=latency)
    if kind == "regulate":
        ref = _pd_ref(pkg, ol, cs, pairs, kw)
        assert ref["n_sure"].max() > 0, "no knot of the case clips"
        _check_against(pkg, ol, cs, ref, _pd_emu(emu, cs, kw), pairs, _pd_ref(pkg, ol, cs, _nomp(b), kw))
        kw = dict(kw, sat=pc.WIDE)
    ref = mc.conditions(lambda **o: _pd_ref(pkg, ol, cs, pairs, dict(kw, **o)), cs["sensor"], latency,
                        skip=LEFT + (mc.DELAY[0],) + ((mc.COMMAND,) if (kind == "regulate" or mode == 1) else ()))
    _check_against(pkg, ol, cs, ref, _pd_emu(emu, cs, kw), pairs, _pd_ref(pkg, ol, cs, _nomp(b), kw))


def _law(c2, law, **over):
    if law == "tv":
        return _tv_kw(c2, **over), _tv_ref, _tv_emu
    return _pd_kw(c2, "regulate" if law == "pd_regulate" else "track_ff", 1 if law == "pd_regulate" else 0, **over), _pd_ref, _pd_emu


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd", "pd_regulate"])
def test_emulated_fast_starts(pkg, ol, emu, cs, law, latency):
    """the body rate filtered_common.FAST added to the starts, limits +-25: the case on which the gyroscopic term of Phi_ww shows,
    and the command in predict under regulation; every condition but the update order, then parity"""
    c2 = dict(cs, x0s=cs["x0s"] + np.r_[mc.FAST, np.zeros(4)])
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw, ref_of, run = _law(c2, law, latency=latency, sat=pc.WIDE)
    ref = mc.conditions(lambda **o: ref_of(pkg, ol, c2, pairs, dict(kw, **o)), cs["sensor"], latency, skip=(mc.ORDER,))
    _check_against(pkg, ol, c2, ref, run(emu, c2, kw), pairs, ref_of(pkg, ol, c2, _nomp(b), kw))


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_loud_sensor_shows_the_update_order(pkg, ol, emu, cs, law, latency):
    """the sensor and filter levels model_filtered_common.LOUD_SENS / LOUD_FILT, limits +-25: the case on which the order of the two
    updates shows; that condition, then parity"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw, ref_of, run = _law(cs, law, latency=latency, sat=pc.WIDE, sens=mc.LOUD_SENS, filt=mc.LOUD_FILT)
    ref = ref_of(pkg, ol, cs, pairs, kw)
    d = mc.moved(ref, ref_of(pkg, ol, cs, pairs, dict(kw, variant=dict(mc.VARIANT, order="ba"))))
    print(f"  condition: {mc.ORDER}: max|d final state| {d:.2e}")
    assert d >= gc.MOVED
    _check_against(pkg, ol, cs, ref, run(emu, cs, kw), pairs, ref_of(pkg, ol, cs, _nomp(b), kw))


def test_tiny_horizons_at_latency_1(pkg, ol, emu, cs):
    """n_knots = 2 (one command, from the first sample) and 3 (two commands: the first sample, then the model's prediction from it
    with no update in between) at latency 1: filt_final is the record of ``first``"""
    b = dataclasses.replace(cs["b"], n_knots=np.array([2, 3], dtype=np.int32))
    c2 = dict(cs, b=b)
    pairs = dc.all_pairs(b.T, M)
    for law, kw in (("tv", _tv_kw(cs, latency=1)), ("pd", _pd_kw(cs, "track_ff", 0, latency=1)), ("pd", _pd_kw(cs, "regulate", 1, latency=1))):
        ref_of = _tv_ref if law == "tv" else _pd_ref
        ref = ref_of(pkg, ol, c2, pairs, kw)
        got = (_tv_emu if law == "tv" else _pd_emu)(emu, c2, kw)
        dc.compare(ref, got, pairs)
        mc.compare_estimates(ref, got, pairs)
        ec.same_stats(ref_of(pkg, ol, c2, _nomp(b), kw)["stats"], got["nominal"])
        for t, n in enumerate(b.n_knots):
            assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
        np.testing.assert_allclose(got["filt_final"], np.broadcast_to(mc.first_record(mc.FILT), got["filt_final"].shape), rtol=1e-15, atol=0)
        # y_0 is the first sample whatever the latency; y_1 of the 3-knot slew is the model's prediction from it, rate included
        r0 = ref_of(pkg, ol, c2, pairs, dict(kw, latency=0))
        assert np.array_equal(ref["X_hat"][:, 0], r0["X_hat"][:, 0])
        three = pairs[:, 0] == 1
        assert np.all(np.any(ref["X_hat"][three, 1, 0:3] != ref["X_hat"][three, 0, 0:3], axis=1))
        assert np.all(np.any(ref["X_hat"][three, 1, 3:7] != r0["X_hat"][three, 1, 3:7], axis=1))


@pytest.fixture(scope="module")
def long_case(pkg, ol):
    """T = 1, N = 200, M = 16 (model_filtered_common.long_case): the references of this filter and of the six-state one, once"""
    return mc.long_case(pkg, ol, N=200, M=16)


def test_filter_smooths_the_gyro_noise_on_a_long_horizon(pkg, ol, emu, long_case):
    """on the references first (model_filtered_common.assert_filter_works): rate error below a quarter of the raw sample's, attitude
    no worse than the six-state filter's within 10 %, the bias inside 3 sigma of its own covariance; then the emulator against the
    reference to 1e-9"""
    mc.assert_filter_works(long_case)
    c = long_case
    got = emu.pd(c["b"], c["o"], c["x0s"], sc.KD, sc.KP, **c["kw"])
    dc.compare(c["ref"], got, c["pairs"])
    mc.compare_estimates(c["ref"], got, c["pairs"])


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
            assert np.max(np.abs(new["X_sim"] - _tv_emu(emu, cs, dict(kw, filt=mc.FILT))["X_sim"])) >= gc.MOVED
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


def test_the_flat_record_round_trips(pkg, emu):
    """ModelFilterState::load / save: TSAT_MODEL_FILTER_STATE_W = 58 values, every one of them carried, strided as a held loop's
    component-major records are"""
    src = open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_model_filtered.hpp")).read()
    assert re.search(r"#define TSAT_MODEL_FILTER_STATE_W 58\b", src)
    src_in, out = np.arange(1.0, 59.0), np.zeros((58, 5))
    assert emu.lib.emu_model_filter_state_roundtrip(pkg._abi.as_dp(src_in), pkg._abi.as_dp(out), C.c_int64(5)) == 58
    assert np.array_equal(out[:, 0], src_in) and not out[:, 1:].any()


def test_rejected_arguments(pkg, emu, cs):
    """check_model_filter, the validation function both entry points add to their sensed parents', through the emulator driver; the
    drivers refuse what it refuses and what the parents refuse; f = NULL with an output asked for is refused by the entry points
    before anything else, with its text"""
    b = cs["b"]
    good = mc.PdCall(pkg._abi, b, cs["o"], cs["x0s"], sc.KD, sc.KP, **_pd_kw(cs, "track_ff", 0))
    tv = mc.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], K=cs["K"], **_tv_kw(cs))
    assert emu.check(good) == (0, "")
    assert emu.lib.emu_pd_ensemble_model_filtered(*good.c_args()) == 0 and emu.lib.emu_tvlqr_ensemble_model_filtered(*tv.c_args(emu=True)) == 0
    for label, call, words in mc.filter_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert emu.lib.emu_pd_ensemble_model_filtered(*call.c_args()) == -1, label
    for label, call, words in mc.filter_rejections(tv):
        assert emu.lib.emu_tvlqr_ensemble_model_filtered(*call.c_args(emu=True)) == -1, label
    # what the sensed parents reject is still rejected
    for label, call, words in sc.sensor_rejections(good):
        assert emu.lib.emu_pd_ensemble_model_filtered(*call.c_args()) == -1, label
    for label, call, words in sc.sensor_rejections(tv):
        assert emu.lib.emu_tvlqr_ensemble_model_filtered(*call.c_args(emu=True)) == -1, label
    assert emu.lib.emu_pd_ensemble_model_filtered(*good.edit(limit_mode=3).c_args()) == -1
    assert emu.lib.emu_tvlqr_ensemble_model_filtered(*tv.edit(Rtab=None).c_args(emu=True)) == -1          # gm != 0 needs the table
    # f = NULL with X_hat or filt_final
    for call, fn, kw in ((good, emu.lib.emu_pd_ensemble_model_filtered, {}), (tv, emu.lib.emu_tvlqr_ensemble_model_filtered, dict(emu=True))):
        assert fn(*call.edit(f=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None, filt_final=None).c_args(**kw)) == 0
    # the entry points: a code and a text, not a crash
    lib = pkg._abi.load()
    for fn, call in ((lib.tsat_pd_ensemble_model_filtered, good), (lib.tsat_tvlqr_ensemble_model_filtered, tv)):
        assert fn(None, *call.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, filt_final=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, X_hat=None, filt_final=None).c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_filter_options_and_host_layers(pkg):
    tr, abi = pkg.tracking, pkg._abi
    lib = abi.load()
    deg = math.pi / 180.0
    names = ["sigma_v", "sigma_w", "sigma_u", "sigma_a", "sigma_g", "p0_att", "p0_bias"]
    # the struct, its defaults and the three symbols through every layer
    assert C.sizeof(abi.ModelFilterOptions) == 64
    assert [(n, C.sizeof(t)) for n, t in abi.ModelFilterOptions._fields_] == [(n, 8) for n in names] + [("reserved", 4)]
    fo = abi.ModelFilterOptions(9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 7)
    lib.tsat_model_filter_default_options(C.byref(fo))
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 0.0, 0.0, deg, 0.38 * math.pi / 180.0, deg, 0.0, 0]
    assert (fo.sigma_g, fo.sigma_a) == (tr.SENSOR_SIGMA_GYRO, tr.SENSOR_SIGMA_ATT)
    lib.tsat_model_filter_default_options(None)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    body = re.search(r"struct tsat_model_filter_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", n) for n in names] + [("int32_t", "reserved")]
    assert re.search(r"#define TSAT_MODEL_FILTER_W 12\b", hdr) and tr.MODEL_FILTER_W == 12 == mc.FILTER_W
    for name in ("tsat_model_filter_default_options", "tsat_tvlqr_ensemble_model_filtered", "tsat_pd_ensemble_model_filtered"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
    # the prototypes are the six-state filter's with the new options struct
    for law in ("tvlqr", "pd"):
        s, f = abi.PROTOTYPES[f"tsat_{law}_ensemble_filtered"], abi.PROTOTYPES[f"tsat_{law}_ensemble_model_filtered"]
        assert f[0] is s[0] and len(f[1]) == len(s[1]) and f[1][:-3] == s[1][:-3] and f[1][-2:] == s[1][-2:]
        assert f[1][-3]._type_ is abi.ModelFilterOptions
    # model_filter_options: sigma_w is required
    assert list(inspect.signature(tr.model_filter_options).parameters) == ["sigma_w", "sigma_g", "sigma_a", "sigma_v", "sigma_u", "p0_att",
                                                                            "p0_bias"]
    assert inspect.signature(tr.model_filter_options).parameters["sigma_w"].default is inspect.Parameter.empty
    fo = tr.model_filter_options(1e-4, 1e-3, 2e-3)
    assert [getattr(fo, n) for n in names] + [fo.reserved] == [0.0, 1e-4, 0.0, 2e-3, 1e-3, 2e-3, 0.0, 0]
    fo = tr.model_filter_options(1e-4, 1e-3, 2e-3, sigma_v=6e-4, sigma_u=3e-5, p0_att=4e-2, p0_bias=5e-3)
    assert [getattr(fo, n) for n in names] == [6e-4, 1e-4, 3e-5, 2e-3, 1e-3, 4e-2, 5e-3] and isinstance(fo, abi.ModelFilterOptions)
    for bad in (dict(sigma_w=-1.0, sigma_g=1.0, sigma_a=1.0), dict(sigma_w=1.0, sigma_g=0.0, sigma_a=1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_a=0.0), dict(sigma_w=1.0, sigma_g=1.0, sigma_a=1.0, sigma_u=-1.0),
                dict(sigma_w=1.0, sigma_g=1.0, sigma_a=1.0, p0_bias=-1.0), dict(sigma_w=float("nan"), sigma_g=1.0, sigma_a=1.0),
                dict(sigma_w=float("inf"), sigma_g=1.0, sigma_a=1.0)):
        with pytest.raises(ValueError):
            tr.model_filter_options(**bad)
    # the two calls take the six-state wrappers' signatures
    for new, old in ((tr.attitude_ensemble_model_filtered, tr.attitude_ensemble_filtered),
                     (tr.attitude_ensemble_pd_model_filtered, tr.attitude_ensemble_pd_filtered)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
    fo, Xh, ff = tr._model_filtering(2, 3, 5, fo, True)
    assert Xh.shape == (2, 3, 5, 7) and ff.shape == (2, 3, 12)
    assert tr._model_filtering(2, 3, 5, fo, False)[1] is None
    for bad in (None, dict(sigma_w=1.0), tr.filter_options(1e-3, 2e-3)):
        with pytest.raises(ValueError):
            tr._model_filtering(2, 3, 5, bad, False)
    assert lib.tsat_version() == 300
