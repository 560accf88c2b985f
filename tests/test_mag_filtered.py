"""CPU tier of the ensemble controllers behind the magnetometer-updated attitude filter (tsat_tvlqr_ensemble_mag_filtered,
tsat_pd_ensemble_mag_filtered): H of the reference against a central difference, the reference of tests/mag_filtered_common.py pinned
to the sensed reference with the filter off, a zero field row, the kernel source of tortoisesat.jl_amd/csrc/tsat_mag_filtered.hpp under
the lane emulator against the reference (X_sim, X_hat, filt_final to 1e-9; stats, n_clipped, summary as tests/test_sensed.py compares
them), f = NULL against the emulated sensed parents, what the calls reject (the library's own check_mag_filter) and the host layers.

The case is tests/test_filtered.py's: ``pd_common.case`` (8 slews, N = 20, ragged horizons) at M = 5, the sampled pairs of
``dispersed_common.sampled_pairs`` compared, all five plant dispersions, plant noise on, gravity gradient on, TVLQR weights
r = 0.5e-6, PD gains 10 x pd_common's, sensor levels sensed_common.SIGMAS / BIAS, filter levels mag_filtered_common.MFILT."""
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
import mag_filtered_common as mc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

M = 5
KINDS = ("track", "track_ff", "regulate")
N_COND = 4


@pytest.fixture(scope="module")
def emu(pkg):
    return mc.EmuMagFiltered(pkg._abi)


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
    kw = dict(Rtab=cs["Rtab"], gm=gc.GM, plant=cs["plant"], sat=sat, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"], filt=mc.MFILT)
    kw.update(over)
    return kw


def _pd_kw(cs, kind, mode, **over):
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"], gm=gc.GM,
              plant=cs["plant"], sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], sens=sc.SIGMAS, latency=0, sensor=cs["sensor"],
              filt=mc.MFILT)
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


def _cond_pairs(cs):
    """the first N_COND pairs of full horizon: the conditions are shown on a part of the pairs, they hold on all"""
    full = cs["pairs"][ec.horizons(cs["b"])[cs["pairs"][:, 0]] == cs["b"].N]
    return full[:: max(1, len(full) // N_COND)][:N_COND]


def test_h_is_the_derivative_of_the_predicted_field(ol):
    """H = -C(n) [r]x of the reference against a central difference of qrot(q (x) [1; dtheta / 2], r) in dtheta, relative bar 1e-6;
    and H = -[b^]x C(n), the equivalent form of the header"""
    ol.load()
    rng = np.random.default_rng(3)
    eps, worst = 1e-6, 0.0
    for _ in range(20):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        r = 2.5e-5 * rng.standard_normal(3)
        H = mc.h_matrix(q, r)
        num = np.zeros((3, 3))
        for j in range(3):
            e = np.zeros(3)
            e[j] = eps
            num[:, j] = (ol.qrot(ol.qmult(q, np.r_[1.0, e / 2]), r) - ol.qrot(ol.qmult(q, np.r_[1.0, -e / 2]), r)) / (2 * eps)
        worst = max(worst, float(np.max(np.abs(H - num)) / np.max(np.abs(H))))
        np.testing.assert_allclose(H, -fc._skew(ol.qrot(q, r)) @ mc.cmat(q), rtol=0, atol=1e-15 * 2.5e-5 * 100)
        np.testing.assert_allclose(mc.cmat(q) @ r, ol.qrot(q, r), rtol=0, atol=1e-19)
    print(f"H against the central difference at step {eps:.0e}: {worst:.1e} relative")
    assert worst < 1e-6


def test_reference_with_the_filter_off_is_the_sensed_reference(pkg, ol, cs):
    """the anchor: ``mag_filtered_common.pairs_of`` with filt = None is ``sensed_common.pairs_of``, max |d| = 0, both laws and both
    latencies, the nominal slot included"""
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


def test_a_zero_row_leaves_the_estimate_at_the_propagated_one(ol):
    """a step against r = 0: H = 0 and K = 0, so q^ is q- normalised, b^ stays, w^ = w_m - b^ and P is P-; the same step with the
    update off gives the same record"""
    ol.load()
    rng = np.random.default_rng(9)
    w0, q0 = 0.02 * rng.standard_normal(3), rng.standard_normal(4)
    w1, bm = 0.02 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3)
    B0, b0, r1 = 1e-6 * rng.standard_normal((3, 3)), 1e-3 * rng.standard_normal(3), 2.5e-5 * rng.standard_normal(3)

    def stepped(update, r):
        e = mc.MagEkf(ol, 0.2, mc.MFILT, update)
        e.first(w0, q0)
        e.B, e.b = B0.copy(), b0.copy()                     # a record in which every block is at work
        e.step(w1, bm, r)
        return e

    z, off, moved = stepped(True, np.zeros(3)), stepped(False, np.zeros(3)), stepped(True, r1)
    assert np.max(np.abs(moved.q - z.q)) > 1e-6, "a non-zero row must move the estimate, or the test shows nothing"
    qm, Am, Bm, Dm = z.prior
    assert np.array_equal(z.q, qm / math.sqrt(float(qm @ qm))) and np.array_equal(z.w, w1 - z.b)
    assert np.array_equal(z.A, fc._sym(Am)) and np.array_equal(z.B, Bm) and np.array_equal(z.D, fc._sym(Dm))
    for a, c in ((z.q, off.q), (z.b, off.b), (z.w, off.w), (z.A, off.A), (z.B, off.B), (z.D, off.D)):
        assert np.array_equal(a, c)
    assert np.isfinite(z.final()).all()


def _check_against(pkg, ol, cs, ref, got, pairs, keep, nom_ref):
    b = cs["b"]
    dc.compare(ref, got, pairs, keep)
    mc.compare_estimates(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
    ec.same_stats(nom_ref["stats"], got["nominal"])


def _parity(pkg, ol, emu, cs, law, kw, with_conditions=True, prediction=None):
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
        mc.conditions(lambda **o_: ref_of(pkg, ol, cs, cp, dict(kw, **o_)), kw["sensor"],
                      prediction=(law == "tv") if prediction is None else prediction, pairing=False)
    got = run(emu, cs, kw)
    _check_against(pkg, ol, cs, ref, got, pairs, keep, ref_of(pkg, ol, cs, _nomp(b), kw))
    return ref, got, keep


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
def test_emulated_tvlqr_matches_reference(pkg, ol, emu, cs, limits, latency):
    """8 slews x M = 5, limits +-0.6 and +-25, latency 0 and 1. Behind this coarser estimate the TVLQR gains of the case (|K| up to
    4.8e3) reach +-25 at a few knots too: the clip counts are compared there as under +-0.6"""
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
    c2 = dict(cs, x0s=cs["x0s"] + np.r_[mc.FAST, np.zeros(4)])
    _parity(pkg, ol, emu, c2, "pd", _pd_kw(c2, kind, 0, latency=1, sat=pc.WIDE), prediction=True)


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_emulated_delayed_sample_is_paired_with_its_own_row(pkg, ol, emu, cs, law):
    """latency 1 on ``mag_filtered_common.fast_table``, tables whose rows turn 25 deg from one to the next: there the row the delayed
    sample is updated against moves the final state (at the case's own tables, whose neighbouring rows differ by 4.5e-4 of the field,
    it moves it by 4e-8 and 8e-9, under the bar); the condition on references alone, then parity"""
    c2 = dict(cs, b=mc.fast_table(cs["b"]))
    kw = _tv_kw(c2, latency=1, sat=pc.WIDE) if law == "tv" else _pd_kw(c2, "track_ff", 0, latency=1, sat=pc.WIDE)
    ref_of = _tv_ref if law == "tv" else _pd_ref
    cp = _cond_pairs(c2)
    pc.differs(ref_of(pkg, ol, c2, cp, kw), ref_of(pkg, ol, c2, cp, dict(kw, pair_own_row=False)), "the delayed sample against r_{k-1}, not r_k")
    _parity(pkg, ol, emu, c2, law, kw, with_conditions=False)


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
            assert np.max(np.abs(new["X_sim"] - _tv_emu(emu, cs, dict(kw, filt=mc.MFILT))["X_sim"])) >= gc.MOVED
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
    """check_mag_filter, the validation function both entry points add to their sensed parents', through the emulator driver; the
    drivers refuse what it refuses and what the parents refuse; f = NULL with an output asked for is refused by the entry points
    before anything else, with its text"""
    b = cs["b"]
    good = mc.PdCall(pkg._abi, b, cs["o"], cs["x0s"], sc.KD, sc.KP, **_pd_kw(cs, "track_ff", 0))
    tv = mc.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], K=cs["K"], **_tv_kw(cs))
    assert emu.check(good) == (0, "")
    assert emu.check(good.edit(f=None)) == (-1, "null filter options")
    assert emu.lib.emu_pd_ensemble_mag_filtered(*good.c_args()) == 0 and emu.lib.emu_tvlqr_ensemble_mag_filtered(*tv.c_args(emu=True)) == 0
    for label, call, words in mc.filter_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert emu.lib.emu_pd_ensemble_mag_filtered(*call.c_args()) == -1, label
    for label, call, words in mc.filter_rejections(tv):
        assert emu.lib.emu_tvlqr_ensemble_mag_filtered(*call.c_args(emu=True)) == -1, label
    # what the sensed parents reject is still rejected
    for label, call, words in sc.sensor_rejections(good):
        assert emu.lib.emu_pd_ensemble_mag_filtered(*call.c_args()) == -1, label
    for label, call, words in sc.sensor_rejections(tv):
        assert emu.lib.emu_tvlqr_ensemble_mag_filtered(*call.c_args(emu=True)) == -1, label
    assert emu.lib.emu_pd_ensemble_mag_filtered(*good.edit(limit_mode=3).c_args()) == -1
    assert emu.lib.emu_tvlqr_ensemble_mag_filtered(*tv.edit(Rtab=None).c_args(emu=True)) == -1          # gm != 0 needs the table
    # f = NULL with X_hat or filt_final
    for call, fn, kw in ((good, emu.lib.emu_pd_ensemble_mag_filtered, {}), (tv, emu.lib.emu_tvlqr_ensemble_mag_filtered, dict(emu=True))):
        assert fn(*call.edit(f=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None).c_args(**kw)) == -1
        assert fn(*call.edit(f=None, X_hat=None, filt_final=None).c_args(**kw)) == 0
    # the entry points: a code and a text, not a crash
    lib = pkg._abi.load()
    for fn, call in ((lib.tsat_pd_ensemble_mag_filtered, good), (lib.tsat_tvlqr_ensemble_mag_filtered, tv)):
        assert fn(None, *call.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, filt_final=None).c_args()) == -1
        assert b"X_hat and filt_final must be NULL" in lib.tsat_ensemble_last_error()
        assert fn(None, *call.edit(f=None, X_hat=None, filt_final=None).c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_mag_filter_options_and_host_layers(pkg):
    """the header, ``_abi``, the wrappers and this tier's constants agree"""
    tr, abi = pkg.tracking, pkg._abi
    lib = abi.load()
    deg = math.pi / 180.0
    assert C.sizeof(abi.MagFilterOptions) == 48
    assert [(n, C.sizeof(t)) for n, t in abi.MagFilterOptions._fields_] == [("sigma_v", 8), ("sigma_u", 8), ("sigma_m", 8), ("p0_att", 8),
                                                                             ("p0_bias", 8), ("reserved", 4)]
    fo = abi.MagFilterOptions(9.0, 9.0, 9.0, 9.0, 9.0, 7)
    lib.tsat_mag_filter_default_options(C.byref(fo))
    # the six-state filter's defaults, and sigma_m left 0
    ref = abi.FilterOptions()
    lib.tsat_filter_default_options(C.byref(ref))
    assert (fo.sigma_v, fo.sigma_u, fo.sigma_m, fo.p0_att, fo.p0_bias, fo.reserved) == (ref.sigma_v, ref.sigma_u, 0.0, ref.p0_att, ref.p0_bias, 0)
    assert (fo.sigma_v, fo.p0_att) == (tr.SENSOR_SIGMA_GYRO, deg)
    lib.tsat_mag_filter_default_options(None)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    body = re.search(r"struct tsat_mag_filter_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", "sigma_v"), ("double", "sigma_u"), ("double", "sigma_m"),
                                                              ("double", "p0_att"), ("double", "p0_bias"), ("int32_t", "reserved")]
    assert re.search(r"#define TSAT_FILTER_W 9\b", hdr) and tr.FILTER_W == 9 == mc.FILTER_W
    for name in ("tsat_mag_filter_default_options", "tsat_tvlqr_ensemble_mag_filtered", "tsat_pd_ensemble_mag_filtered"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
    # the prototypes are the sensed ones plus (filter options, X_hat, filt_final)
    for law in ("tvlqr", "pd"):
        s, f = abi.PROTOTYPES[f"tsat_{law}_ensemble_sensed"], abi.PROTOTYPES[f"tsat_{law}_ensemble_mag_filtered"]
        assert f[0] is s[0] and f[1][:len(s[1])] == s[1] and len(f[1]) == len(s[1]) + 3
        assert f[1][-3]._type_ is abi.MagFilterOptions
    # the statements the headers have to make
    for text in (hdr, open(os.path.join(ec.ROOT, "tortoisesat.jl_amd", "csrc", "tsat_mag_filtered.hpp")).read()):
        assert "H = -C(n) [r_j]x" in text and "r_{k-1}, not r_k" in text
    # mag_filter_options
    fo = tr.mag_filter_options(1e-3, 5e-7)
    assert (fo.sigma_v, fo.sigma_m, fo.sigma_u, fo.p0_att, fo.p0_bias, fo.reserved) == (1e-3, 5e-7, 0.0, deg, 0.0, 0)
    fo = tr.mag_filter_options(1e-3, 5e-7, sigma_u=3e-5, p0_att=4e-2, p0_bias=5e-3)
    assert (fo.sigma_v, fo.sigma_m, fo.sigma_u, fo.p0_att, fo.p0_bias, fo.reserved) == (1e-3, 5e-7, 3e-5, 4e-2, 5e-3, 0)
    assert isinstance(fo, abi.MagFilterOptions)
    assert list(inspect.signature(tr.mag_filter_options).parameters) == ["sigma_v", "sigma_m", "sigma_u", "p0_att", "p0_bias"]
    for bad in (dict(sigma_v=-1.0, sigma_m=1.0), dict(sigma_v=1.0, sigma_m=0.0), dict(sigma_v=1.0, sigma_m=1.0, sigma_u=-1.0),
                dict(sigma_v=1.0, sigma_m=1.0, p0_att=-1.0), dict(sigma_v=1.0, sigma_m=1.0, p0_bias=-1.0),
                dict(sigma_v=1.0, sigma_m=float("nan"))):
        with pytest.raises(ValueError):
            tr.mag_filter_options(**bad)
    # the two calls take the arguments of the filtered wrappers
    for new, old in ((tr.attitude_ensemble_mag_filtered, tr.attitude_ensemble_filtered), (tr.attitude_ensemble_pd_mag_filtered, tr.attitude_ensemble_pd_filtered)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
        assert inspect.signature(new).parameters["want_estimates"].default is False
    fo, Xh, ff = tr._mag_filtering(2, 3, 5, fo, True)
    assert Xh.shape == (2, 3, 5, 7) and ff.shape == (2, 3, 9)
    assert tr._mag_filtering(2, 3, 5, fo, False)[1] is None
    for bad in (None, tr.filter_options(1e-3, 2e-3)):           # sigma_m has no default; another filter's options are not these
        with pytest.raises(ValueError):
            tr._mag_filtering(2, 3, 5, bad, False)
