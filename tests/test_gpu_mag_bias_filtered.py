"""GPU tier of the ensemble controllers behind the magnetometer-updated filter that estimates the magnetometer bias
(tsat_tvlqr_ensemble_mag_bias_filtered, tsat_pd_ensemble_mag_bias_filtered through ``tracking.attitude_ensemble_mag_bias_filtered`` /
``attitude_ensemble_pd_mag_bias_filtered``) against the reference of tests/mag_bias_filtered_common.py, on the smallest shapes at
which the kernels can go wrong. The bars are the parents' (dispersed_common.compare) and 1e-9 on X_hat and filt_final. Every parity
test first asserts its conditions on references alone (mag_bias_filtered_common.conditions, bar 1e-7), over the first N_COND compared
pairs of full horizon.

The case is tests/test_gpu_mag_filtered.py's — ``pd_common.case``, 8 slews, N = 20, ragged horizons, all five plant dispersions,
plant noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels sensed_common.SIGMAS / BIAS —
with the filter levels mag_bias_filtered_common.MBFILT; M = 63 fills one wavefront exactly with the model slot, M = 64 puts the model
slot alone into a second one. The plan is solved once per module at the 1 x 3 budget; the gains of the references are the oracle's."""
import dataclasses

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mag_bias_filtered_common as mb
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
KINDS = ("track", "track_ff", "regulate")
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")
N_COND = 4          # compared pairs the conditions are evaluated on: shown on a part of them, they hold on all


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


def _ws(pkg, solver):
    return int(pkg._abi.load().tsat_workspace_bytes(solver._h))


def _trim(pkg, solver):
    assert pkg._abi.load().tsat_workspace_trim(solver._h, 1) == 0
    assert _ws(pkg, solver) == 0


@pytest.fixture(scope="module")
def ens(pkg, ol, solver):
    """the plan (solved here, 1 x 3 budget), the oracle's gains of it, 64 realisations, their plants and sensor biases; computed once
    and left unchanged"""
    to = pkg.trajopt
    b, Rtab = pc.case(pkg)
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    r = to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    W = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], *W, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 64, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=W, K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 64),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, 64))


def _cut(a, M):
    return None if a is None else np.ascontiguousarray(a[:, :M])


def _tv_kw(e, M, sat=hc.SAT, **over):
    """the keyword arguments that both the reference and the wrapper take (``sens`` is spread into the wrapper's sigma_*, ``filt``
    becomes its ``filter``)"""
    kw = dict(Rtab=e["Rtab"], gm=gc.GM, plant=_cut(e["plant"], M), sat=sat, sens=sc.SIGMAS, latency=0, sensor=_cut(e["sensor"], M),
              filt=mb.MBFILT)
    kw.update(over)
    return kw


def _pd_kw(e, kind, mode, M, **over):
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"], gm=gc.GM,
              plant=_cut(e["plant"], M), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"], sens=sc.SIGMAS, latency=0, sensor=_cut(e["sensor"], M),
              filt=mb.MBFILT)
    kw.update(over)
    return kw


def _wrap(pkg, kw, parent=False):
    """the wrapper's keyword arguments; ``parent``: those of the mag-filtered wrappers, the bias state's two levels dropped"""
    kw = dict(kw)
    kw.update(kw.pop("sens"))
    f = kw.pop("filt")
    if parent:
        kw["filter"] = pkg.tracking.mag_filter_options(f["sigma_v"], f["sigma_m"], sigma_u=f["sigma_u"], p0_att=f["p0_att"], p0_bias=f["p0_bias"])
    else:
        kw["filter"] = pkg.tracking.mag_bias_filter_options(f["sigma_v"], f["sigma_m"], sigma_u=f["sigma_u"], sigma_c=f["sigma_c"],
                                                            p0_att=f["p0_att"], p0_bias=f["p0_bias"], p0_mag=f["p0_mag"])
    return kw


def _tv_run(pkg, solver, e, M, kw, batch=None, traj=True, est=True, parent=False):
    fn = pkg.tracking.attitude_ensemble_mag_filtered if parent else pkg.tracking.attitude_ensemble_mag_bias_filtered
    return fn(solver, batch or e["b"], e["X"], e["U"], _cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True, want_trajectories=traj,
              want_estimates=est, **STAT, **_wrap(pkg, kw, parent))


def _pd_run(pkg, solver, e, M, kw, batch=None, traj=True, est=True, parent=False):
    fn = pkg.tracking.attitude_ensemble_pd_mag_filtered if parent else pkg.tracking.attitude_ensemble_pd_mag_bias_filtered
    return fn(solver, batch or e["b"], _cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED, want_trajectories=traj, want_estimates=est, **STAT,
              **_wrap(pkg, kw, parent))


def _tv_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return mb.pairs_of(ol, pkg._abi, "tv", batch or e["b"], e["x0s"][:, :M], e["K"], e["o"], pairs, X=e["X"], U=e["U"], **kw)


def _pd_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return mb.pairs_of(ol, pkg._abi, "pd", batch or e["b"], e["x0s"][:, :M], (sc.KD, sc.KP), e["o"], pairs, **kw)


def _nomp(b):
    return np.array([(t, -1) for t in range(b.T)])


def _parity(pkg, ol, solver, e, M, law, kw, with_conditions=True, prediction=None, pairing=False, only_pairing=False):
    """34 seeded (t, m) drawn, the first 32 off the thresholds compared (at most 2 replaced): X_sim, stats, n_clipped, X_hat and
    filt_final; summary, zero fill and stats_nominal with them. The conditions are asserted first, on references alone, over the
    first N_COND compared pairs of full horizon. ``prediction``: whether the condition on the prediction across the delay is among
    them (default: under the TVLQR law; under the PD law it shows on the case of test_gpu_pd_prediction_across_the_delay).
    ``pairing``: likewise the row the delayed sample is paired with, which shows on ``mag_filtered_common.fast_table``
    (test_gpu_delayed_sample_is_paired_with_its_own_row, which asserts that one alone: ``only_pairing``)"""
    b = e["b"]
    ref_of, run = (_tv_ref, _tv_run) if law == "tv" else (_pd_ref, _pd_run)
    pairs = dc.sampled_pairs(b.T, M)
    ref = ref_of(pkg, ol, e, M, pairs, kw)
    keep = gc.kept(ref, e["o"])
    cp = pairs[keep[ref["n_knots"][keep] == b.N][:N_COND]]
    assert len(cp) == N_COND
    if only_pairing:
        pc.differs(ref_of(pkg, ol, e, M, cp, kw), ref_of(pkg, ol, e, M, cp, dict(kw, pair_own_row=False)),
                   "the delayed sample against r_{k-1}, not r_k")
    elif with_conditions:
        mb.conditions(lambda **o: ref_of(pkg, ol, e, M, cp, dict(kw, **o)), kw["sensor"], filt=kw["filt"],
                      prediction=(law == "tv") if prediction is None else prediction, pairing=pairing)
    got = run(pkg, solver, e, M, kw)
    dc.compare(ref, got, pairs, keep)
    mb.compare_estimates(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
    ec.same_stats(ref_of(pkg, ol, e, M, _nomp(b), kw)["stats"], got["nominal"])
    return ref, got, keep


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_tvlqr_matches_reference(pkg, ol, solver, ens, M, limits, latency):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront"""
    kw = _tv_kw(ens, M, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = _parity(pkg, ol, solver, ens, M, "tv", kw)
    ec.same_gains(ens["K"], got["K"])
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_pd_matches_reference(pkg, ol, solver, ens, M, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation saturates every
    component under the +-0.6 clip: it is compared under +-0.6 and under +-25, and asserts its conditions there"""
    kw = _pd_kw(ens, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = _parity(pkg, ol, solver, ens, M, "pd", kw, with_conditions=False)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    _parity(pkg, ol, solver, ens, M, "pd", kw)


@pytest.mark.parametrize("kind", ["track_ff", "regulate"])
def test_gpu_pd_prediction_across_the_delay(pkg, ol, solver, ens, kind):
    """the PD law at latency 1 on the case where the prediction across the delay shows: starts with the body rate FAST, limits
    +-25, M = 64; every condition, then parity"""
    e = dict(ens, x0s=ens["x0s"] + np.r_[mb.FAST, np.zeros(4)])
    _parity(pkg, ol, solver, e, 64, "pd", _pd_kw(e, kind, 0, 64, latency=1, sat=pc.WIDE), prediction=True)


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_gpu_delayed_sample_is_paired_with_its_own_row(pkg, ol, solver, ens, law):
    """latency 1 on ``mag_filtered_common.fast_table`` (rows that turn 25 deg from one to the next, the level this condition
    needs), limits +-25, M = 64: updating the delayed sample against r_k in the place of r_{k-1} moves the final state of the
    reference; then parity"""
    b = mb.fast_table(ens["b"])
    e = dict(ens, b=b, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains on these tables
    kw = _tv_kw(e, 64, latency=1, sat=pc.WIDE) if law == "tv" else _pd_kw(e, "track_ff", 0, 64, latency=1, sat=pc.WIDE)
    _parity(pkg, ol, solver, e, 64, law, kw, only_pairing=True)


def test_gpu_tiny_horizons_at_latency_1(pkg, ol, solver, ens):
    """n_knots = 2 (one command, from the first sample) and 3 (the first sample, then it predicted across the delay with no step
    made) among the slews, latency 1, M = 64"""
    e, M = ens, 64
    nk = e["b"].n_knots.copy()
    nk[[0, 5]], nk[[1, 7]] = 2, 3
    b = dataclasses.replace(e["b"], n_knots=nk)
    e = dict(e, K=ol.tvlqr_batch(b, e["X"], e["U"], *e["W"], e["X"][:, 0])["K"])      # the gains of the shortened horizons
    pairs = dc.sampled_pairs(b.T, M)
    for law, kw in (("tv", _tv_kw(e, M, latency=1)), ("pd", _pd_kw(e, "track_ff", 0, M, latency=1)), ("pd", _pd_kw(e, "regulate", 1, M, latency=1))):
        ref_of, run = (_tv_ref, _tv_run) if law == "tv" else (_pd_ref, _pd_run)
        ref = ref_of(pkg, ol, e, M, pairs, kw, batch=b)
        tiny = np.flatnonzero(ref["n_knots"] <= 3)
        assert set(ref["n_knots"][tiny]) == {2, 3}, "the sample must hold both tiny horizons"
        got = run(pkg, solver, e, M, kw, batch=b)
        t, m = pairs[tiny, 0], pairs[tiny, 1]
        d = float(np.max(np.abs(ref["X_sim"][tiny] - got["X_sim"][t, m])))
        print(f"{law}: tiny horizons, max|dX_sim| {d:.2e}")
        assert d < 1e-9
        # a tiny horizon has no sample past min_steps: nothing of it can sit on a threshold, and the margin is taken on the others
        big = np.flatnonzero(ref["n_knots"] > 3)
        o = e["o"]
        ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], o.min_steps, o.w_tol, o.angle_tol)
                       > dc.MARGIN for i in big])
        assert np.count_nonzero(~ok) <= dc.N_DRAWN - dc.N_KEPT, "more than 2 of the sampled realisations sit on a threshold"
        idx = np.concatenate([tiny, big[ok]])
        dc.compare(ref, got, pairs, idx)
        mb.compare_estimates(ref, got, pairs, idx)
        assert np.all(got["stats"]["failed"][t, m] == 1)
        ec.same_stats(ref_of(pkg, ol, e, M, _nomp(b), kw, batch=b)["stats"], got["nominal"])
        for s, n in enumerate(nk):
            assert np.all(got["X_sim"][s, :, n:] == 0) and np.all(got["X_hat"][s, :, n - 1:] == 0)
        # no step was made on a tiny horizon: the initial covariance, zero bias estimates
        f = mb.MBFILT
        want = np.r_[np.zeros(3), np.full(3, f["p0_att"]), np.full(3, f["p0_bias"]), np.zeros(3), np.full(3, f["p0_mag"])]
        np.testing.assert_allclose(got["filt_final"][t, m], np.broadcast_to(want, (len(tiny), 15)), rtol=1e-15, atol=0)
        # the second command of a 3-knot slew comes from the first sample predicted: the rate of row 1 is that of row 0
        three = pairs[tiny][ref["n_knots"][tiny] == 3]
        assert np.array_equal(got["X_hat"][three[:, 0], three[:, 1], 1, 0:3], got["X_hat"][three[:, 0], three[:, 1], 0, 0:3])


def _same_bytes(a, c, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_gpu_realisations_do_not_depend_on_m(pkg, solver, ens):
    """with explicit generator ids, realisations 0 .. 62 of the M = 64 run are the M = 63 run, byte for byte"""
    id0 = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
    for run, k63, k64 in ((_tv_run, _tv_kw(ens, 63, latency=1, noise_id0=id0), _tv_kw(ens, 64, latency=1, noise_id0=id0)),
                          (_pd_run, _pd_kw(ens, "regulate", 1, 63, latency=1, noise_id0=id0), _pd_kw(ens, "regulate", 1, 64, latency=1, noise_id0=id0)),
                          (_pd_run, _pd_kw(ens, "track_ff", 0, 63, noise_id0=id0), _pd_kw(ens, "track_ff", 0, 64, noise_id0=id0))):
        a, c = run(pkg, solver, ens, 63, k63), run(pkg, solver, ens, 64, k64)
        for k in ("stats", "X_sim", "n_clipped", "X_hat", "filt_final"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


def test_gpu_byte_equalities(pkg, solver, ens):
    """f = NULL is the sensed entry point byte for byte; X_hat / filt_final requested or not does not change the run"""
    e, b, M = ens, ens["b"], 64
    lib, abi = pkg._abi.load(), pkg._abi
    for latency in (0, 1):
        tvkw, pdkw = _tv_kw(e, M, latency=latency), _pd_kw(e, "track_ff", 1, M, latency=latency)
        for fn_f, fn_s, new, old in (
                (lib.tsat_tvlqr_ensemble_mag_bias_filtered, lib.tsat_tvlqr_ensemble_sensed,
                 mb.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **dict(tvkw, filt=None)),
                 sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **{k: v for k, v in tvkw.items() if k != "filt"})),
                (lib.tsat_pd_ensemble_mag_bias_filtered, lib.tsat_pd_ensemble_sensed,
                 mb.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **dict(pdkw, filt=None)),
                 sc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **{k: v for k, v in pdkw.items() if k != "filt"}))):
            assert fn_f(solver._h, *new.c_args()) == 0 and fn_s(solver._h, *old.c_args()) == 0
            _same_bytes(new.result(), old.result())
        a = _tv_run(pkg, solver, e, M, tvkw)
        _same_bytes(a, _tv_run(pkg, solver, e, M, tvkw, est=False))
        sensed = pkg.tracking.attitude_ensemble_sensed(solver, b, e["X"], e["U"], _cut(e["x0s"], M), *e["W"], ec.SEED, want_trajectories=True,
                                                       **STAT, **{k: v for k, v in _wrap(pkg, tvkw).items() if k != "filter"})
        assert np.max(np.abs(a["X_sim"] - sensed["X_sim"])) >= gc.MOVED
        a = _pd_run(pkg, solver, e, M, pdkw)
        c = _pd_run(pkg, solver, e, M, pdkw, est=False)
        _same_bytes(a, c)
        assert c["X_hat"] is None and a["filt_final"].tobytes() == c["filt_final"].tobytes()


def test_gpu_reduction_to_the_mag_filter(pkg, solver, ens):
    """p0_mag = sigma_c = 0: the call equals the mag-filtered call of the same run on X_sim, X_hat and filt_final[0:9] to 1e-12 (byte
    equality is not demanded: the compiler may contract differently), filt_final[9:15] is exactly 0; with the bias state on the run
    is another one. Both laws, both latencies, M = 64"""
    e, M = ens, 64
    off = dict(mb.MBFILT, p0_mag=0.0, sigma_c=0.0)
    worst = 0.0
    for latency in (0, 1):
        for run, kw in ((_tv_run, _tv_kw(e, M, latency=latency, filt=off)), (_pd_run, _pd_kw(e, "track_ff", 1, M, latency=latency, filt=off)),
                        (_pd_run, _pd_kw(e, "regulate", 0, M, latency=latency, filt=off, sat=pc.WIDE))):
            new, old = run(pkg, solver, e, M, kw), run(pkg, solver, e, M, kw, parent=True)
            d = max(float(np.max(np.abs(new["X_sim"] - old["X_sim"]))), float(np.max(np.abs(new["X_hat"] - old["X_hat"]))),
                    float(np.max(np.abs(new["filt_final"][..., 0:9] - old["filt_final"]))))
            worst = max(worst, d)
            assert np.all(new["filt_final"][..., 9:15] == 0.0)
            on = run(pkg, solver, e, M, dict(kw, filt=mb.MBFILT))
            assert np.max(np.abs(on["X_sim"] - new["X_sim"])) >= gc.MOVED and np.abs(on["filt_final"][..., 9:12]).min() > 0
    print(f"reduction to the mag-filtered calls at p0_mag = sigma_c = 0: max difference {worst:.1e}")
    assert worst < 1e-12


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every rejection returns -1 with its text and leaves the handle's workspaces empty; a good call grows them by exactly what its
    sensed parent's call grows them by"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    abi = pkg._abi
    pd = mb.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **_pd_kw(e, "track_ff", 0, M))
    tv = mb.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **_tv_kw(e, M))
    _trim(pkg, solver)
    null_f = [("f NULL with X_hat", lambda c: c.edit(f=None), "X_hat and filt_final must be NULL"),
              ("f NULL with filt_final", lambda c: c.edit(f=None, X_hat=None), "X_hat and filt_final must be NULL")]
    tv_parent = [("Rtab NULL, gm != 0", tv.edit(Rtab=None), "Rtab is NULL but gm != 0"),
                 ("one limit NULL", tv.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"), ("X NULL", tv.edit(X=None), "null array")]
    for fn, call, cases in ((lib.tsat_pd_ensemble_mag_bias_filtered, pd,
                             mb.filter_rejections(pd) + sc.sensor_rejections(pd) + pc.rejections(pd, b, e["Rtab"])),
                            (lib.tsat_tvlqr_ensemble_mag_bias_filtered, tv, mb.filter_rejections(tv) + sc.sensor_rejections(tv) + tv_parent)):
        for label, bad, words in cases + [(l, ed(call), w) for l, ed, w in null_f]:
            rc = fn(solver._h, *bad.c_args())
            msg = lib.tsat_ensemble_last_error().decode()
            assert rc == -1 and words in msg, (label, rc, msg)
            assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    # good calls: the sensed parent's bytes, nothing more
    sens_tv = sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **{k: v for k, v in _tv_kw(e, M).items() if k != "filt"})
    assert lib.tsat_tvlqr_ensemble_sensed(solver._h, *sens_tv.c_args()) == 0
    parent = _ws(pkg, solver)
    _trim(pkg, solver)
    assert lib.tsat_tvlqr_ensemble_mag_bias_filtered(solver._h, *tv.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent and parent >= 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]
    _trim(pkg, solver)
    sens_pd = sc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **{k: v for k, v in _pd_kw(e, "track_ff", 0, M).items() if k != "filt"})
    assert lib.tsat_pd_ensemble_sensed(solver._h, *sens_pd.c_args()) == 0
    parent = _ws(pkg, solver)
    _trim(pkg, solver)
    assert lib.tsat_pd_ensemble_mag_bias_filtered(solver._h, *pd.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, as tsat_pd_ensemble
    assert lib.tsat_tvlqr_ensemble_mag_bias_filtered(solver._h, *tv.edit(plant=None, Rtab=None, gm=0.0).c_args()) == 0
    _trim(pkg, solver)


@pytest.mark.parametrize("latency", [0, 1])
def test_gpu_zero_row_inside_the_horizon(pkg, ol, solver, ens, latency):
    """row 5 of field table 0 set to zero: under the case's clock (row floor(0.25 + 0.9 k)) it is the stage-0 row of knot 6 of every
    slew on that table whose horizon reaches it, so the filter makes an update against r = 0 there, at both latencies — H = 0 and
    z = b_m - c^ observing c directly — and the plant flies a stage without a field. Results finite, and parity of both laws"""
    b0 = ens["b"]
    B = b0.Btab.copy()
    B[0, 5] = 0.0
    b = dataclasses.replace(b0, Btab=np.ascontiguousarray(B))
    assert any(np.array_equal(dc._row(b, t, 6, 0.0), np.zeros(3)) and b.n_knots[t] > 8 for t in range(b.T))
    e = dict(ens, b=b, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains on this table
    for law, kw in (("tv", _tv_kw(e, 64, latency=latency, sat=pc.WIDE)), ("pd", _pd_kw(e, "track_ff", 1, 64, latency=latency))):
        ref, got, keep = _parity(pkg, ol, solver, e, 64, law, kw, with_conditions=False)
        assert np.isfinite(got["X_hat"]).all() and np.isfinite(got["filt_final"]).all() and np.isfinite(ref["X_hat"]).all()


def test_gpu_filter_on_a_long_horizon(pkg, ol, solver):
    """T = 1, N = 400, M = 8 (mag_bias_filtered_common.long_case: mag_filtered_common.long_case's batch, starts, generator ids and
    gyro figures, a magnetometer bias of 3e-6 T in a drawn direction per realisation, p0_mag = 3e-6, sigma_c = 0). On the references
    alone: the mean over the 8 realisations of the rms attitude error of X_hat over the last half is below the six-state mag
    filter's on the same samples (measured 3.32 deg against 6.43 deg), it is below it individually on at least 6 of the 8 (measured
    7, worst ratio 1.06), and |c^ - c| < 0.5 |c| on every realisation (measured at most 0.28); a reference that does not give these
    figures to their printed digits is wrong. Then the kernel against the reference to 1e-9 on X_sim, X_hat and filt_final"""
    c = mb.long_case(pkg, ol, N=400, M=8)
    assert len(c["pairs"]) == 8
    fig = mb.assert_filter_works(c)
    assert (round(fig["est"], 2), round(fig["mag"], 2), fig["better"], round(fig["worst"], 2), round(fig["rel"], 2)) == (3.32, 6.43, 7, 1.06, 0.28)
    got = pkg.tracking.attitude_ensemble_pd_mag_bias_filtered(solver, c["b"], c["x0s"], sc.KD, sc.KP, ec.SEED, want_trajectories=True,
                                                              want_estimates=True, **STAT, **_wrap(pkg, c["kw"]))
    dc.compare(c["ref"], got, c["pairs"])
    mb.compare_estimates(c["ref"], got, c["pairs"])
