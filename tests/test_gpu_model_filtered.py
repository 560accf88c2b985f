"""GPU tier of the ensemble controllers behind the model-based rate filter (tsat_tvlqr_ensemble_model_filtered,
tsat_pd_ensemble_model_filtered through ``tracking.attitude_ensemble_model_filtered`` / ``attitude_ensemble_pd_model_filtered``) against
the reference of tests/model_filtered_common.py, on the smallest shapes at which the kernels can go wrong: tests/test_gpu_filtered.py's.
The bars are the parents' (dispersed_common.compare) and 1e-9 on X_hat and filt_final. Every parity test first asserts its conditions
on references alone (model_filtered_common.conditions, bar gg_common.MOVED = 1e-7 on the final states), over the first N_COND compared
pairs of full horizon, and prints every figure.

The case is tests/test_gpu_sensed.py's — ``pd_common.case``, 8 slews, N = 20, ragged horizons, all five plant dispersions, plant
noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels sensed_common.SIGMAS / BIAS — with
the filter levels model_filtered_common.FILT. The plan is solved once per module at the 1 x 3 budget; the gains of the references are
the oracle's.

Which case shows which term: on the case's own starts and levels every term of ``model_filtered_common.terms_of`` and, at latency 1,
the prediction across the delay, except
  - the gyroscopic term of Phi_ww (size h |w| (J_i - J_j) / J_k): the starts with the body rate filtered_common.FAST,
    test_gpu_fast_starts (both laws, regulation included, both latencies);
  - the command in predict under the PD law when it regulates or flies the direction-preserving limit: the FAST starts too;
  - the prediction across the delay under the PD law (7e-8 .. 2e-7 at the case's own rates, as with the six-state filter): the
    FAST starts too;
  - the order of the two updates (it acts only through the second-order term of the quaternion correction): the sensor levels
    model_filtered_common.LOUD_SENS, test_gpu_loud_sensor_shows_the_update_order (both laws, both latencies)."""
import dataclasses

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import model_filtered_common as mc
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
KINDS = ("track", "track_ff", "regulate")
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")
N_COND = 4          # compared pairs the conditions are evaluated on: shown on a part of them, they hold on all
LEFT = (mc.GYROSCOPIC, mc.ORDER)


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
              filt=mc.FILT)
    kw.update(over)
    return kw


def _pd_kw(e, kind, mode, M, **over):
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"], gm=gc.GM,
              plant=_cut(e["plant"], M), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"], sens=sc.SIGMAS, latency=0, sensor=_cut(e["sensor"], M),
              filt=mc.FILT)
    kw.update(over)
    return kw


def _wrap(pkg, kw):
    kw = dict(kw)
    kw.update(kw.pop("sens"))
    f = kw.pop("filt")
    kw["filter"] = pkg.tracking.model_filter_options(f["sigma_w"], f["sigma_g"], f["sigma_a"], sigma_v=f["sigma_v"], sigma_u=f["sigma_u"],
                                                     p0_att=f["p0_att"], p0_bias=f["p0_bias"])
    return kw


def _tv_run(pkg, solver, e, M, kw, batch=None, traj=True, est=True):
    return pkg.tracking.attitude_ensemble_model_filtered(solver, batch or e["b"], e["X"], e["U"], _cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True,
                                                   want_trajectories=traj, want_estimates=est, **STAT, **_wrap(pkg, kw))


def _pd_run(pkg, solver, e, M, kw, batch=None, traj=True, est=True):
    return pkg.tracking.attitude_ensemble_pd_model_filtered(solver, batch or e["b"], _cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED,
                                                      want_trajectories=traj, want_estimates=est, **STAT, **_wrap(pkg, kw))


def _tv_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return mc.pairs_of(ol, pkg._abi, "tv", batch or e["b"], e["x0s"][:, :M], e["K"], e["o"], pairs, X=e["X"], U=e["U"], **kw)


def _pd_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return mc.pairs_of(ol, pkg._abi, "pd", batch or e["b"], e["x0s"][:, :M], (sc.KD, sc.KP), e["o"], pairs, **kw)


def _nomp(b):
    return np.array([(t, -1) for t in range(b.T)])


def _cond_pairs(b, ref, pairs, keep):
    cp = pairs[keep[ref["n_knots"][keep] == b.N][:N_COND]]
    assert len(cp) == N_COND
    return cp


def _parity(pkg, ol, solver, e, M, law, kw, skip=LEFT, with_conditions=True):
    """34 seeded (t, m) drawn, the first 32 off the thresholds compared (at most 2 replaced): X_sim, stats, n_clipped, X_hat and
    filt_final; summary, zero fill and stats_nominal with them. The conditions are asserted on references alone, over the first
    N_COND compared pairs of full horizon; ``skip`` names those left to the test that flies the case on which they show"""
    b = e["b"]
    ref_of, run = (_tv_ref, _tv_run) if law == "tv" else (_pd_ref, _pd_run)
    pairs = dc.sampled_pairs(b.T, M)
    ref = ref_of(pkg, ol, e, M, pairs, kw)
    keep = gc.kept(ref, e["o"])
    if with_conditions:
        cp = _cond_pairs(b, ref, pairs, keep)
        mc.conditions(lambda **o: ref_of(pkg, ol, e, M, cp, dict(kw, **o)), kw["sensor"], kw["latency"], skip=skip, filt=kw["filt"])
    got = run(pkg, solver, e, M, kw)
    dc.compare(ref, got, pairs, keep)
    mc.compare_estimates(ref, got, pairs, keep)
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
    _parity(pkg, ol, solver, ens, M, "pd", kw, skip=LEFT + (mc.DELAY[0],) + ((mc.COMMAND,) if (kind == "regulate" or mode == 1) else ()))


def _law(e, law, M, **over):
    if law == "tv":
        return "tv", _tv_kw(e, M, **over)
    return "pd", _pd_kw(e, "regulate" if law == "pd_regulate" else "track_ff", 1 if law == "pd_regulate" else 0, M, **over)


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd", "pd_regulate"])
def test_gpu_fast_starts(pkg, ol, solver, ens, law, latency):
    """the starts with the body rate filtered_common.FAST, limits +-25, M = 64: the case on which the gyroscopic term of Phi_ww
    shows, and the command in predict under regulation; every condition but the update order, then parity"""
    e = dict(ens, x0s=ens["x0s"] + np.r_[mc.FAST, np.zeros(4)])
    name, kw = _law(e, law, 64, latency=latency, sat=pc.WIDE)
    _parity(pkg, ol, solver, e, 64, name, kw, skip=(mc.ORDER,))


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd"])
def test_gpu_loud_sensor_shows_the_update_order(pkg, ol, solver, ens, law, latency):
    """the sensor and filter levels model_filtered_common.LOUD_SENS / LOUD_FILT, limits +-25, M = 64: the case on which the order of
    the two updates shows; that condition on references alone, then parity"""
    e, M, b = ens, 64, ens["b"]
    name, kw = _law(e, law, M, latency=latency, sat=pc.WIDE, sens=mc.LOUD_SENS, filt=mc.LOUD_FILT)
    ref_of = _tv_ref if name == "tv" else _pd_ref
    pairs = dc.sampled_pairs(b.T, M)
    ref = ref_of(pkg, ol, e, M, pairs, kw)
    cp = _cond_pairs(b, ref, pairs, gc.kept(ref, e["o"]))
    d = mc.moved(ref_of(pkg, ol, e, M, cp, kw), ref_of(pkg, ol, e, M, cp, dict(kw, variant=dict(mc.VARIANT, order="ba"))))
    print(f"  condition: {mc.ORDER}: max|d final state| {d:.2e}")
    assert d >= gc.MOVED
    _parity(pkg, ol, solver, e, M, name, kw, with_conditions=False)


def test_gpu_tiny_horizons_at_latency_1(pkg, ol, solver, ens):
    """n_knots = 2 (one command, from the first sample) and 3 (the first sample, then the model's prediction from it with no update
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
        mc.compare_estimates(ref, got, pairs, idx)
        assert np.all(got["stats"]["failed"][t, m] == 1)
        ec.same_stats(ref_of(pkg, ol, e, M, _nomp(b), kw, batch=b)["stats"], got["nominal"])
        for s, n in enumerate(nk):
            assert np.all(got["X_sim"][s, :, n:] == 0) and np.all(got["X_hat"][s, :, n - 1:] == 0)
        # no update was made on a tiny horizon: filt_final is the record of `first`
        np.testing.assert_allclose(got["filt_final"][t, m], np.broadcast_to(mc.first_record(mc.FILT), (len(tiny), 12)), rtol=1e-15, atol=0)


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
    """f = NULL is the sensed entry point byte for byte; X_hat / filt_final requested or not does not change the run; the filtered
    run differs from the sensed one by at least gg_common.MOVED"""
    e, b, M = ens, ens["b"], 64
    lib, abi = pkg._abi.load(), pkg._abi
    for latency in (0, 1):
        tvkw, pdkw = _tv_kw(e, M, latency=latency), _pd_kw(e, "track_ff", 1, M, latency=latency)
        for fn_f, fn_s, new, old in (
                (lib.tsat_tvlqr_ensemble_model_filtered, lib.tsat_tvlqr_ensemble_sensed,
                 mc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **dict(tvkw, filt=None)),
                 sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **{k: v for k, v in tvkw.items() if k != "filt"})),
                (lib.tsat_pd_ensemble_model_filtered, lib.tsat_pd_ensemble_sensed,
                 mc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **dict(pdkw, filt=None)),
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


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every rejection returns -1 with its text and leaves the handle's workspaces empty; a good call grows them by exactly what its
    sensed parent's call grows them by"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    abi = pkg._abi
    pd = mc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **_pd_kw(e, "track_ff", 0, M))
    tv = mc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **_tv_kw(e, M))
    _trim(pkg, solver)
    null_f = [("f NULL with X_hat", lambda c: c.edit(f=None), "X_hat and filt_final must be NULL"),
              ("f NULL with filt_final", lambda c: c.edit(f=None, X_hat=None), "X_hat and filt_final must be NULL")]
    tv_parent = [("Rtab NULL, gm != 0", tv.edit(Rtab=None), "Rtab is NULL but gm != 0"),
                 ("one limit NULL", tv.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"), ("X NULL", tv.edit(X=None), "null array")]
    for fn, call, cases in ((lib.tsat_pd_ensemble_model_filtered, pd, mc.filter_rejections(pd) + sc.sensor_rejections(pd) + pc.rejections(pd, b, e["Rtab"])),
                            (lib.tsat_tvlqr_ensemble_model_filtered, tv, mc.filter_rejections(tv) + sc.sensor_rejections(tv) + tv_parent)):
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
    assert lib.tsat_tvlqr_ensemble_model_filtered(solver._h, *tv.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent and parent >= 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]
    _trim(pkg, solver)
    assert lib.tsat_pd_ensemble_model_filtered(solver._h, *pd.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, as tsat_pd_ensemble
    assert lib.tsat_tvlqr_ensemble_model_filtered(solver._h, *tv.edit(plant=None, Rtab=None, gm=0.0).c_args()) == 0
    _trim(pkg, solver)


def test_gpu_filter_on_a_long_horizon(pkg, ol, solver):
    """T = 1, N = 400, M = 8 (model_filtered_common.long_case, sigma_w = LONG_SIGMA_W). On the references alone, over the last half:
    the rms rate error of the estimate is below a quarter of the raw sample's, the attitude error no worse than the six-state
    reference's on the same draws within 10 %, the bias estimate inside 3 x its own sqrt(diag P_bb) on every realisation (all
    printed); then the kernel against the reference to 1e-9 on X_sim, X_hat and filt_final"""
    c = mc.long_case(pkg, ol, N=400, M=8)
    mc.assert_filter_works(c)
    got = pkg.tracking.attitude_ensemble_pd_model_filtered(solver, c["b"], c["x0s"], sc.KD, sc.KP, ec.SEED, want_trajectories=True,
                                                           want_estimates=True, **STAT, **_wrap(pkg, c["kw"]))
    dc.compare(c["ref"], got, c["pairs"])
    mc.compare_estimates(c["ref"], got, c["pairs"])
