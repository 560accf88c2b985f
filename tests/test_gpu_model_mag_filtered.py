"""GPU tier of the ensemble controllers behind the model-based rate filter updated by the magnetometer
(tsat_tvlqr_ensemble_model_mag_filtered, tsat_pd_ensemble_model_mag_filtered through ``tracking.attitude_ensemble_model_mag_filtered``
/ ``attitude_ensemble_pd_model_mag_filtered``) against the reference of tests/model_mag_filtered_common.py, on the smallest shapes at
which the kernels can go wrong. The bars are the parents' (dispersed_common.compare) and 1e-9 on X_hat and filt_final. Every parity
test first asserts its conditions on references alone (model_mag_filtered_common.conditions, bar 1e-7), over the first N_COND compared
pairs of full horizon; which case carries which condition is stated in tests/test_model_mag_filtered.py, whose cases these are.

The case is tests/test_gpu_mag_filtered.py's — ``pd_common.case``, 8 slews, N = 20, ragged horizons, all five plant dispersions, plant
noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels sensed_common.SIGMAS / BIAS — with
the filter levels model_mag_filtered_common.FILT. The plan is solved once per module at the 1 x 3 budget; the gains of the references
are the oracle's."""
import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mag_filtered_common as gfc
import model_mag_filtered_common as mc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")


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


def _wrap(pkg, kw):
    """the reference's keyword arguments as the wrapper takes them: ``sens`` spread into sigma_*, ``filt`` as ``filter``"""
    kw = dict(kw)
    kw.update(kw.pop("sens"))
    f = kw.pop("filt")
    kw["filter"] = pkg.tracking.model_mag_filter_options(f["sigma_w"], f["sigma_g"], f["sigma_m"], sigma_v=f["sigma_v"], sigma_u=f["sigma_u"],
                                                         p0_att=f["p0_att"], p0_bias=f["p0_bias"])
    return kw


@pytest.fixture(scope="module")
def run(pkg, solver):
    """the tier's call: the library through ``tracking``"""
    tr = pkg.tracking

    def call(law, e, M, kw, batch=None, traj=True, est=True):
        b = batch or e["b"]
        if law == "tv":
            return tr.attitude_ensemble_model_mag_filtered(solver, b, e["X"], e["U"], mc.cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True,
                                                           want_trajectories=traj, want_estimates=est, **STAT, **_wrap(pkg, kw))
        return tr.attitude_ensemble_pd_model_mag_filtered(solver, b, mc.cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED, want_trajectories=traj,
                                                          want_estimates=est, **STAT, **_wrap(pkg, kw))
    return call


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_tvlqr_matches_reference(pkg, ol, run, ens, M, limits, latency):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront"""
    kw = mc.tv_kw(ens, M, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = mc.parity(pkg, ol, run, ens, M, "tv", kw)
    ec.same_gains(ens["K"], got["K"])
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_pd_matches_reference(pkg, ol, run, ens, M, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation saturates every
    component under the +-0.6 clip: it is compared under +-0.6 and under +-25, and asserts its conditions there"""
    kw = mc.pd_kw(ens, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = mc.parity(pkg, ol, run, ens, M, "pd", kw, skip=None)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    mc.parity(pkg, ol, run, ens, M, "pd", kw)


def _law(e, law, M, **over):
    if law == "tv":
        return "tv", mc.tv_kw(e, M, **over)
    return "pd", mc.pd_kw(e, "regulate" if law == "pd_regulate" else "track_ff", 1 if law == "pd_regulate" else 0, M, **over)


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd", "pd_regulate"])
def test_gpu_fast_starts(pkg, ol, run, ens, law, latency):
    """the body rate filtered_common.FAST added to the starts, limits +-25, M = 64: the case that carries the command in predict,
    the gyroscopic term of Phi_ww and, at latency 1, the prediction across the delay; those conditions, then parity"""
    e = dict(ens, x0s=ens["x0s"] + np.r_[mc.FAST, np.zeros(4)])
    law, kw = _law(e, law, 64, latency=latency, sat=pc.WIDE)
    mc.parity(pkg, ol, run, e, 64, law, kw, only=(mc.COMMAND, mc.GYROSCOPIC) + ((mc.DELAY,) if latency else ()))


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("law", ["tv", "pd"])
def test_gpu_loud_sensor_shows_the_update_order(pkg, ol, run, ens, law, latency):
    """the sensor and filter levels LOUD_SENS / LOUD_FILT, limits +-25, M = 64: the case that carries the order of the two updates;
    that condition, then parity"""
    law, kw = _law(ens, law, 64, latency=latency, sat=pc.WIDE, sens=mc.LOUD_SENS, filt=mc.LOUD_FILT)
    mc.parity(pkg, ol, run, ens, 64, law, kw, only=(mc.ORDER,))


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_gpu_delayed_sample_is_paired_with_its_own_row(pkg, ol, run, ens, law):
    """latency 1 on ``mag_filtered_common.fast_table`` (rows that turn 25 deg from one to the next), limits +-25, M = 64: updating
    the delayed sample against r_k in the place of r_{k-1} moves the final state of the reference; then parity"""
    b = gfc.fast_table(ens["b"])
    e = dict(ens, b=b, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains on these tables
    law, kw = _law(e, law, 64, latency=1, sat=pc.WIDE)
    mc.parity(pkg, ol, run, e, 64, law, kw, only=(mc.PAIRING,))


def test_gpu_tiny_horizons_at_latency_1(pkg, ol, run, ens):
    """n_knots = 2, 3 and 4 among the slews at latency 1, M = 64 (model_mag_filtered_common.check_tiny): with 2 ``first`` only and
    filt_final is ``first_record``; with 3, k = 1 makes no update; with 4, one update"""
    b = mc.tiny_batch(ens["b"])
    e = dict(ens, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains of the shortened horizons
    mc.check_tiny(pkg, ol, run, e, 64, b)


@pytest.mark.parametrize("latency", [0, 1])
def test_gpu_zero_row_inside_the_horizon(pkg, ol, run, ens, latency):
    """row 5 of field table 0 set to zero (model_mag_filtered_common.zero_row_batch): the filter makes an update against r = 0
    (Hm = 0, K = 0) at knot 6, at both latencies, and the plant flies a stage without a field. Parity of both laws shows that the
    row puts no NaN into X_hat"""
    b = mc.zero_row_batch(ens["b"])
    e = dict(ens, b=b, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains on this table
    for law, kw in (("tv", mc.tv_kw(e, 64, latency=latency, sat=pc.WIDE)), ("pd", mc.pd_kw(e, "track_ff", 1, 64, latency=latency))):
        ref, got, keep = mc.parity(pkg, ol, run, e, 64, law, kw, skip=None)
        assert np.isfinite(got["X_hat"]).all() and np.isfinite(got["filt_final"]).all() and np.isfinite(ref["X_hat"]).all()


def _same_bytes(a, c, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_gpu_realisations_do_not_depend_on_m(pkg, run, ens):
    """with explicit generator ids, realisations 0 .. 62 of the M = 64 run are the M = 63 run, byte for byte"""
    id0 = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
    for law, k63, k64 in (("tv", mc.tv_kw(ens, 63, latency=1, noise_id0=id0), mc.tv_kw(ens, 64, latency=1, noise_id0=id0)),
                          ("pd", mc.pd_kw(ens, "regulate", 1, 63, latency=1, noise_id0=id0), mc.pd_kw(ens, "regulate", 1, 64, latency=1, noise_id0=id0)),
                          ("pd", mc.pd_kw(ens, "track_ff", 0, 63, noise_id0=id0), mc.pd_kw(ens, "track_ff", 0, 64, noise_id0=id0))):
        a, c = run(law, ens, 63, k63), run(law, ens, 64, k64)
        for k in ("stats", "X_sim", "n_clipped", "X_hat", "filt_final"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


def test_gpu_byte_equalities(pkg, solver, run, ens):
    """f = NULL is the sensed entry point byte for byte, and differs from the sensed wrapper's run of the same call not at all; twice
    the same call gives the same bytes (``load`` zeroes the record); X_hat / filt_final requested or not does not change the run"""
    e, b, M = ens, ens["b"], 64
    lib, abi = pkg._abi.load(), pkg._abi
    for latency in (0, 1):
        tvkw, pdkw = mc.tv_kw(e, M, latency=latency), mc.pd_kw(e, "track_ff", 1, M, latency=latency)
        for fn_f, fn_s, new, old in (
                (lib.tsat_tvlqr_ensemble_model_mag_filtered, lib.tsat_tvlqr_ensemble_sensed,
                 mc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **dict(tvkw, filt=None)),
                 sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **{k: v for k, v in tvkw.items() if k != "filt"})),
                (lib.tsat_pd_ensemble_model_mag_filtered, lib.tsat_pd_ensemble_sensed,
                 mc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **dict(pdkw, filt=None)),
                 sc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **{k: v for k, v in pdkw.items() if k != "filt"}))):
            assert fn_f(solver._h, *new.c_args()) == 0 and fn_s(solver._h, *old.c_args()) == 0
            _same_bytes(new.result(), old.result())
        a = run("tv", e, M, tvkw)
        _same_bytes(a, run("tv", e, M, tvkw), keys=OUT + ("X_hat", "filt_final"))
        _same_bytes(a, run("tv", e, M, tvkw, est=False))
        sensed = pkg.tracking.attitude_ensemble_sensed(solver, b, e["X"], e["U"], mc.cut(e["x0s"], M), *e["W"], ec.SEED, want_trajectories=True,
                                                       **STAT, **{k: v for k, v in _wrap(pkg, tvkw).items() if k != "filter"})
        assert np.max(np.abs(a["X_sim"] - sensed["X_sim"])) >= gc.MOVED
        a = run("pd", e, M, pdkw)
        _same_bytes(a, run("pd", e, M, pdkw), keys=OUT + ("X_hat", "filt_final"))
        c = run("pd", e, M, pdkw, est=False)
        _same_bytes(a, c)
        assert c["X_hat"] is None and a["filt_final"].tobytes() == c["filt_final"].tobytes()


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every rejection returns -1 with its text and leaves the handle's workspaces empty; a good call grows them by exactly what its
    sensed parent's call grows them by"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    abi = pkg._abi
    pd = mc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **mc.pd_kw(e, "track_ff", 0, M))
    tv = mc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **mc.tv_kw(e, M))
    pd_fn, tv_fn = lib.tsat_pd_ensemble_model_mag_filtered, lib.tsat_tvlqr_ensemble_model_mag_filtered
    _trim(pkg, solver)
    null_f = [("f NULL with X_hat", lambda c: c.edit(f=None), "X_hat and filt_final must be NULL"),
              ("f NULL with filt_final", lambda c: c.edit(f=None, X_hat=None), "X_hat and filt_final must be NULL")]
    tv_parent = [("Rtab NULL, gm != 0", tv.edit(Rtab=None), "Rtab is NULL but gm != 0"),
                 ("one limit NULL", tv.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"), ("X NULL", tv.edit(X=None), "null array")]
    for fn, call, cases in ((pd_fn, pd, mc.filter_rejections(pd) + sc.sensor_rejections(pd) + pc.rejections(pd, b, e["Rtab"])),
                            (tv_fn, tv, mc.filter_rejections(tv) + sc.sensor_rejections(tv) + tv_parent)):
        for label, bad, words in cases + [(l, ed(call), w) for l, ed, w in null_f]:
            rc = fn(solver._h, *bad.c_args())
            msg = lib.tsat_ensemble_last_error().decode()
            assert rc == -1 and words in msg, (label, rc, msg)
            assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    # good calls: the sensed parent's bytes, nothing more
    sens_tv = sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **{k: v for k, v in mc.tv_kw(e, M).items() if k != "filt"})
    assert lib.tsat_tvlqr_ensemble_sensed(solver._h, *sens_tv.c_args()) == 0
    parent = _ws(pkg, solver)
    _trim(pkg, solver)
    assert tv_fn(solver._h, *tv.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent and parent >= 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]
    _trim(pkg, solver)
    sens_pd = sc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **{k: v for k, v in mc.pd_kw(e, "track_ff", 0, M).items() if k != "filt"})
    assert lib.tsat_pd_ensemble_sensed(solver._h, *sens_pd.c_args()) == 0
    parent = _ws(pkg, solver)
    _trim(pkg, solver)
    assert pd_fn(solver._h, *pd.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, as tsat_pd_ensemble
    assert tv_fn(solver._h, *tv.edit(plant=None, Rtab=None, gm=0.0).c_args()) == 0
    _trim(pkg, solver)


def test_gpu_filter_on_a_long_horizon(pkg, ol, solver):
    """T = 1, N = 400, M = 8 (model_mag_filtered_common.long_case). On the references alone, rms over the last half: the rate error
    of the estimate below 0.25 x the raw sample's (measured 9.2e-4 rad/s against 1.17e-2, ratio 0.08); the attitude error below gyro
    dead reckoning's on every realisation (4.19 deg worst against 6.10 deg best) and its mean no worse than 1.10 x the mag filter's
    (2.77 deg against 3.01 deg); |b^ - b_w| < GYRO_BIAS on every realisation (at most 1.2e-3 against 2e-3). Then the kernel against
    the reference to 1e-9 on X_sim, X_hat and filt_final"""
    c = mc.long_case(pkg, ol, N=400, M=8)
    assert len(c["pairs"]) == 8
    mc.assert_filter_works(c)
    got = pkg.tracking.attitude_ensemble_pd_model_mag_filtered(solver, c["b"], c["x0s"], sc.KD, sc.KP, ec.SEED, want_trajectories=True,
                                                               want_estimates=True, **STAT, **_wrap(pkg, c["kw"]))
    dc.compare(c["ref"], got, c["pairs"])
    mc.compare_estimates(c["ref"], got, c["pairs"])
