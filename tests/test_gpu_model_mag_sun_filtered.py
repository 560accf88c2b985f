"""GPU tier of the ensemble controllers behind the magnetometer-updated model filter with a sun sensor that eclipse blinds
(tsat_tvlqr_ensemble_model_mag_sun_filtered, tsat_pd_ensemble_model_mag_sun_filtered through
``tracking.attitude_ensemble_model_mag_sun_filtered`` / ``attitude_ensemble_pd_model_mag_sun_filtered``) against the reference of
tests/model_mag_sun_filtered_common.py, on the smallest shapes at which the kernels can go wrong. The bars are the parents'
(dispersed_common.compare) and 1e-9 on X_hat and filt_final. Every parity test first asserts its conditions on references alone
(model_mag_sun_filtered_common.conditions, bar 1e-7); the cases are those of tests/test_model_mag_sun_filtered.py.

Besides the matrix: a table dark throughout and Stab = NULL against tsat_*_model_mag_filtered OF THE SAME RUN (max |d| = 0), f = NULL
against the sensed call (equal bytes), the library against the emulated kernels at M = 70 in every combination of law, limit mode and
latency, rejections that leave the handle's workspaces as they were (the packed sun rows are one of them), and one long horizon."""
import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import model_mag_filtered_common as mc
import model_mag_sun_filtered_common as uc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")
EST = OUT + ("X_hat", "filt_final")


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
    """the plan (solved here, 1 x 3 budget), the oracle's gains of it, 70 realisations, their plants and sensor biases, the sun
    tables; computed once and left unchanged"""
    to = pkg.trajopt
    b, Rtab = pc.case(pkg)
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    r = to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    W = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], *W, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 70, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=W, K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 70),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, 70), Stab=uc.sun_table(b))


def _wrap(pkg, kw):
    """the reference's keyword arguments as the wrapper takes them: ``sens`` spread into sigma_*, ``filt`` as ``filter``"""
    kw = dict(kw)
    kw.update(kw.pop("sens"))
    f = kw.pop("filt")
    kw["filter"] = pkg.tracking.model_mag_sun_filter_options(f["sigma_w"], f["sigma_g"], f["sigma_m"], f["sigma_s"], sigma_v=f["sigma_v"],
                                                             sigma_u=f["sigma_u"], p0_att=f["p0_att"], p0_bias=f["p0_bias"])
    return kw


def _wrap_parent(pkg, kw):
    kw = dict(uc.parent_kw(kw))
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
            return tr.attitude_ensemble_model_mag_sun_filtered(solver, b, e["X"], e["U"], uc.cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True,
                                                               want_trajectories=traj, want_estimates=est, **STAT, **_wrap(pkg, kw))
        return tr.attitude_ensemble_pd_model_mag_sun_filtered(solver, b, uc.cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED, want_trajectories=traj,
                                                              want_estimates=est, **STAT, **_wrap(pkg, kw))
    return call


@pytest.fixture(scope="module")
def run_parent(pkg, solver):
    """tsat_*_model_mag_filtered of the same run, on this family's keyword arguments less the sun's"""
    tr = pkg.tracking

    def call(law, e, M, kw):
        if law == "tv":
            return tr.attitude_ensemble_model_mag_filtered(solver, e["b"], e["X"], e["U"], uc.cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True,
                                                           want_trajectories=True, want_estimates=True, **STAT, **_wrap_parent(pkg, kw))
        return tr.attitude_ensemble_pd_model_mag_filtered(solver, e["b"], uc.cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED, want_trajectories=True,
                                                          want_estimates=True, **STAT, **_wrap_parent(pkg, kw))
    return call


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_tvlqr_matches_reference(pkg, ol, run, ens, M, limits, latency):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront"""
    kw = uc.tv_kw(ens, M, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref, got, keep = uc.parity(pkg, ol, run, ens, M, "tv", kw)
    ec.same_gains(ens["K"], got["K"])
    if limits == "0.6":
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", uc.KINDS)
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_pd_matches_reference(pkg, ol, run, ens, M, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation saturates every
    component under the +-0.6 clip: it is compared under +-0.6 and under +-25, and asserts its conditions there"""
    kw = uc.pd_kw(ens, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = uc.parity(pkg, ol, run, ens, M, "pd", kw, skip=None)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    uc.parity(pkg, ol, run, ens, M, "pd", kw)


@pytest.mark.parametrize("law", ["tv", "pd"])
def test_gpu_delayed_sun_sample_is_paired_with_its_own_row(pkg, ol, run, ens, law):
    """latency 1 on ``pairing_table`` (sun rows alternately lit and dark), M = 64: pairing the delayed sample with s_k in the place
    of s_{k-1} moves the final state of the reference; then parity"""
    b, S = ens["b"], uc.pairing_table(ens["b"])
    kw = uc.tv_kw(ens, 64, latency=1, Stab=S) if law == "tv" else uc.pd_kw(ens, "track_ff", 0, 64, latency=1, Stab=S)
    pairs = dc.sampled_pairs(b.T, 64)
    ref = uc.ref_of(pkg, ol, ens, 64, law, pairs, kw)
    keep = gc.kept(ref, ens["o"])
    cp = mc.cond_pairs(ens, ref, pairs, keep)
    d = uc.moved(uc.ref_of(pkg, ol, ens, 64, law, cp, kw), uc.ref_of(pkg, ol, ens, 64, law, cp, dict(kw, sun_own_row=False)))
    print(f"  condition: {uc.SUN_PAIRING}: max|d final state| {d:.2e}")
    assert d >= gc.MOVED
    got = run(law, ens, 64, kw)
    dc.compare(ref, got, pairs, keep)
    uc.compare_estimates(ref, got, pairs, keep)


def test_gpu_tiny_horizons_at_latency_1(pkg, ol, run, ens):
    """n_knots = 2, 3 and 4 among the slews at latency 1, M = 64 (model_mag_sun_filtered_common.check_tiny): filt_final is
    ``first_record`` with 2 and 3 knots; with 4 the first sun update is made at k = 2"""
    b = mc.tiny_batch(ens["b"])
    e = dict(ens, K=ol.tvlqr_batch(b, ens["X"], ens["U"], *ens["W"], ens["X"][:, 0])["K"])      # the gains of the shortened horizons
    uc.check_tiny(pkg, ol, run, e, 64, b)


def _same(a, c, keys=EST):
    for k in keys:
        if a[k].dtype.kind == "f":
            d = float(np.max(np.abs(a[k] - c[k])))
            assert d == 0.0, (k, d)
        assert a[k].tobytes() == c[k].tobytes(), k


@pytest.mark.parametrize("latency", [0, 1])
def test_gpu_dark_table_and_null_table_are_the_parent_of_the_same_run(pkg, run, run_parent, ens, latency):
    """a table dark throughout, and Stab = NULL, against tsat_*_model_mag_filtered of the same run: max |d| = 0 on X_sim, X_hat and
    filt_final, equal stats, summary, nominal statistics and n_clipped; a lit table differs. Both laws, with and without gravity rows"""
    M, zero = 64, np.zeros_like(ens["Stab"])
    for rt, gm in ((ens["Rtab"], gc.GM), (None, 0.0)):
        for law, kw in (("tv", uc.tv_kw(ens, M, latency=latency, Rtab=rt, gm=gm)),
                        ("pd", uc.pd_kw(ens, "track_ff", 0, M, latency=latency, Rtab=rt, gm=gm)),
                        ("pd", uc.pd_kw(ens, "regulate", 1, M, latency=latency, Rtab=rt, gm=gm))):
            old = run_parent(law, ens, M, kw)
            _same(old, run(law, ens, M, dict(kw, Stab=zero)))
            _same(old, run(law, ens, M, dict(kw, Stab=None, sigma_sun=0.0)))
            d = float(np.max(np.abs(old["X_hat"] - run(law, ens, M, kw)["X_hat"])))
            print(f"{law} latency {latency}: a dark table and no table are the parent (max|d| 0); the case's table moves X_hat by {d:.2e}")
            assert d >= gc.MOVED


def test_gpu_null_filter_is_the_sensed_call(pkg, solver, run, ens):
    """f = NULL is the sensed entry point byte for byte; twice the same call gives the same bytes (``load`` zeroes the record and
    the sample memory); X_hat / filt_final requested or not does not change the run"""
    e, b, M = ens, ens["b"], 64
    lib, abi = pkg._abi.load(), pkg._abi
    x0 = np.ascontiguousarray(e["x0s"][:, :M])
    for latency in (0, 1):
        tvkw, pdkw = uc.tv_kw(e, M, latency=latency), uc.pd_kw(e, "track_ff", 1, M, latency=latency)
        off = dict(filt=None, Stab=None, sigma_sun=0.0)
        strip = lambda kw: {k: v for k, v in kw.items() if k not in ("filt", "Stab", "sigma_sun")}
        for fn_f, fn_s, new, old in (
                (lib.tsat_tvlqr_ensemble_model_mag_sun_filtered, lib.tsat_tvlqr_ensemble_sensed,
                 uc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], x0, **dict(tvkw, **off)),
                 sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], x0, **strip(tvkw))),
                (lib.tsat_pd_ensemble_model_mag_sun_filtered, lib.tsat_pd_ensemble_sensed,
                 uc.PdCall(abi, b, e["o"], x0, sc.KD, sc.KP, **dict(pdkw, **off)),
                 sc.PdCall(abi, b, e["o"], x0, sc.KD, sc.KP, **strip(pdkw)))):
            assert fn_f(solver._h, *new.c_args()) == 0 and fn_s(solver._h, *old.c_args()) == 0
            _same(new.result(), old.result(), OUT)
        for law, kw in (("tv", tvkw), ("pd", pdkw)):
            a = run(law, e, M, kw)
            _same(a, run(law, e, M, kw))
            c = run(law, e, M, kw, est=False)
            _same(a, c, OUT)
            assert c["X_hat"] is None and a["filt_final"].tobytes() == c["filt_final"].tobytes()


def _emu_run(emu, law, e, M, kw):
    if law == "tv":
        return emu.tv(e["b"], e["o"], e["X"], e["U"], *e["W"], uc.cut(e["x0s"], M), e["K"], **kw)
    return emu.pd(e["b"], e["o"], uc.cut(e["x0s"], M), sc.KD, sc.KP, **kw)


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("combo", ["tv-0.6", "tv-25", "track-0", "track-1", "track_ff-0", "track_ff-1", "regulate-0", "regulate-1"])
def test_gpu_library_against_emulated_kernels_two_wavefronts(pkg, run, ens, combo, latency):
    """M = 70: lanes 0 .. 5 of a second wavefront and the model slot in it. Every realisation of every slew, the library against the
    emulated kernels: X_sim, X_hat and filt_final to the 1e-9 of the tier (the maximum is printed), the nominal statistics equal. The
    emulated TVLQR kernel is given the library's own gains"""
    M = 70
    a, c = combo.split("-")
    if a == "tv":
        law, kw = "tv", uc.tv_kw(ens, M, sat=hc.SAT if c == "0.6" else pc.WIDE, latency=latency)
    else:
        law, kw = "pd", uc.pd_kw(ens, a, int(c), M, latency=latency)
    got = run(law, ens, M, kw)
    emu = _emu_run(uc.EmuModelMagSunFiltered(pkg._abi), law, dict(ens, K=got["K"]) if law == "tv" else ens, M, kw)
    d = {k: float(np.max(np.abs(got[k] - emu[k]))) for k in ("X_sim", "X_hat", "filt_final")}
    print(f"{combo} latency {latency}, M = 70, library against emulator: " + "  ".join(f"max|d{k}| {v:.2e}" for k, v in d.items()))
    assert max(d.values()) < 1e-9
    assert np.isfinite(got["X_hat"]).all() and np.isfinite(got["filt_final"]).all()
    ec.same_stats(emu["nominal"], got["nominal"])
    agree = np.count_nonzero(got["stats"]["failed"] == emu["stats"]["failed"])
    assert agree >= got["stats"].size - (dc.N_DRAWN - dc.N_KEPT), "more realisations than the cap disagree on the statistic"


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every rejection returns -1 with its text and leaves the handle's workspaces empty; a good call grows them by what its parent's
    call grows them by plus the packed sun rows, which are part of the handle's accounting; Stab = NULL grows the parent's only"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    abi = pkg._abi
    x0 = np.ascontiguousarray(e["x0s"][:, :M])
    pd = uc.PdCall(abi, b, e["o"], x0, sc.KD, sc.KP, **uc.pd_kw(e, "track_ff", 0, M))
    tv = uc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], x0, **uc.tv_kw(e, M))
    pd_fn, tv_fn = lib.tsat_pd_ensemble_model_mag_sun_filtered, lib.tsat_tvlqr_ensemble_model_mag_sun_filtered
    _trim(pkg, solver)
    null_f = [("f NULL with X_hat", lambda c: c.edit(f=None, Stab=None, sigma_sun=0.0), "X_hat and filt_final must be NULL"),
              ("f NULL with filt_final", lambda c: c.edit(f=None, Stab=None, sigma_sun=0.0, X_hat=None), "X_hat and filt_final must be NULL")]
    tv_parent = [("Rtab NULL, gm != 0", tv.edit(Rtab=None), "Rtab is NULL but gm != 0"),
                 ("one limit NULL", tv.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"), ("X NULL", tv.edit(X=None), "null array")]
    for fn, call, cases in ((pd_fn, pd, uc.filter_rejections(pd) + sc.sensor_rejections(pd) + pc.rejections(pd, b, e["Rtab"])),
                            (tv_fn, tv, uc.filter_rejections(tv) + sc.sensor_rejections(tv) + tv_parent)):
        for label, bad, words in cases + [(l, ed(call), w) for l, ed, w in null_f]:
            rc = fn(solver._h, *bad.c_args())
            msg = lib.tsat_ensemble_last_error().decode()
            assert rc == -1 and words in msg, (label, rc, msg)
            assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    rows = e["Stab"].shape[0] * e["Stab"].shape[1]
    par_tv = mc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], x0, **uc.parent_kw(uc.tv_kw(e, M)))
    par_pd = mc.PdCall(abi, b, e["o"], x0, sc.KD, sc.KP, **uc.parent_kw(uc.pd_kw(e, "track_ff", 0, M)))
    for fn, call, par_fn, par in ((tv_fn, tv, lib.tsat_tvlqr_ensemble_model_mag_filtered, par_tv),
                                  (pd_fn, pd, lib.tsat_pd_ensemble_model_mag_filtered, par_pd)):
        assert par_fn(solver._h, *par.c_args()) == 0
        parent = _ws(pkg, solver)
        _trim(pkg, solver)
        assert fn(solver._h, *call.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
        grown = _ws(pkg, solver)
        assert grown == parent + 32 * rows, (grown, parent)                      # the packed sun rows: four doubles a row
        assert fn(solver._h, *call.edit(sigma_sun=-1.0).c_args()) == -1 and _ws(pkg, solver) == grown      # a rejection leaves the size
        _trim(pkg, solver)
        assert fn(solver._h, *call.edit(Stab=None, sigma_sun=0.0).c_args()) == 0 and _ws(pkg, solver) == parent
        _trim(pkg, solver)
    assert tv_fn(solver._h, *tv.edit(plant=None, Rtab=None, gm=0.0).c_args()) == 0
    _trim(pkg, solver)


def test_gpu_filter_on_a_long_horizon(pkg, ol, solver):
    """T = 1, N = 400, M = 8 (model_mag_sun_filtered_common.long_case), a sun direction 35.2 deg from the nearest field row. On the
    references alone, rms over the last half (measured: attitude error lit throughout 0.26 deg mean, 0.16 .. 0.38, against the
    model-mag filter's 2.77 deg mean, 1.56 .. 4.19, on the same draws; dark from knot 100 on 0.66 deg mean, 0.21 .. 1.58; rate error
    1.9e-4 rad/s lit and 3.4e-4 half dark against the raw sample's 1.17e-2, under the parent's bar of 0.25 x it); then the kernels
    against both references to 1e-9 on X_sim, X_hat and filt_final"""
    c = uc.long_case(pkg, ol, N=400, M=8)
    assert len(c["pairs"]) == 8
    uc.assert_sun_helps(c)
    for name, kw in (("ref", c["kw"]), ("half", c["kw_half"])):
        got = pkg.tracking.attitude_ensemble_pd_model_mag_sun_filtered(solver, c["b"], c["x0s"], sc.KD, sc.KP, ec.SEED,
                                                                       want_trajectories=True, want_estimates=True, **STAT, **_wrap(pkg, kw))
        dc.compare(c[name], got, c["pairs"])
        uc.compare_estimates(c[name], got, c["pairs"])
