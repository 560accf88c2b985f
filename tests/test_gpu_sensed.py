"""GPU tier of the ensemble controllers fed measurements (tsat_tvlqr_ensemble_sensed, tsat_pd_ensemble_sensed through
``tracking.attitude_ensemble_sensed`` / ``attitude_ensemble_pd_sensed``) against the references of tests/sensed_common.py, on the
smallest shapes at which the kernels can go wrong. The bars are the parents' (dispersed_common.compare). Every parity test first
asserts its conditions on references alone (sensed_common.conditions, bar 1e-7), over the first N_COND compared pairs.

The case is ``pd_common.case`` — 8 slews, N = 20, horizons (20, 13, 6, 7, 20, 19, 6, 20), the 3U model inertia, two dipole tables
with their orbits behind btab_idx = (0, 1, 1, 0, 1, 0, 0, 1), all five plant dispersions, plant noise on, gravity gradient on, the
statistic thresholds of mpc_held_common — with the TVLQR weights r = 0.5e-6, the PD gains 10 x pd_common's and the sensor levels
sensed_common.SIGMAS / BIAS. The plan is solved once per module at the 1 x 3 budget; the gains of the references are the
oracle's."""
import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
KINDS = ("track", "track_ff", "regulate")
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")
N_COND = 8          # compared pairs the conditions are evaluated on: shown on a part of them, they hold on all


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
    """the keyword arguments that both the reference and the wrapper take (``sens`` is spread into the wrapper's sigma_*)"""
    kw = dict(Rtab=e["Rtab"], gm=gc.GM, plant=_cut(e["plant"], M), sat=sat, sens=sc.SIGMAS, latency=0, sensor=_cut(e["sensor"], M))
    kw.update(over)
    return kw


def _pd_kw(e, kind, mode, M, **over):
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"], gm=gc.GM,
              plant=_cut(e["plant"], M), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"], sens=sc.SIGMAS, latency=0, sensor=_cut(e["sensor"], M))
    kw.update(over)
    return kw


def _wrap(kw):
    kw = dict(kw)
    kw.update(kw.pop("sens"))
    return kw


def _tv_run(pkg, solver, e, M, kw, batch=None, traj=True):
    return pkg.tracking.attitude_ensemble_sensed(solver, batch or e["b"], e["X"], e["U"], _cut(e["x0s"], M), *e["W"], ec.SEED, want_K=True,
                                                 want_trajectories=traj, **STAT, **_wrap(kw))


def _pd_run(pkg, solver, e, M, kw, batch=None, traj=True):
    return pkg.tracking.attitude_ensemble_pd_sensed(solver, batch or e["b"], _cut(e["x0s"], M), sc.KD, sc.KP, ec.SEED,
                                                    want_trajectories=traj, **STAT, **_wrap(kw))


def _tv_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return sc.pairs_of(ol, pkg._abi, "tv", batch or e["b"], e["x0s"][:, :M], e["K"], e["o"], pairs, X=e["X"], U=e["U"], **kw)


def _pd_ref(pkg, ol, e, M, pairs, kw, batch=None):
    return sc.pairs_of(ol, pkg._abi, "pd", batch or e["b"], e["x0s"][:, :M], (sc.KD, sc.KP), e["o"], pairs, **kw)


def _parity(pkg, ol, solver, e, M, law, kw, with_conditions=True):
    """34 seeded (t, m) drawn, the first 32 off the thresholds compared (at most 2 replaced); summary, zero fill and stats_nominal
    with them. The conditions are asserted on references alone, over the first N_COND compared pairs"""
    b = e["b"]
    ref_of, run = (_tv_ref, _tv_run) if law == "tv" else (_pd_ref, _pd_run)
    pairs = dc.sampled_pairs(b.T, M)
    ref = ref_of(pkg, ol, e, M, pairs, kw)
    keep = gc.kept(ref, e["o"])
    if with_conditions:
        cp = pairs[keep[:N_COND]]
        sc.conditions(lambda **o: ref_of(pkg, ol, e, M, cp, dict(kw, **o)), law, kw["sensor"])
    got = run(pkg, solver, e, M, kw)
    dc.compare(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom = ref_of(pkg, ol, e, M, np.array([(t, -1) for t in range(b.T)]), kw)
    ec.same_stats(nom["stats"], got["nominal"])
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
    component under the +-0.6 clip, where no sensor error reaches the plant: it is compared under +-0.6 and under +-25, and
    asserts its conditions there (as tests/test_sensed.py)"""
    kw = _pd_kw(ens, kind, mode, M, latency=latency)
    if kind == "regulate":
        ref, _, keep = _parity(pkg, ol, solver, ens, M, "pd", kw, with_conditions=False)
        assert ref["n_sure"][keep].max() > 0, "no knot of the case clips"
        kw = dict(kw, sat=pc.WIDE)
    _parity(pkg, ol, solver, ens, M, "pd", kw)


def test_gpu_tiny_horizons_at_latency_1(pkg, ol, solver, ens):
    """n_knots = 2 (one command, from y_0) and 3 (two commands, both from y_0) among the slews, latency 1, M = 64"""
    import dataclasses
    e, M = ens, 64
    nk = e["b"].n_knots.copy()
    nk[[0, 5]], nk[[1, 7]] = 2, 3
    b = dataclasses.replace(e["b"], n_knots=nk)
    e = dict(e, K=ol.tvlqr_batch(b, e["X"], e["U"], *e["W"], e["X"][:, 0])["K"])      # the gains of the shortened horizons
    pairs = dc.sampled_pairs(b.T, M)
    nomp = np.array([(t, -1) for t in range(b.T)])
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
        keep = big[ok]
        dc.compare(ref, got, pairs, np.concatenate([tiny, keep]))
        assert np.all(got["stats"]["failed"][t, m] == 1)
        ec.same_stats(ref_of(pkg, ol, e, M, nomp, kw, batch=b)["stats"], got["nominal"])
        for s, n in enumerate(nk):
            assert np.all(got["X_sim"][s, :, n:] == 0)


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
        for k in ("stats", "X_sim", "n_clipped"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


def _close_to_parent(old, new, label):
    """the ideal sensor against the parent ENTRY POINT: two differently compiled kernels computing the same expressions. The bar is
    the one at which the project pins one computation restated in other code (1e-12); bit equality is expected, the measured maximum
    is printed"""
    d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
    print(f"{label}: ideal sensor against the parent entry point, max|dX_sim| {d:.2e}, bytes equal: {old['X_sim'].tobytes() == new['X_sim'].tobytes()}")
    assert d <= 1e-12
    for k in ("stats", "nominal", "n_clipped", "summary"):
        assert np.array_equal(old[k], new[k]), (label, k)


def test_gpu_ideal_sensor_against_the_parent_entry_points(pkg, solver, ens):
    e, b, M = ens, ens["b"], 64
    tr = pkg.tracking
    zero = np.zeros_like(e["sensor"])
    ideal = dict(sens=sc.IDEAL, latency=0, sensor=zero)
    x0s, plant = _cut(e["x0s"], M), _cut(e["plant"], M)
    common = dict(sat=hc.SAT, want_K=True, want_trajectories=True, **STAT)
    gg = tr.attitude_ensemble_gg(solver, b, e["X"], e["U"], x0s, *e["W"], ec.SEED, plant, e["Rtab"], gc.GM, **common)
    new = _tv_run(pkg, solver, e, M, _tv_kw(e, M, **ideal))
    _close_to_parent(gg, new, "tsat_tvlqr_ensemble_gg")
    assert np.array_equal(gg["K"], new["K"])
    disp = tr.attitude_ensemble_dispersed(solver, b, e["X"], e["U"], x0s, *e["W"], ec.SEED, plant, **common)
    new0 = _tv_run(pkg, solver, e, M, _tv_kw(e, M, Rtab=None, gm=0.0, **ideal))
    _close_to_parent(disp, new0, "tsat_tvlqr_ensemble_dispersed")
    assert np.max(np.abs(new["X_sim"] - new0["X_sim"])) >= gc.MOVED
    for kind in KINDS:
        for mode in (0, 1):
            for rt in (e["Rtab"], None):
                kw = _pd_kw(e, kind, mode, M, Rtab=rt, gm=gc.GM if rt is not None else 0.0, **ideal)
                pkw = {k: v for k, v in kw.items() if k not in ("sens", "latency", "sensor")}
                old = tr.attitude_ensemble_pd(solver, b, x0s, sc.KD, sc.KP, ec.SEED, want_trajectories=True, **STAT, **pkw)
                _close_to_parent(old, _pd_run(pkg, solver, e, M, kw), f"tsat_pd_ensemble ({kind}, mode {mode}, Rtab {'given' if rt is not None else 'NULL'})")


def test_gpu_bit_equalities(pkg, solver, ens):
    """sensor = NULL against zeros, Rtab with gm = 0 against Rtab = NULL, plant = NULL against the model's plants: byte for byte,
    sensor noise on and latency 1"""
    e, b, M = ens, ens["b"], 64
    zero = np.zeros_like(e["sensor"])
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    tv = _tv_kw(e, M, gm=0.0, latency=1)
    a = _tv_run(pkg, solver, e, M, tv)
    _same_bytes(a, _tv_run(pkg, solver, e, M, dict(tv, Rtab=None)))
    assert np.max(np.abs(_tv_run(pkg, solver, e, M, dict(tv, gm=gc.GM))["X_sim"] - a["X_sim"])) >= gc.MOVED
    z = _tv_run(pkg, solver, e, M, dict(tv, sensor=zero))
    _same_bytes(z, _tv_run(pkg, solver, e, M, dict(tv, sensor=None)))
    assert np.max(np.abs(z["X_sim"] - a["X_sim"])) >= gc.MOVED
    _same_bytes(_tv_run(pkg, solver, e, M, dict(tv, plant=None)), _tv_run(pkg, solver, e, M, dict(tv, plant=model)))
    for kind in KINDS:
        pd = _pd_kw(e, kind, 1, M, gm=0.0, latency=1)
        a = _pd_run(pkg, solver, e, M, pd)
        _same_bytes(a, _pd_run(pkg, solver, e, M, dict(pd, Rtab=None)))
        z = _pd_run(pkg, solver, e, M, dict(pd, sensor=zero))
        _same_bytes(z, _pd_run(pkg, solver, e, M, dict(pd, sensor=None)))
        assert np.max(np.abs(z["X_sim"] - a["X_sim"])) >= gc.MOVED


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every rejection returns -1 with its text and leaves the handle's workspaces empty; a good call grows them by exactly what its
    parent's call grows them by"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    abi = pkg._abi
    pd = sc.PdCall(abi, b, e["o"], e["x0s"][:, :M], sc.KD, sc.KP, **_pd_kw(e, "track_ff", 0, M))
    tv = sc.TvCall(abi, b, e["o"], e["X"], e["U"], *e["W"], e["x0s"][:, :M], **_tv_kw(e, M))
    _trim(pkg, solver)
    bad_plant = tv.v["plant"].copy()
    bad_plant[1, 2, 20] = np.nan
    tv_parent = [("plant NaN", tv.edit(plant=bad_plant), "non-finite plant entry at (t, m) = (1, 2)"),
                 ("Rtab NULL, gm != 0", tv.edit(Rtab=None), "Rtab is NULL but gm != 0"),
                 ("one limit NULL", tv.edit(sat_hi=None), "exactly one of sat_lo / sat_hi is NULL"),
                 ("noise_mode 0", tv.edit(o=(lambda o: (setattr(o, "noise_mode", 0), o)[1])(abi.TvlqrOptions.from_buffer_copy(tv.v["o"]))),
                  "noise_mode must be 1"), ("X NULL", tv.edit(X=None), "null array")]
    for fn, cases in ((lib.tsat_pd_ensemble_sensed, sc.sensor_rejections(pd) + pc.rejections(pd, b, e["Rtab"])),
                      (lib.tsat_tvlqr_ensemble_sensed, sc.sensor_rejections(tv) + tv_parent)):
        for label, call, words in cases:
            rc = fn(solver._h, *call.c_args())
            msg = lib.tsat_ensemble_last_error().decode()
            assert rc == -1 and words in msg, (label, rc, msg)
            assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    # good calls: the parent's bytes, nothing more
    tr = pkg.tracking
    x0s, plant = _cut(e["x0s"], M), _cut(e["plant"], M)
    tr.attitude_ensemble_gg(solver, b, e["X"], e["U"], x0s, *e["W"], ec.SEED, plant, e["Rtab"], gc.GM, sat=hc.SAT, **STAT)
    parent = _ws(pkg, solver)
    _trim(pkg, solver)
    assert lib.tsat_tvlqr_ensemble_sensed(solver._h, *tv.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == parent and parent >= 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]
    _trim(pkg, solver)
    assert lib.tsat_pd_ensemble_sensed(solver._h, *pd.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, as tsat_pd_ensemble
    # allowed here, rejected by the parent: the NULL plant, the NULL Rtab with gm = 0
    assert lib.tsat_tvlqr_ensemble_sensed(solver._h, *tv.edit(plant=None, Rtab=None, gm=0.0).c_args()) == 0
    _trim(pkg, solver)


def test_gpu_long_horizon_regulation(pkg, ol, solver):
    """T = 2, M = 64, N = 20 000 knots, PD regulation with X = NULL, sensors on, latency 1: the generator's 32-bit knot counter and
    the table clock far past the small case. Two runs give byte-identical statistics, everything is finite, and two RK4 steps at
    k = 10 000 re-integrated with numpy from X_sim of two pairs — the command recomputed from the definition, the first one from the
    measurement of knot 9 999 — match to 1e-9"""
    N, M, k0 = 20000, 64, 10000
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=2, N=N))
    b.dtau[:] = 0.01
    Rtab = gc.orbit(pkg, b.n_tab, 0.2)[None]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    plant = dc.all_five_plants(pkg, b, M)
    sensor = sc.biases(pkg, b.T, M)
    o = pc.options(ol)
    kw = dict(Rtab=Rtab, gm=gc.GM, plant=plant, sat=hc.SAT, limit_mode=1, x0_nom=np.ascontiguousarray(b.x0), sensor=sensor, latency=1,
              **sc.SIGMAS)
    run = lambda traj: pkg.tracking.attitude_ensemble_pd_sensed(solver, b, x0s, sc.KD, sc.KP, ec.SEED, want_trajectories=traj, **STAT, **kw)
    a, c = run(True), run(False)
    _same_bytes(a, c, ("stats", "summary", "nominal", "n_clipped"))
    for f in ("slew_time", "final_w_norm", "final_angle"):
        assert np.all(np.isfinite(a["stats"][f])) and np.all(np.isfinite(a["nominal"][f]))
    assert np.all(np.isfinite(a["X_sim"]))
    ol.load()
    for t, m in ((0, 5), (1, 63)):
        args = (ol, "pd", b, t, None, None, (sc.KD, sc.KP), a["X_sim"][t, m, k0], o, t * M + m, Rtab, gc.GM, plant[t, m], hc.SAT[0], hc.SAT[1])
        kws = dict(limit_mode=1, sens=sc.SIGMAS, latency=1, bias=sensor[t, m], k_start=k0, k_stop=k0 + 2, x_before=a["X_sim"][t, m, k0 - 1])
        Xs, _, Uc = sc.loop(*args, **kws)
        d = float(np.max(np.abs(Xs[k0 + 1:k0 + 3] - a["X_sim"][t, m, k0 + 1:k0 + 3])))
        print(f"(t, m) = ({t}, {m}): two steps from k = {k0} re-integrated, max|d| {d:.2e}")
        assert d < 1e-9
        # the condition: a loop that took y_k for the command of knot k would differ at these two knots
        Uc0 = sc.loop(*args, **dict(kws, latency=0))[2]
        assert np.max(np.abs(Uc[k0:k0 + 2] - Uc0[k0:k0 + 2])) >= gc.MOVED
