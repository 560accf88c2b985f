"""GPU tier of the projection PD baseline (tsat_pd_ensemble through ``tracking.attitude_ensemble_pd``) against the reference of
tests/pd_common.py, on the smallest shapes at which the kernels can go wrong. The bars are the parents' (dispersed_common.compare).
Every parity test first asserts its conditions on references alone (pd_common.differs, bar 1e-7; pd_common.limit_condition).

The case is the fixture of tests/test_gpu_gg.py — 8 slews, N = 20, horizons (20, 13, 6, 7, 20, 19, 6, 20), the 3U model inertia, two
dipole tables with their orbits behind btab_idx = (0, 1, 1, 0, 1, 0, 0, 1), 16 rows under a clock that runs to row 17.3, all five
dispersions, noise on, limits +-0.6, the statistic thresholds of mpc_held_common — with the gains kd = (2e-5, 3e-5, 1e-5),
kp = (4e-7, 2e-7, 6e-7) for every slew. Regulating from the plan's start, slews 0, 1, 3 have e0 < 0 at every knot (the sign rule
decides the attitude term), slews 0, 2, 3, 4, 6 clip at every knot and 1, 5, 7 never do."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
KINDS = ("track", "track_ff", "regulate")
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
    """the plan (solved here, 1 x 3 budget), 64 realisations and their plants; computed once and left unchanged"""
    to = pkg.trajopt
    b, Rtab = pc.case(pkg)
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    r = to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 64, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 64),
                x0n=np.ascontiguousarray(b.x0))


def _kw(e, kind, mode, M, **over):
    """the keyword arguments that both the reference and the wrapper take"""
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"], gm=gc.GM,
              plant=np.ascontiguousarray(e["plant"][:, :M]), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"])
    kw.update(over)
    return kw


def _run(pkg, solver, e, M, kw, batch=None, traj=True):
    return pkg.tracking.attitude_ensemble_pd(solver, batch or e["b"], np.ascontiguousarray(e["x0s"][:, :M]), pc.KD, pc.KP, ec.SEED,
                                             want_trajectories=traj, **STAT, **kw)


def _ref(pkg, ol, e, M, pairs, kw, kd=pc.KD, kp=pc.KP, batch=None, **extra):
    return pc.reference_pairs(ol, pkg._abi, batch or e["b"], e["x0s"][:, :M], kd, kp, e["o"], pairs, **kw, **extra)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [63, 64])
def test_gpu_kernel_matches_reference(pkg, ol, solver, ens, M, kind, mode):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront. 34 seeded (t, m) drawn, the
    first 32 off the thresholds compared (at most 2 replaced); summary, zero fill and stats_nominal with them"""
    e, b = ens, ens["b"]
    pairs = dc.sampled_pairs(b.T, M)
    kw = _kw(e, kind, mode, M)
    ref = _ref(pkg, ol, e, M, pairs, kw)
    keep = gc.kept(ref, e["o"])
    sub = lambda r: dict(X_sim=r["X_sim"][keep], n_knots=r["n_knots"][keep])
    # the conditions, on references alone, over the compared pairs
    pc.differs(sub(ref), sub(_ref(pkg, ol, e, M, pairs, kw, kd=np.zeros(3), kp=np.zeros(3))), "law on against law off")
    pc.differs(sub(ref), sub(_ref(pkg, ol, e, M, pairs, dict(kw, gm=0.0))), "gm on against gm = 0")
    pc.differs(sub(ref), sub(_ref(pkg, ol, e, M, pairs, dict(kw, Rtab=e["Rtab"][::-1]))), "orbit tables swapped")
    if kind == "regulate":
        pc.differs(sub(ref), sub(_ref(pkg, ol, e, M, pairs, kw, sign_rule=False)), "sign rule on against s = +1")
    if kind == "track_ff":
        pc.differs(sub(ref), sub(_ref(pkg, ol, e, M, pairs, dict(kw, U=None))), "feed-forward on against off")
    kref = {k: (v[keep] if isinstance(v, np.ndarray) else [v[i] for i in keep]) for k, v in ref.items()}
    pc.limit_condition(kref, lambda: {k: v[keep] for k, v in _ref(pkg, ol, e, M, pairs, dict(kw, limit_mode=0)).items() if k in ("X_sim", "n_knots")},
                       kind, mode)
    got = _run(pkg, solver, e, M, kw)
    dc.compare(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom = _ref(pkg, ol, e, M, np.array([(t, -1) for t in range(b.T)]), kw)
    ec.same_stats(nom["stats"], got["nominal"])


def _same_bytes(a, c, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_gpu_bit_equalities(pkg, solver, ens):
    e, b, M = ens, ens["b"], 64
    run = lambda kw: _run(pkg, solver, e, M, kw)
    # Rtab given with gm = 0 against Rtab = NULL: the kernel with the gravity rows against the one without
    kw = _kw(e, "track_ff", 0, M, gm=0.0)
    off = run(kw)
    _same_bytes(off, run(dict(kw, Rtab=None)))
    assert np.max(np.abs(run(dict(kw, gm=gc.GM))["X_sim"] - off["X_sim"])) >= gc.MOVED
    # plant = NULL against plants filled with (Jmat, I, 0)
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    for kind in KINDS:
        kw = _kw(e, kind, 1, M)
        none = run(dict(kw, plant=None))
        _same_bytes(none, run(dict(kw, plant=model)))
    assert np.max(np.abs(none["X_sim"] - run(kw)["X_sim"])) >= gc.MOVED
    # X = xf tiled against X = NULL, the same explicit x0_nom
    tiled = np.ascontiguousarray(np.broadcast_to(b.xf[:, None, :], (b.T, b.N, 7)))
    for mode in (0, 1):
        kw = _kw(e, "regulate", mode, M)
        _same_bytes(run(kw), run(dict(kw, X=tiled)))
    # mode 1 against mode 0 under limits nothing reaches
    for kind in KINDS:
        kw = _kw(e, kind, 0, M, sat=pc.WIDE)
        a = run(kw)
        assert not a["n_clipped"].any()
        _same_bytes(a, run(dict(kw, limit_mode=1)))


def test_gpu_realisations_do_not_depend_on_m(pkg, solver, ens):
    """with explicit generator ids, realisations 0 .. 62 of the M = 64 run are the M = 63 run, byte for byte"""
    id0 = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
    for kind, mode in (("regulate", 1), ("track_ff", 0)):
        a = _run(pkg, solver, ens, 63, _kw(ens, kind, mode, 63, noise_id0=id0))
        c = _run(pkg, solver, ens, 64, _kw(ens, kind, mode, 64, noise_id0=id0))
        for k in ("stats", "X_sim", "n_clipped"):
            assert a[k].tobytes() == np.ascontiguousarray(c[k][:, :63]).tobytes(), k
        assert a["nominal"].tobytes() == c["nominal"].tobytes()


def test_gpu_zero_field_row(pkg, ol, solver, ens):
    """Btab[:, 15, :] = 0: the last knots of the 20- and 19-knot horizons sit on it; every output is finite and matches the reference,
    whose command at those knots is the feed-forward alone"""
    e, M = ens, 64
    B = e["b"].Btab.copy()
    B[:, 15, :] = 0.0
    b = dataclasses.replace(e["b"], Btab=np.ascontiguousarray(B))
    pairs = dc.sampled_pairs(b.T, M)
    for kind, mode in (("track_ff", 0), ("regulate", 1)):
        kw = _kw(e, kind, mode, M)
        ref = _ref(pkg, ol, e, M, pairs, kw, batch=b)
        on_zero = [k for k in range(b.N - 1) if not dc._row(b, 0, k, 0.0).any()]
        assert len(on_zero) >= 2
        seen = 0
        for i, p in enumerate(pairs):
            if b.n_knots[p[0]] == b.N:
                want = e["U"][p[0]][on_zero] if kind == "track_ff" else np.zeros((len(on_zero), 3))
                assert np.array_equal(ref["U_cmd"][i, on_zero], want)
                seen += 1
        assert seen > 0
        keep = gc.kept(ref, e["o"])
        got = _run(pkg, solver, e, M, kw, batch=b)
        assert np.all(np.isfinite(got["X_sim"])) and np.all(np.isfinite(got["summary"]))
        for f in ("slew_time", "final_w_norm", "final_angle"):
            assert np.all(np.isfinite(got["stats"][f])) and np.all(np.isfinite(got["nominal"][f]))
        dc.compare(ref, got, pairs, keep)


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every listed error returns -1 with its text and leaves the handle's workspaces empty; a good regulating call without an orbit
    table grows them by nothing that scales with N (N = 20 against N = 2000), and tsat_workspace_trim(h, 1) returns what there is"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    kw = _kw(e, "track_ff", 0, M)
    good = pc.Call(pkg._abi, b, e["o"], e["x0s"][:, :M], pc.KD, pc.KP, **kw)
    _trim(pkg, solver)
    for label, call, words in pc.rejections(good, b, e["Rtab"]):
        rc = lib.tsat_pd_ensemble(solver._h, *call.c_args())
        msg = lib.tsat_ensemble_last_error().decode()
        assert rc == -1 and words in msg, (label, rc, msg)
        assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    sizes = []
    for N in (20, 2000):
        bn = hc.mpc_batch(pkg, T=2, N=N)
        x0s = pkg.tracking.ensemble_initial_states(bn.x0, M, np.random.default_rng(5))
        r = pkg.tracking.attitude_ensemble_pd(solver, bn, x0s, pc.KD, pc.KP, ec.SEED, sat=hc.SAT, limit_mode=1, **STAT)
        assert r["nominal"] is None and r["X_sim"] is None and np.all(np.isfinite(r["summary"]))
        sizes.append(_ws(pkg, solver))
    assert sizes[0] == sizes[1], sizes
    rc = lib.tsat_pd_ensemble(solver._h, *good.c_args())
    assert rc == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) - sizes[1] == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, the handle's
    _trim(pkg, solver)


def test_gpu_long_horizon_regulation(pkg, ol, solver):
    """T = 2, M = 64, N = 20 000 knots, X = NULL, a 200-row table under dtau = 0.01: the generator's 32-bit knot counter and the table
    clock far past the small case. Two runs give byte-identical statistics, everything is finite, and two RK4 steps at k = 10 000
    re-integrated with numpy from X_sim of two pairs match to 1e-9"""
    N, M, k0 = 20000, 64, 10000
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=2, N=N))
    b.dtau[:] = 0.01
    Rtab = gc.orbit(pkg, b.n_tab, 0.2)[None]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    plant = dc.all_five_plants(pkg, b, M)
    o = pc.options(ol)
    kw = dict(Rtab=Rtab, gm=gc.GM, plant=plant, sat=hc.SAT, limit_mode=1, x0_nom=np.ascontiguousarray(b.x0))
    run = lambda traj: pkg.tracking.attitude_ensemble_pd(solver, b, x0s, pc.KD, pc.KP, ec.SEED, want_trajectories=traj, **STAT, **kw)
    a, c = run(True), run(False)
    _same_bytes(a, c, ("stats", "summary", "nominal", "n_clipped"))
    for f in ("slew_time", "final_w_norm", "final_angle"):
        assert np.all(np.isfinite(a["stats"][f])) and np.all(np.isfinite(a["nominal"][f]))
    assert np.all(np.isfinite(a["X_sim"]))
    ol.load()
    for t, m in ((0, 5), (1, 63)):
        Xs = pc.reference_loop(ol, b, t, None, None, pc.KD, pc.KP, a["X_sim"][t, m, k0], o, t * M + m, Rtab, gc.GM, plant[t, m],
                               hc.SAT[0], hc.SAT[1], limit_mode=1, k_start=k0, k_stop=k0 + 2)[0]
        d = float(np.max(np.abs(Xs[k0 + 1:k0 + 3] - a["X_sim"][t, m, k0 + 1:k0 + 3])))
        print(f"(t, m) = ({t}, {m}): two steps from k = {k0} re-integrated, max|d| {d:.2e}")
        assert d < 1e-9
