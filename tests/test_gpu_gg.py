"""GPU tier of the gravity-gradient entry points (tsat_tvlqr_ensemble_gg through ``tracking.attitude_ensemble_gg``,
tsat_mpc_run_held_gg through ``mpc.receding_horizon_held_gg``) against the references of tests/gg_common.py, on the smallest shapes
at which the kernels can go wrong: 20 knots, 8 slews. The bars are those of the parents' tests (dispersed_common.compare,
mpc_dispersed_common.same). Every parity test first asserts on the references alone that the term moves the final state by at
least 1e-7 (gg_common.moved), so a kernel that ignores the orbit table cannot pass.

The ensemble case: horizons (20, 13, 6, 7, 20, 19, 6, 20), two field tables with the two orbits they were sampled on behind a
non-identity btab_idx, 16 rows under a clock that runs to row 17.3 (the last knots clamp to row 15), all five dispersions, noise
on, limits +-0.6. The hold cases: those of tests/test_gpu_mpc_held.py with the 3U model inertia."""
import ctypes as C
import math

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc

pytestmark = pytest.mark.gpu

N_STEPS = 12
KEYS = ("X_hist", "U_hist", "stats", "tracking_stats", "n_clipped")
STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
BIDX = np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=np.int32)
ORBITS = ((0.0, 0.0), (40.0, 70.0))            # RAAN, true anomaly (deg) of the two tables


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


# ---------------------------------------------------------------------------------------------------------------------------
# ensemble
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ens(pkg, ol, solver):
    """the plan (solved here, 1 x 3 budget), its gains from the oracle, 64 realisations; computed once and left unchanged"""
    ss, to = pkg.slew_setup, pkg.trajopt
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    n_tab = 16
    b.Btab = np.ascontiguousarray(np.stack([ss.dipole_btable(n_tab, 0.2, gc.A_KM, gc.INC, ra, nu) for ra, nu in ORBITS]))
    b.n_tab, b.btab_idx = n_tab, BIDX.copy()
    b.tau0[:], b.dtau[:] = 0.25, 0.9
    b.n_knots = hc.RAGGED.copy()
    Rtab = np.ascontiguousarray(np.stack([gc.orbit(pkg, n_tab, 0.2, ra, nu) for ra, nu in ORBITS]))
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    r = to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 64, np.random.default_rng(5))
    o = ec.tv_options(ol)
    o.min_steps, o.w_tol, o.angle_tol = hc.MIN_STEPS, hc.W_TOL, hc.ANGLE_TOL
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], w=(Qd, Qfd, Rd), K=K, x0s=x0s, o=o, plant=dc.all_five_plants(pkg, b, 64))


def _ens_run(pkg, solver, e, M, gm, fn=None, **kw):
    fn = fn or pkg.tracking.attitude_ensemble_gg
    extra = () if fn is pkg.tracking.attitude_ensemble_dispersed else (e["Rtab"], gm)
    return fn(solver, e["b"], e["X"], e["U"], np.ascontiguousarray(e["x0s"][:, :M]), *e["w"], ec.SEED,
              np.ascontiguousarray(e["plant"][:, :M]), *extra, sat=hc.SAT, want_K=True, want_trajectories=True, **STAT, **kw)


def _finals(r):
    return [r["X_sim"][i, n - 1] for i, n in enumerate(r["n_knots"])]


@pytest.mark.parametrize("M", [63, 64])
def test_gpu_ensemble_matches_reference(pkg, ol, solver, ens, M):
    """M = 63: M + 1 fills one wavefront exactly; M = 64: the model slot is alone in a second wavefront. 34 seeded (t, m) drawn, the
    first 32 off the thresholds compared (at most 2 replaced), stats_nominal with them"""
    e, b = ens, ens["b"]
    x0s, plant = e["x0s"][:, :M], e["plant"][:, :M]
    pairs = dc.sampled_pairs(b.T, M)
    args = (ol, pkg._abi, b, e["X"], e["U"], e["K"], x0s, e["o"], pairs)
    ref = gc.ensemble_pairs(*args, e["Rtab"], gc.GM, plant=plant, sat=hc.SAT)
    gc.moved(_finals(ref), _finals(dc.reference_pairs(*args, plant=plant, sat=hc.SAT)), f"ensemble M = {M}")
    # the two orbit tables are really two: the reference with them swapped is another trajectory
    gc.moved(_finals(ref), _finals(gc.ensemble_pairs(*args, e["Rtab"][::-1], gc.GM, plant=plant, sat=hc.SAT)), "orbit tables swapped")
    rows = [math.floor(0.25 + 0.9 * (k + c)) for k in range(19) for c in (0.0, 0.5, 1.0)]
    assert max(rows) > b.n_tab - 1, "the clock of the case must run past the last row"
    keep = gc.kept(ref, e["o"])
    got = _ens_run(pkg, solver, e, M, gc.GM)
    ec.same_gains(e["K"], got["K"])
    dc.compare(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom_pairs = np.array([(t, -1) for t in range(b.T)])
    nargs = (ol, pkg._abi, b, e["X"], e["U"], e["K"], x0s, e["o"], nom_pairs)
    nom = gc.ensemble_pairs(*nargs, e["Rtab"], gc.GM, sat=hc.SAT)
    gc.moved(_finals(nom), _finals(dc.reference_pairs(*nargs, sat=hc.SAT)), "noise-free model plant")
    ec.same_stats(nom["stats"], got["nominal"])


@pytest.mark.parametrize("M", [63, 64])
def test_gpu_ensemble_at_gm0_is_bit_equal_to_the_dispersed_entry_point(pkg, solver, ens, M):
    old = _ens_run(pkg, solver, ens, M, 0.0, fn=pkg.tracking.attitude_ensemble_dispersed)
    new = _ens_run(pkg, solver, ens, M, 0.0)
    for f in ("stats", "summary", "nominal", "K", "X_sim", "n_clipped"):
        assert old[f].tobytes() == new[f].tobytes(), f
    on = _ens_run(pkg, solver, ens, M, gc.GM)
    assert np.max(np.abs(on["X_sim"] - new["X_sim"])) >= gc.MOVED
    assert np.array_equal(on["K"], new["K"])                      # the gains do not see the term


def test_gpu_ensemble_rejections_and_workspace(pkg, solver, ens):
    """every listed error returns -1 with its text and launches nothing (the handle's workspaces stay empty); a good call grows them by
    the packed table, 32 bytes per row, and tsat_workspace_trim(h, 1) returns it"""
    e, b = ens, ens["b"]
    lib, abi = pkg._abi.load(), pkg._abi
    M = 5
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    plant, lo, hi = c(e["plant"][:, :M]), c(np.broadcast_to(hc.SAT[0], (8, 3))), c(np.broadcast_to(hc.SAT[1], (8, 3)))
    d = abi.as_dp

    def call(Rtab, gm, plant=plant):
        _, head, tail, out = pkg.tracking._ensemble_call(solver, b, e["X"], e["U"], c(e["x0s"][:, :M]), *e["w"], ec.SEED, None, 1.0, False,
                                                         False, True, 1e-2, hc.MIN_STEPS, hc.W_TOL, hc.ANGLE_TOL)
        ncl = np.zeros((8, M), dtype=np.int32)
        rc = lib.tsat_tvlqr_ensemble_gg(*head, d(plant), d(lo), d(hi), *tail, abi.as_ip(ncl), d(None if Rtab is None else c(Rtab)), gm)
        return rc, lib.tsat_ensemble_last_error()

    def edit(idx, v):
        r = e["Rtab"].copy()
        r[idx] = v
        return r

    _trim(pkg, solver)
    bad_plant = plant.copy(); bad_plant[2, 3, 20] = np.nan
    for Rtab, gm, kw, word in ((None, gc.GM, {}, b"null Rtab"), (edit((1, 4, 2), np.nan), gc.GM, {}, b"non-finite Rtab entry in row 20"),
                               (edit((0, 15, 0), np.inf), gc.GM, {}, b"non-finite Rtab entry in row 15"),
                               (edit((1, 0), 0.0), gc.GM, {}, b"row 16 has |r| = 0"), (e["Rtab"], -1.0, {}, b"gm must be finite"),
                               (e["Rtab"], np.nan, {}, b"gm must be finite"), (e["Rtab"], np.inf, {}, b"gm must be finite"),
                               (e["Rtab"], gc.GM, dict(plant=bad_plant), b"non-finite plant entry at (t, m) = (2, 3)")):   # the parent's
        rc, msg = call(Rtab, gm, **kw)
        assert rc == -1 and word in msg, (word, rc, msg)
        assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    _ens_run(pkg, solver, e, M, 0.0, fn=pkg.tracking.attitude_ensemble_dispersed)
    w1 = _ws(pkg, solver)
    rc, msg = call(e["Rtab"], 0.0)
    assert rc == 0 and msg == b""
    w2 = _ws(pkg, solver)
    assert w2 - w1 == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1], (w1, w2)
    rc, msg = call(e["Rtab"], gc.GM)
    assert rc == 0 and _ws(pkg, solver) == w2                     # grow-only: the second call allocates nothing
    _trim(pkg, solver)


# ---------------------------------------------------------------------------------------------------------------------------
# hold
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(pkg, ol):
    """the three cases of tests/test_gpu_mpc_held.py on the 3U inertia, and their references with and without the term, each
    computed once on demand and left unchanged"""
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    br = gc.use_3u(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    br.n_knots = hc.RAGGED.copy()
    Rtab = gc.orbit(pkg, b.n_tab, 0.2)[None]
    po = hc.noise_options(ol, **STAT)
    plant = hc.plants(pkg, b)
    setups = dict(saturated=(b, 0, hc.SAT, N_STEPS), wide=(b, 0, hc.WIDE, N_STEPS), ragged=(br, 1, hc.SAT, 8))
    refs = {}

    def ref(name, R, fb):
        if (name, R, fb) not in refs:
            bb, es, sat, n = setups[name]
            so = hc.solve_options(ol, error_state=es)
            r = gc.held_loop(ol, bb, so, n, R, fb, po, Rtab, gc.GM, plant, sat, hc.IDS, nthreads=8)
            r0 = hc.reference_loop(ol, bb, so, n, R, fb, po, plant, sat, hc.IDS, nthreads=8)
            gc.moved(r["X_hist"][:, -1], r0["X_hist"][:, -1], f"{name} R = {R} feedback = {fb}")
            assert np.all(r["statuses"] <= hc.TSAT_MAX_OUTER), "a block solve ended REG_FAIL or DIVERGED: its gains are undefined"
            refs[(name, R, fb)] = r
        return refs[(name, R, fb)]

    return dict(b=b, br=br, Rtab=Rtab, po=po, plant=plant, setups=setups, ref=ref)


def _run(pkg, solver, b, n, R, fb, po, Rtab, gm=gc.GM, error_state=0, **kw):
    prob = pkg.trajopt.BatchProblem.from_arrays(b, error_state=error_state)
    return pkg.mpc.receding_horizon_held_gg(prob, solver, n, R, Rtab, gm, feedback=fb, noise_opts=po, **kw)


def _case_run(pkg, solver, case, name, R, fb, gm=gc.GM):
    b, es, sat, n = case["setups"][name]
    return _run(pkg, solver, b, n, R, fb, case["po"], case["Rtab"], gm, error_state=es, plant=case["plant"], sat=sat, noise_id=hc.IDS)


def _tally(pkg, solver, T):
    t = np.zeros((T, 4), dtype=np.int64)
    assert pkg._abi.load().tsat_mpc_tally(solver._h, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return t


@pytest.mark.parametrize("R", [3, 5])
def test_gpu_saturated_hold_matches_reference(pkg, solver, case, R):
    """limits +-0.6, gains on: blocks 3 x 4 and 5 + 5 + 2; the last plan, the number of solves and the tally with it"""
    ref = case["ref"]("saturated", R, 1)
    got = _case_run(pkg, solver, case, "saturated", R, 1)
    got.update(solver.download(want_K=False))
    hc.same(ref, got, case["b"], case["po"], plan=True)
    assert got["n_solves"] == ref["n_solves"] == -(-N_STEPS // R)
    tally = _tally(pkg, solver, 8)
    print(f"tally {tally.tolist()}")
    # backward sweeps, dual updates and inner iterations are the oracle's; n_forward counts the sweeps of the backend that ran
    assert np.array_equal(tally[:, [0, 2, 3]], ref["tally"][:, [0, 2, 3]])


def test_gpu_wide_limits_fly_the_gains(pkg, solver, case):
    """limits +-25, R = 5: nothing clips, so U_hist of the held steps is U_j + K_j dx itself, on states the torque has moved"""
    for fb in (1, 0):
        ref = case["ref"]("wide", 5, fb)
        assert np.array_equal(ref["n_maybe"], np.zeros(8)), "a step of the wide-limits case is near a limit"
        got = _case_run(pkg, solver, case, "wide", 5, fb)
        got.update(solver.download(want_K=False))
        hc.same(ref, got, case["b"], case["po"], plan=True)
        assert np.array_equal(got["n_clipped"], np.zeros(8, dtype=np.int32))
        assert np.array_equal(_tally(pkg, solver, 8)[:, [0, 2, 3]], ref["tally"][:, [0, 2, 3]])


@pytest.mark.parametrize("R", [3, 5])
def test_gpu_ragged_horizons_with_quaternion_hooks(pkg, solver, case, R):
    """n_knots (20, 13, 6, 7, 20, 19, 6, 20), error_state = 1, 8 steps; R = 5 is the largest the six-knot horizons allow"""
    ref = case["ref"]("ragged", R, 1)
    got = _case_run(pkg, solver, case, "ragged", R, 1)
    got.update(solver.download(want_K=False))
    hc.same(ref, got, case["br"], case["po"], plan=True)
    assert np.array_equal(_tally(pkg, solver, 8)[:, [0, 2, 3]], ref["tally"][:, [0, 2, 3]])


def test_gpu_hold_at_gm0_is_bit_equal_to_the_held_entry_point(pkg, solver, case):
    b, es, sat, n = case["setups"]["saturated"]
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    for R, fb in ((3, 1), (1, 0)):
        old = pkg.mpc.receding_horizon_held(prob, solver, n, R, feedback=fb, plant=case["plant"], sat=sat, noise_opts=case["po"],
                                            noise_id=hc.IDS)
        old.update(solver.download(want_K=False))
        tally_old = _tally(pkg, solver, 8)
        new = _case_run(pkg, solver, case, "saturated", R, fb, gm=0.0)
        new.update(solver.download(want_K=False))
        for k in KEYS + ("X", "U"):
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)
        np.testing.assert_array_equal(tally_old, _tally(pkg, solver, 8))
        on = _case_run(pkg, solver, case, "saturated", R, fb)
        assert np.max(np.abs(on["X_hist"] - new["X_hist"])) >= gc.MOVED


def test_gpu_continuation_equals_one_longer_run(pkg, solver, case):
    """6 + 6 steps with step0 = 6 and no new upload at R = 3 (6 is a multiple of R) are the 12-step run, bit for bit"""
    b, es, sat, n = case["setups"]["saturated"]
    whole = _case_run(pkg, solver, case, "saturated", 3, 1)
    whole.update(solver.download(want_K=False))
    kw = dict(plant=case["plant"], sat=sat, noise_id=hc.IDS)
    first = _run(pkg, solver, b, 6, 3, 1, case["po"], case["Rtab"], **kw)
    second = _run(pkg, solver, b, 6, 3, 1, case["po"], case["Rtab"], step0=6, upload=False, **kw)
    second.update(solver.download(want_K=False))
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("stats", "X", "U"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)


def test_gpu_wave_boundary_tiled_batch_is_the_individual_loops(pkg, ol, solver):
    """2 slews x 33 realisations through mpc.tile_realisations: T = 66, lane 63 -> 64 inside slew 1, two lanes in the last wavefront,
    horizons (20, 13), 6 steps at R = 4 (4 + 2); all 66 against one-trajectory reference loops. The orbit table is per slew and
    follows btab_idx, so the tiled batch takes it as it is"""
    M, n, R = 33, 6, 4
    b = gc.use_3u(pkg, hc.mpc_batch(pkg, T=2, N=20))
    b.n_knots = np.array([20, 13], dtype=np.int32)
    Rtab = gc.orbit(pkg, b.n_tab, 0.2)[None]
    po = hc.noise_options(ol, **STAT)
    plant = hc.plants(pkg, b, M)
    id0 = np.array([5, 2 ** 33], dtype=np.int64)
    tiled, kw = pkg.mpc.tile_realisations(b, M, plant=plant, noise_id0=id0, sat=hc.SAT)
    assert tiled.T == 66
    got = _run(pkg, solver, tiled, n, R, 1, po, Rtab, **kw)
    o = hc.solve_options(ol)
    least = np.inf
    for t in range(2):
        for m in range(M):
            one_b = b.slice(t, t + 1)
            args = (plant[t, m][None], hc.SAT, id0[t:t + 1] + m)
            ref = gc.held_loop(ol, one_b, o, n, R, 1, po, Rtab, gc.GM, *args, nthreads=1)
            ref0 = hc.reference_loop(ol, one_b, o, n, R, 1, po, *args, nthreads=1)
            least = min(least, float(np.max(np.abs(ref["X_hist"][:, -1] - ref0["X_hist"][:, -1]))))
            assert np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
            i = t * M + m
            hc.same(ref, {k: got[k][i:i + 1] for k in KEYS}, one_b, po)
    print(f"the term moves the final state of every one of the 66 references by at least {least:.2e}")
    assert least >= gc.MOVED


def test_gpu_hold_rejections_and_workspace(pkg, ol, solver, case):
    """every listed error is a RuntimeError with its text (tsat_last_error) and launches nothing; a good call grows the handle's
    workspaces by the packed table over what tsat_mpc_run_held holds, and tsat_workspace_trim(h, 1) returns it"""
    lib, abi = pkg._abi.load(), pkg._abi
    b, po, Rtab = case["b"], case["po"], case["Rtab"]

    def edit(idx, v):
        r = Rtab.copy()
        r[idx] = v
        return r

    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    pkg.mpc.receding_horizon_held(prob, solver, 3, 3, noise_opts=po, sat=hc.SAT)       # the resident batch
    _trim(pkg, solver)
    for R_, gm, kw, word in ((edit((0, 9, 1), np.nan), gc.GM, {}, "non-finite Rtab entry in row 9"),
                             (edit((0, 199), 0.0), gc.GM, {}, r"row 199 has \|r\| = 0"), (Rtab, -2.0, {}, "gm must be finite"),
                             (Rtab, np.nan, {}, "gm must be finite"), (Rtab, gc.GM, dict(R=0), "replan_every must be >= 1"),
                             (Rtab, gc.GM, dict(R=20), "min n_knots - 1 = 19"), (Rtab, gc.GM, dict(fb=2), "feedback must be 0")):
        with pytest.raises(RuntimeError, match=word):
            _run(pkg, solver, b, 6, kw.get("R", 3), kw.get("fb", 1), po, R_, gm, sat=hc.SAT, upload=False)
        assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    # Rtab NULL: through the C ABI
    o = solver.opts.to_abi(b.N, b.n_tab, 3)
    o.max_outer, o.max_inner = 1, 3
    Xh, Uh = np.empty((8, 4, 7)), np.empty((8, 3, 3))
    d = abi.as_dp
    assert lib.tsat_mpc_run_held_gg(solver._h, C.byref(o), C.byref(po), 3, 0, 3, 1, None, None, None, None, d(Xh), d(Uh), None, None, None,
                                    None, None, gc.GM) == -1
    assert b"null Rtab" in lib.tsat_last_error(solver._h) and _ws(pkg, solver) == 0
    pkg.mpc.receding_horizon_held(prob, solver, 6, 3, noise_opts=po, sat=hc.SAT)
    w1 = _ws(pkg, solver)
    _run(pkg, solver, b, 6, 3, 1, po, Rtab, sat=hc.SAT)
    w2 = _ws(pkg, solver)
    assert w2 - w1 == 32 * Rtab.shape[0] * Rtab.shape[1], (w1, w2)
    _trim(pkg, solver)
    # the handle is as good as before: tsat_mpc_run on it matches the oracle on a 3-step run
    got = pkg.mpc.receding_horizon(prob, solver, 3, plant_integrator=4)
    ref = ol.mpc_batch(b, hc.solve_options(ol), 3, plant_integrator=4)
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-9 and np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-8
