"""GPU tier of the receding-horizon loop on a noisy, dispersed plant with limits (tsat_mpc_run_dispersed through
``mpc.receding_horizon_dispersed``) against the reference loop of tests/mpc_dispersed_common.py, on the smallest shapes at which
the kernel can go wrong; the bars are the project's MPC bars (mpc_dispersed_common.same)."""
import ctypes as C

import numpy as np
import pytest

import mpc_dispersed_common as mc

pytestmark = pytest.mark.gpu

N_STEPS = 12
# statistic of case 1, chosen on the reference alone (seed 3: min |w| over the judged samples 0.49e-4 .. 1.28e-4 rad/s, error angles
# 1.73 .. 4.19 rad, hardly moving over 2.4 s): four of the eight arrive, three fail on the angle, one on the rate
W_TOL, ANGLE_TOL, MIN_STEPS = 1.25e-4, 3.0, 3
IDS = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


@pytest.fixture(scope="module")
def case1(pkg, ol):
    """T = 8, N = 20, 12 steps: all five dispersions (non-diagonal Jp on an isotropic model), noise, limits, ids; the reference
    once, with the condition on the seed checked before any kernel result is looked at"""
    b = mc.mpc_batch(pkg, T=8, N=20, seed=3)
    po = mc.noise_options(ol, min_steps=MIN_STEPS, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant = mc.plants(pkg, b)
    assert np.all(np.abs(plant[:, [1, 2, 5]]) > 0)
    ref = mc.reference_loop(ol, b, mc.solve_options(ol), N_STEPS, po, plant, mc.SAT, IDS, nthreads=8)
    m = mc.margins(ref, b, po)
    failed = ref["tracking_stats"]["failed"]
    print(f"case 1 reference: margins {m}, failed {failed}")
    assert np.all(m > mc.MARGIN), "a trajectory of the chosen seed sits on a threshold"
    assert 0 < np.count_nonzero(failed) < 8, "the reference must have both arrivals and failures"
    return b, po, plant, ref


def _run(pkg, solver, b, n, po, error_state=0, **kw):
    prob = pkg.trajopt.BatchProblem.from_arrays(b, error_state=error_state)
    return pkg.mpc.receding_horizon_dispersed(prob, solver, n, noise_opts=po, **kw)


def test_gpu_dispersed_loop_matches_reference(pkg, solver, case1):
    b, po, plant, ref = case1
    got = _run(pkg, solver, b, N_STEPS, po, plant=plant, sat=mc.SAT, noise_id=IDS, step0=0)
    got.update(solver.download(want_K=False))
    ok = mc.same(ref, got, b, po, plan=True)
    assert ok.all()


def test_gpu_ragged_horizons_with_quaternion_hooks(pkg, ol, solver):
    b = mc.mpc_batch(pkg, T=8, N=20, seed=3)
    b.n_knots = np.array([20, 13, 2, 7, 20, 19, 3, 20], dtype=np.int32)
    po = mc.noise_options(ol, min_steps=MIN_STEPS, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant = mc.plants(pkg, b)
    ref = mc.reference_loop(ol, b, mc.solve_options(ol, error_state=1), 8, po, plant, mc.SAT, IDS, nthreads=8)
    got = _run(pkg, solver, b, 8, po, error_state=1, plant=plant, sat=mc.SAT, noise_id=IDS)
    mc.same(ref, got, b, po)


def test_gpu_continuation_equals_one_longer_run(pkg, solver, case1):
    b, po, plant, ref = case1
    first = _run(pkg, solver, b, 8, po, plant=plant, sat=mc.SAT, noise_id=IDS)
    second = _run(pkg, solver, b, 4, po, plant=plant, sat=mc.SAT, noise_id=IDS, step0=8, upload=False)
    np.testing.assert_array_equal(second["X_hist"][:, 0], first["X_hist"][:, -1])
    X = np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1)
    U = np.concatenate([first["U_hist"], second["U_hist"]], axis=1)
    dX, dU = float(np.max(np.abs(X - ref["X_hist"]))), float(np.max(np.abs(U - ref["U_hist"])))
    print(f"8 + 4 steps against one 12-step reference: max|dX_hist| {dX:.2e} max|dU_hist| {dU:.2e}")
    assert dX < 1e-9 and dU < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], second["stats"][k]), k
    n = first["n_clipped"] + second["n_clipped"]
    assert np.all(ref["n_sure"] <= n) and np.all(n <= ref["n_maybe"])
    # the second call's statistic counts its own five samples
    ts = mc.dc.stats_of(pkg._abi, ref["X_hist"][:, 8:], b.xf, np.full(8, 5), b.dt, po.min_steps, po.w_tol, po.angle_tol)
    for k in ("slew_index", "failed", "slew_time"):
        assert np.array_equal(ts[k], second["tracking_stats"][k]), k
    # without step0 the continued call draws the noise of knots 0 .. 3 again: another history
    third = _run(pkg, solver, b, 8, po, plant=plant, sat=mc.SAT, noise_id=IDS)
    again = _run(pkg, solver, b, 4, po, plant=plant, sat=mc.SAT, noise_id=IDS, step0=0, upload=False)
    np.testing.assert_array_equal(third["X_hist"], first["X_hist"])
    assert np.max(np.abs(again["X_hist"][:, 1] - second["X_hist"][:, 1])) > 1e-9


def test_gpu_nominal_limit_is_the_existing_loop(pkg, ol, solver):
    """plant = NULL, noise_mode = 0, no limits on the configs[4] shape of tests/test_mpc.py (T = 8, N = 200, 30 steps) against
    tsat_mpc_run on a fresh upload of the same batch; not bit-equal by construction (the plant flies the full-tensor instantiation)"""
    lib, abi = pkg._abi.load(), pkg._abi
    b = mc.mpc_batch(pkg, T=8, N=200, seed=3, rows=400)
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    old = pkg.mpc.receding_horizon(prob, solver, 30, plant_integrator=4)
    old.update(solver.download(want_K=False))
    tally_old = np.zeros((8, 4), dtype=np.int64)
    assert lib.tsat_mpc_tally(solver._h, tally_old.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    new = _run(pkg, solver, b, 30, mc.noise_options(ol, noise=False))
    new.update(solver.download(want_K=False))
    tally_new = np.zeros((8, 4), dtype=np.int64)
    assert lib.tsat_mpc_tally(solver._h, tally_new.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    dX = float(np.max(np.abs(old["X_hist"] - new["X_hist"])))
    print(f"nominal limit: max|dX_hist| against tsat_mpc_run {dX:.2e}, max|dU_hist| {np.max(np.abs(old['U_hist'] - new['U_hist'])):.2e}")
    assert dX < 1e-9 and np.max(np.abs(old["U_hist"] - new["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status", "outer_iters", "n_backward"):
        assert np.array_equal(old["stats"][k], new["stats"][k]), k
    assert np.max(np.abs(old["X"] - new["X"])) < 1e-9 and np.max(np.abs(old["U"] - new["U"])) < 1e-8
    assert np.array_equal(tally_old, tally_new) and tally_new[:, 3].min() >= 30
    assert np.array_equal(new["n_clipped"], np.zeros(8, dtype=np.int32))
    ts = mc.dc.stats_of(abi, new["X_hist"], b.xf, np.full(8, 31), b.dt)
    for k in ("slew_index", "failed", "slew_time"):
        assert np.array_equal(ts[k], new["tracking_stats"][k]), k


def test_gpu_tiled_batch_is_the_individual_loops(pkg, ol, solver):
    """T = 2 slews x M = 4 realisations through mpc.tile_realisations = eight one-trajectory reference loops with ids id0[t] + m"""
    M, n = 4, 6
    b = mc.mpc_batch(pkg, T=2, N=20)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = mc.noise_options(ol, min_steps=MIN_STEPS, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant = mc.plants(pkg, b, M)
    id0 = np.array([5, 2 ** 33], dtype=np.int64)
    tiled, kw = pkg.mpc.tile_realisations(b, M, plant=plant, noise_id0=id0, sat=mc.SAT)
    got = _run(pkg, solver, tiled, n, po, **kw)
    o = mc.solve_options(ol)
    for t in range(2):
        for m in range(M):
            ref = mc.reference_loop(ol, b.slice(t, t + 1), o, n, po, plant[t, m][None], mc.SAT, id0[t:t + 1] + m, nthreads=1)
            i = t * M + m
            one = {k: got[k][i:i + 1] for k in ("X_hist", "U_hist", "stats", "tracking_stats", "n_clipped")}
            mc.same(ref, one, b.slice(t, t + 1), po)
    # model's plant, no limits: the draws of realisation (t, m) are the ones the ensemble gets for the same id — one control step
    # whose four stages take their nine values from tracking.generated_noise (field noise raised so that it shows above the bar)
    po = mc.noise_options(ol, field_amp=1e-6)
    tiled, kw = pkg.mpc.tile_realisations(b, M, noise_id0=id0)
    gen = pkg.tracking.generated_noise(mc.SEED, kw["noise_id"], 2, po.sigma_gyro, po.sigma_att, po.field_amp)     # (T M, 1, 4, 9)
    for i in range(2 * M):
        nz = ol.plant_noise(mc.SEED, int(kw["noise_id"][i]), 0, 0, po.sigma_gyro, po.sigma_att, po.field_amp)
        np.testing.assert_allclose(gen[i, 0, 0], nz, rtol=1e-12, atol=0)
    ref = mc.reference_loop(ol, tiled, o, 1, po, noise_fn=lambda t, k, st: gen[t, k, st])
    got = _run(pkg, solver, tiled, 1, po, noise_id=kw["noise_id"])
    d = float(np.max(np.abs(ref["X_hist"] - got["X_hist"])))
    quiet = mc.reference_loop(ol, tiled, o, 1, mc.noise_options(ol, noise=False))
    print(f"one step on the ensemble's draws: max|dX_hist| {d:.2e}; the draws move the state by {np.max(np.abs(quiet['X_hist'] - ref['X_hist'])):.2e}")
    assert d < 1e-9 and np.max(np.abs(quiet["X_hist"] - ref["X_hist"])) > 1e-6


def test_gpu_bad_arguments_are_codes_and_texts(pkg, ol, solver):
    lib, abi = pkg._abi.load(), pkg._abi
    b = mc.mpc_batch(pkg, T=2, N=20)
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    plant = mc.plants(pkg, b)
    po = mc.noise_options(ol)
    run = lambda **kw: pkg.mpc.receding_horizon_dispersed(prob, solver, kw.pop("n", 3), noise_opts=kw.pop("po", po), **kw)
    run(plant=plant, sat=mc.SAT)
    for kw, word in ((dict(n=0), "n_steps"), (dict(step0=-1), "step0"), (dict(sat=(np.full(3, 0.6), np.full(3, -0.6))), "sat_lo > sat_hi"),
                     (dict(plant=-plant), "not positive definite at t = 0"), (dict(po=mc.noise_options(ol, rate_as_written=1)), "rate_as_written"),
                     (dict(po=mc.noise_options(ol, noise_mode=3)), "noise_mode")):
        with pytest.raises(RuntimeError, match=word):
            run(**kw)
    p = plant.copy(); p[1, 12] = np.inf
    with pytest.raises(RuntimeError, match="non-finite plant entry at t = 1"):
        run(plant=p)
    p = plant.copy(); p[1, 3] += 1e-9 * p[1, 0]
    with pytest.raises(RuntimeError, match="Jp is not symmetric at t = 1"):
        run(plant=p)
    # exactly one limit array, precision 32: through the C ABI
    o = solver.opts.to_abi(b.N, b.n_tab, 3)
    o.max_outer, o.max_inner = 1, 3
    Xh, Uh, lo = np.empty((2, 4, 7)), np.empty((2, 3, 3)), np.full((2, 3), -0.6)
    d = abi.as_dp
    call = lambda o_, lo_, hi_: lib.tsat_mpc_run_dispersed(solver._h, C.byref(o_), C.byref(po), 3, 0, None, lo_, hi_, None, d(Xh), d(Uh),
                                                           None, None, None, None)
    assert call(o, d(lo), None) == -1 and b"exactly one" in lib.tsat_last_error(solver._h)
    o32 = o.copy(); o32.precision = 32
    assert call(o32, None, None) == -1 and b"precision" in lib.tsat_last_error(solver._h)
    assert lib.tsat_mpc_run_dispersed(solver._h, C.byref(o), C.byref(po), 3, 0, None, None, None, None, None, d(Uh), None, None, None, None) == -1
    assert lib.tsat_mpc_run_dispersed(solver._h, C.byref(o), None, 3, 0, None, None, None, None, d(Xh), d(Uh), None, None, None, None) == -1
    # the handle is as good as before: tsat_mpc_run on it matches the oracle on a 3-step run
    got = pkg.mpc.receding_horizon(prob, solver, 3, plant_integrator=4)
    ref = ol.mpc_batch(b, mc.solve_options(ol), 3, plant_integrator=4)
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-9 and np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
