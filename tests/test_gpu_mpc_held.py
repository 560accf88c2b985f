"""GPU tier of the loop that re-plans every R control steps and flies the solver's gains in between (tsat_mpc_run_held through
``mpc.receding_horizon_held``) against the reference loop of tests/mpc_held_common.py, on the smallest shapes at which the kernels
can go wrong; the bars are the project's MPC bars (mpc_dispersed_common.same). Every case asserts its condition on the reference
alone (mpc_held_common.condition) before a kernel result is looked at.

Measured on the reference (workload mpc_batch(T=8, N=20, seed=3), all five dispersions, noise on): saturated case, limits +-0.6:
every block solve ends TSAT_MAX_OUTER with 3 inner iterations, every step clips with the gains on, 4 of 8 fail with the gains and 3
without, margins >= 7.5e-3; wide limits +-25 at R = 5: no step clips, max |U_hist| 20.4, gains on against off differ by 0.76 in
U_hist, 6 of 8 fail, margin 3.6e-2; ragged horizons with error_state = 1: 4 of 8 fail, margin 8.1e-3."""
import ctypes as C

import numpy as np
import pytest

import mpc_held_common as hc

pytestmark = pytest.mark.gpu

N_STEPS = 12
KEYS = ("X_hist", "U_hist", "stats", "tracking_stats", "n_clipped")


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


@pytest.fixture(scope="module")
def case(pkg, ol):
    """the workload of all three cases, and their references, each computed once on demand and left unchanged"""
    b = hc.mpc_batch(pkg, T=8, N=20, seed=3)
    br = hc.mpc_batch(pkg, T=8, N=20, seed=3)
    br.n_knots = hc.RAGGED.copy()
    po = hc.noise_options(ol, min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
    plant = hc.plants(pkg, b)
    setups = dict(saturated=(b, 0, hc.SAT, N_STEPS), wide=(b, 0, hc.WIDE, N_STEPS), ragged=(br, 1, hc.SAT, 8))
    refs = {}

    def ref(name, R, fb):
        if (name, R, fb) not in refs:
            bb, es, sat, n = setups[name]
            r = hc.reference_loop(ol, bb, hc.solve_options(ol, error_state=es), n, R, fb, po, plant, sat, hc.IDS, nthreads=8)
            hc.condition(r, bb, po, f"{name} R = {R} feedback = {fb}")
            refs[(name, R, fb)] = r
        return refs[(name, R, fb)]

    return dict(b=b, br=br, po=po, plant=plant, setups=setups, ref=ref)


def _run(pkg, solver, b, n, R, fb, po, error_state=0, **kw):
    prob = pkg.trajopt.BatchProblem.from_arrays(b, error_state=error_state)
    return pkg.mpc.receding_horizon_held(prob, solver, n, R, feedback=fb, noise_opts=po, **kw)


def _case_run(pkg, solver, case, name, R, fb):
    b, es, sat, n = case["setups"][name]
    return _run(pkg, solver, b, n, R, fb, case["po"], error_state=es, plant=case["plant"], sat=sat, noise_id=hc.IDS)


def _tally(pkg, solver, T):
    t = np.zeros((T, 4), dtype=np.int64)
    assert pkg._abi.load().tsat_mpc_tally(solver._h, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return t


@pytest.mark.parametrize("R", [3, 5])
def test_gpu_saturated_hold_matches_reference(pkg, solver, case, R):
    """limits +-0.6, gains on: blocks 3 x 4 and 5 + 5 + 2; the last plan, the number of solves and the tally with it"""
    ref = case["ref"]("saturated", R, 1)
    assert np.array_equal(ref["n_sure"], np.full(8, N_STEPS)), "every step of the saturated case clips"
    got = _case_run(pkg, solver, case, "saturated", R, 1)
    got.update(solver.download(want_K=False))
    ok = hc.same(ref, got, case["b"], case["po"], plan=True)
    assert ok.all()
    assert got["n_solves"] == ref["n_solves"] == -(-N_STEPS // R)
    tally = _tally(pkg, solver, 8)
    print(f"tally {tally.tolist()}")
    # backward sweeps, dual updates and inner iterations are the oracle's; n_forward counts the sweeps of the backend that ran
    # (include/tortoise_hip.h), so its sum is taken from the same loop flown block by block: every call one solve, whose
    # statistics come back (a continuation after whole blocks is the longer run, bit for bit)
    assert np.array_equal(tally[:, [0, 2, 3]], ref["tally"][:, [0, 2, 3]])
    assert np.array_equal(tally[:, 3], np.full(8, 3 * ref["n_solves"]))
    b, es, sat, n = case["setups"]["saturated"]
    n_forward, parts = np.zeros(8, dtype=np.int64), []
    for s0 in range(0, n, R):
        one = _run(pkg, solver, b, min(R, n - s0), R, 1, case["po"], plant=case["plant"], sat=sat, noise_id=hc.IDS, step0=s0,
                   upload=s0 == 0)
        n_forward += one["stats"]["n_forward"]
        parts.append(one["X_hist"][:, :-1])
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), got["X_hist"][:, :-1])
    assert np.array_equal(tally[:, 1], n_forward), (tally[:, 1], n_forward)


def test_gpu_wide_limits_fly_the_gains(pkg, solver, case):
    """limits +-25, R = 5: nothing clips, so U_hist of the held steps is U_j + K_j dx itself; a kernel that ignores K cannot pass"""
    got = {}
    for fb in (1, 0):
        ref = case["ref"]("wide", 5, fb)
        assert np.array_equal(ref["n_maybe"], np.zeros(8)), "a step of the wide-limits case is near a limit"
        got[fb] = _case_run(pkg, solver, case, "wide", 5, fb)
        assert hc.same(ref, got[fb], case["b"], case["po"]).all()
        assert np.array_equal(got[fb]["n_clipped"], np.zeros(8, dtype=np.int32))
    dU = float(np.max(np.abs(got[1]["U_hist"] - got[0]["U_hist"])))
    dX = float(np.max(np.abs(got[1]["X_hist"] - got[0]["X_hist"])))
    print(f"gains on against off: max|dU_hist| {dU:.2e} max|dX_hist| {dX:.2e}")
    assert dU > 1e-6 and dX > 1e-6


@pytest.mark.parametrize("R", [3, 5])
def test_gpu_ragged_horizons_with_quaternion_hooks(pkg, solver, case, R):
    """n_knots (20, 13, 6, 7, 20, 19, 6, 20), error_state = 1, 8 steps; R = 5 is the largest the six-knot horizons allow"""
    ref = case["ref"]("ragged", R, 1)
    got = _case_run(pkg, solver, case, "ragged", R, 1)
    assert hc.same(ref, got, case["br"], case["po"]).all()


@pytest.mark.parametrize("fb", [0, 1])
def test_gpu_r1_is_bit_equal_to_the_every_step_loop(pkg, solver, case, fb):
    b, es, sat, n = case["setups"]["saturated"]
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    old = pkg.mpc.receding_horizon_dispersed(prob, solver, n, plant=case["plant"], sat=sat, noise_opts=case["po"], noise_id=hc.IDS)
    old.update(solver.download(want_K=False))
    tally_old = _tally(pkg, solver, 8)
    new = _case_run(pkg, solver, case, "saturated", 1, fb)
    new.update(solver.download(want_K=False))
    tally_new = _tally(pkg, solver, 8)
    for k in KEYS + ("X", "U"):
        np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    np.testing.assert_array_equal(tally_old, tally_new)
    assert new["n_solves"] == n


def test_gpu_continuation_equals_one_longer_run(pkg, solver, case):
    """6 + 6 steps with step0 = 6 and no new upload at R = 3 (6 is a multiple of R) are the 12-step run, bit for bit"""
    b, es, sat, n = case["setups"]["saturated"]
    whole = _case_run(pkg, solver, case, "saturated", 3, 1)
    whole.update(solver.download(want_K=False))
    kw = dict(plant=case["plant"], sat=sat, noise_id=hc.IDS)
    first = _run(pkg, solver, b, 6, 3, 1, case["po"], **kw)
    second = _run(pkg, solver, b, 6, 3, 1, case["po"], step0=6, upload=False, **kw)
    second.update(solver.download(want_K=False))
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("stats", "X", "U"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)
    # the second call's statistic counts its own seven samples
    ts = hc.dc.stats_of(pkg._abi, whole["X_hist"][:, 6:], b.xf, np.full(8, 7), b.dt, hc.MIN_STEPS, hc.W_TOL, hc.ANGLE_TOL)
    for k in ("slew_index", "failed", "slew_time"):
        assert np.array_equal(ts[k], second["tracking_stats"][k]), k


def test_gpu_wave_boundary_tiled_batch_is_the_individual_loops(pkg, ol, solver):
    """2 slews x 33 realisations through mpc.tile_realisations: T = 66, lane 63 -> 64 inside slew 1, two lanes in the last wavefront,
    horizons (20, 13), 6 steps at R = 4 (4 + 2); all 66 against one-trajectory reference loops"""
    M, n, R = 33, 6, 4
    b = hc.mpc_batch(pkg, T=2, N=20)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = hc.noise_options(ol, min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
    plant = hc.plants(pkg, b, M)
    id0 = np.array([5, 2 ** 33], dtype=np.int64)
    tiled, kw = pkg.mpc.tile_realisations(b, M, plant=plant, noise_id0=id0, sat=hc.SAT)
    assert tiled.T == 66
    got = _run(pkg, solver, tiled, n, R, 1, po, **kw)
    o = hc.solve_options(ol)
    for t in range(2):
        for m in range(M):
            one_b = b.slice(t, t + 1)
            ref = hc.reference_loop(ol, one_b, o, n, R, 1, po, plant[t, m][None], hc.SAT, id0[t:t + 1] + m, nthreads=1)
            assert np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
            i = t * M + m
            hc.same(ref, {k: got[k][i:i + 1] for k in KEYS}, one_b, po)


def test_gpu_bad_arguments_are_codes_and_texts(pkg, ol, solver, case):
    lib, abi = pkg._abi.load(), pkg._abi
    b, br, po = case["b"], case["br"], case["po"]
    for bb, kw, word in ((b, dict(R=0), "replan_every must be >= 1"), (b, dict(R=20), "min n_knots - 1 = 19"),
                         (br, dict(R=6), "min n_knots - 1 = 5"), (b, dict(R=3, fb=2), "feedback must be 0")):
        with pytest.raises(RuntimeError, match=word):
            _run(pkg, solver, bb, 8, kw["R"], kw.get("fb", 1), po, sat=hc.SAT)
    _run(pkg, solver, br, 8, 5, 1, po, sat=hc.SAT)            # the largest interval the ragged batch allows runs
    # NULL X_hist, and everything tsat_mpc_run_dispersed rejects: through the C ABI
    o = solver.opts.to_abi(b.N, b.n_tab, 3)
    o.max_outer, o.max_inner = 1, 3
    Xh, Uh = np.empty((8, 4, 7)), np.empty((8, 3, 3))
    d = abi.as_dp
    assert lib.tsat_mpc_run_held(solver._h, C.byref(o), C.byref(po), 3, 0, 3, 1, None, None, None, None, None, d(Uh), None, None, None,
                                 None) == -1
    assert b"null array" in lib.tsat_last_error(solver._h)
    assert lib.tsat_mpc_run_held(solver._h, C.byref(o), C.byref(po), 0, 0, 3, 1, None, None, None, None, d(Xh), d(Uh), None, None, None,
                                 None) == -1
    assert b"n_steps" in lib.tsat_last_error(solver._h)
    # the handle is as good as before: tsat_mpc_run on it matches the oracle on a 3-step run
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    got = pkg.mpc.receding_horizon(prob, solver, 3, plant_integrator=4)
    ref = ol.mpc_batch(b, hc.solve_options(ol), 3, plant_integrator=4)
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-9 and np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
