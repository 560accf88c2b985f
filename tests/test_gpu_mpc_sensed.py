"""GPU tier of the held re-planning loop fed measurements (tsat_mpc_run_held_sensed through ``mpc.receding_horizon_held_sensed``)
against the reference loop of tests/mpc_sensed_common.py, on the smallest shapes at which the kernels can go wrong; the bars are the
project's MPC bars (mpc_dispersed_common.same), 1e-9 on Y_hist. Every parity case asserts its conditions on references alone
(mpc_sensed_common.conditions: mpc_held_common.condition, and sensor noise, gyro bias, attitude bias and latency each move the final
state by >= gg_common.MOVED) before a kernel result is looked at.

The workload is the held tests' (mpc_batch(T=8, N=20, seed=3), all five plant dispersions, plant noise on, limits +-0.6, ids
``mpc_held_common.IDS``, statistic w_tol 1.25e-4, angle_tol 3.0, min_steps 3); sensor sigmas ``sensed_common.SIGMAS``, biases at
twice ``sensed_common.BIAS`` (mpc_sensed_common says why). Measured on the reference: every block solve ends TSAT_MAX_OUTER and 3 of
8 fail in every case; margins 8.1e-3 (saturated, R = 3 and 5, either latency; ragged horizons with error_state = 1, R = 5, latency
1) and 3.6e-2 (with gravity: the 3U inertia, plants dispersed around it, R = 3, latency 0, where the torque itself moves the final
state by 3.3e-6). Sensor noise moves the final state by 8.3e-5 .. 4.1e-4, the gyro bias by 1.7e-5 .. 9.4e-5, the attitude bias by
1.7e-5 .. 8.8e-5, latency 1 against 0 by 5.7e-5 .. 2.7e-4 (bar 1e-7).

Measured on an MI355X against the reference: max |dX_hist| 1.7e-17, |dU_hist| 5.2e-13, |dY_hist| 2.8e-17 over the six parity
cases and the 66 tiled loops; the ideal sensor against tsat_mpc_run_held and tsat_mpc_run_held_gg: max |d| 0.0, bit-equal."""
import ctypes as C

import numpy as np
import pytest

import gg_common as gc
import mpc_held_common as hc
import mpc_sensed_common as mc
import sensed_common as sc

pytestmark = pytest.mark.gpu

N_STEPS = 12
KEYS = ("X_hist", "U_hist", "stats", "tracking_stats", "n_clipped")
Y_BAR = 1e-9
IDEAL_BAR = 1e-12            # the bar of test_gpu_sensed.py for "one computation restated in other code"


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


@pytest.fixture(scope="module")
def case(pkg, ol):
    """the workloads of the parity cases, and their references, each computed once on demand and left unchanged"""
    b = hc.mpc_batch(pkg, T=8, N=20, seed=3)
    br = hc.mpc_batch(pkg, T=8, N=20, seed=3)
    br.n_knots = hc.RAGGED.copy()
    bg = gc.use_3u(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    Rtab = gc.orbit(pkg, bg.n_tab, 0.2)[None]
    po = hc.noise_options(ol, min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
    plant, plant_g, bias = hc.plants(pkg, b), hc.plants(pkg, bg), mc.biases(pkg, 8)      # the plants are dispersed around the model's inertia
    setups = dict(saturated=(b, 0, N_STEPS, None, plant), ragged=(br, 1, 8, None, plant), gravity=(bg, 0, N_STEPS, Rtab, plant_g))
    refs = {}

    def ref(name, R, latency):
        if (name, R, latency) not in refs:
            bb, es, n, rt, pl = setups[name]
            o = hc.solve_options(ol, error_state=es)

            def ref_of(sens=mc.SIGMAS, bias=bias, latency=latency):
                return mc.reference_loop(ol, bb, o, n, R, 1, po, sens, bias, latency, pl, hc.SAT, hc.IDS, Rtab=rt,
                                         gm=gc.GM if rt is not None else 0.0, nthreads=8)

            refs[(name, R, latency)] = mc.conditions(ref_of, bias, f"{name} R = {R} latency = {latency}", bb, po)
        return refs[(name, R, latency)]

    return dict(b=b, br=br, bg=bg, Rtab=Rtab, po=po, plant=plant, plant_g=plant_g, bias=bias, setups=setups, ref=ref)


def _run(pkg, solver, b, n, R, po, error_state=0, fb=1, **kw):
    prob = pkg.trajopt.BatchProblem.from_arrays(b, error_state=error_state)
    return pkg.mpc.receding_horizon_held_sensed(prob, solver, n, R, feedback=fb, noise_opts=po, **kw)


def _case_run(pkg, solver, case, name, R, latency):
    b, es, n, rt, pl = case["setups"][name]
    return _run(pkg, solver, b, n, R, case["po"], error_state=es, sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=latency, Rtab=rt,
                gm=gc.GM if rt is not None else 0.0, plant=pl, sat=hc.SAT, noise_id=hc.IDS)


def _same(ref, got, b, po, plan=False):
    ok = hc.same(ref, got, b, po, plan=plan)
    dY = float(np.max(np.abs(ref["Y_hist"] - got["Y_hist"])))
    print(f"max|dY_hist| {dY:.2e}")
    assert dY < Y_BAR
    return ok


@pytest.mark.parametrize("R,latency", [(3, 0), (3, 1), (5, 0), (5, 1)])
def test_gpu_saturated_case_matches_reference(pkg, solver, case, R, latency):
    """limits +-0.6, gains on: blocks 3 x 4 and 5 + 5 + 2, either latency; the last plan, the number of solves and Y_hist with it"""
    ref = case["ref"]("saturated", R, latency)
    got = _case_run(pkg, solver, case, "saturated", R, latency)
    got.update(solver.download(want_K=False))
    assert _same(ref, got, case["b"], case["po"], plan=True).all()
    assert got["n_solves"] == ref["n_solves"] == -(-N_STEPS // R)
    assert np.max(np.abs(got["Y_hist"] - got["X_hist"][:, :-1])) > 1e-4      # X_hist holds true states, Y_hist what was measured


def test_gpu_ragged_horizons_with_quaternion_hooks(pkg, solver, case):
    """n_knots (20, 13, 6, 7, 20, 19, 6, 20), error_state = 1, R = 5, latency 1, 8 steps"""
    ref = case["ref"]("ragged", 5, 1)
    got = _case_run(pkg, solver, case, "ragged", 5, 1)
    assert _same(ref, got, case["br"], case["po"]).all()


def test_gpu_with_gravity_gradient(pkg, ol, solver, case):
    """the 3U inertia under the orbit table of ``gg_common.orbit`` (as test_gpu_gg.py builds it), R = 3, latency 0; the torque
    shows on the reference (against gm = 0), so a kernel that dropped the rows cannot pass"""
    ref = case["ref"]("gravity", 3, 0)
    bg, es, n, rt, pl = case["setups"]["gravity"]
    no_gm = mc.reference_loop(ol, bg, hc.solve_options(ol), n, 3, 1, case["po"], mc.SIGMAS, case["bias"], 0, pl, hc.SAT, hc.IDS,
                              Rtab=rt, gm=0.0, nthreads=8)
    mc.moved(ref, no_gm, "gravity gradient on against gm = 0")
    got = _case_run(pkg, solver, case, "gravity", 3, 0)
    assert _same(ref, got, bg, case["po"]).all()


def test_gpu_ideal_sensor_is_the_parent(pkg, solver, case):
    """sensor NULL, zero sigmas, latency 0 against tsat_mpc_run_held (Rtab NULL) and tsat_mpc_run_held_gg: bar 1e-12 on the
    histories and the plan, identical solve statistics and n_clipped; prints whether it is in fact bit-equal"""
    po = case["po"]
    for label, b, rt, pl in (("held", case["b"], None, case["plant"]), ("held_gg", case["bg"], case["Rtab"], case["plant_g"])):
        kw = dict(plant=pl, sat=hc.SAT, noise_id=hc.IDS)
        prob = pkg.trajopt.BatchProblem.from_arrays(b)
        if rt is None:
            old = pkg.mpc.receding_horizon_held(prob, solver, N_STEPS, 3, noise_opts=po, **kw)
        else:
            old = pkg.mpc.receding_horizon_held_gg(prob, solver, N_STEPS, 3, rt, gm=gc.GM, noise_opts=po, **kw)
        old.update(solver.download(want_K=False))
        new = _run(pkg, solver, b, N_STEPS, 3, po, Rtab=rt, gm=gc.GM if rt is not None else 0.0, **kw)
        new.update(solver.download(want_K=False))
        d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_hist", "U_hist", "X", "U"))
        bit = all(np.array_equal(old[k], new[k]) for k in ("X_hist", "U_hist", "X", "U"))
        print(f"ideal sensor against tsat_mpc_run_{label}: max|d| {d:.2e}, bit-equal: {bit}")
        assert d <= IDEAL_BAR
        for k in ("stats", "n_clipped"):
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)
        for k in ("slew_index", "failed", "slew_time"):
            np.testing.assert_array_equal(old["tracking_stats"][k], new["tracking_stats"][k], err_msg=k)
        assert np.max(np.abs(new["Y_hist"] - new["X_hist"][:, :-1])) <= IDEAL_BAR


def test_gpu_continuation_with_latency_0_equals_one_longer_run(pkg, solver, case):
    """6 + 6 steps with step0 = 6 and no new upload at R = 3 (6 is a multiple of R), latency 0, are the 12-step run, bit for bit,
    Y_hist included: the first call left the TRUE state behind, and the second call's first measurement is the one the longer run
    takes at the end of its second block"""
    b = case["b"]
    whole = _case_run(pkg, solver, case, "saturated", 3, 0)
    whole.update(solver.download(want_K=False))
    kw = dict(sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=0, plant=case["plant"], sat=hc.SAT, noise_id=hc.IDS)
    first = _run(pkg, solver, b, 6, 3, case["po"], **kw)
    x0 = np.array(solver.download(want_K=False)["X"][:, 0])
    second = _run(pkg, solver, b, 6, 3, case["po"], step0=6, upload=False, **kw)
    second.update(solver.download(want_K=False))
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(np.concatenate([first["Y_hist"], second["Y_hist"]], axis=1), whole["Y_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("stats", "X", "U"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)
    # the first call's last solve started from the measurement of step 3; what it left behind is the true state, which the second
    # call flies on from and measures
    assert np.max(np.abs(x0 - first["Y_hist"][:, 3])) < 1e-12
    np.testing.assert_array_equal(second["X_hist"][:, 0], first["X_hist"][:, -1])
    assert np.max(np.abs(first["X_hist"][:, -1] - second["Y_hist"][:, 0])) > 1e-4


def test_gpu_wave_boundary_tiled_batch_is_the_individual_loops(pkg, ol, solver):
    """2 slews x 33 realisations through mpc.tile_realisations with per-realisation biases: T = 66, lane 63 -> 64 inside slew 1, two
    lanes in the last wavefront, horizons (20, 13), 6 steps at R = 4 (4 + 2), latency 1; all 66 against one-trajectory reference loops"""
    M, n, R = 33, 6, 4
    b = hc.mpc_batch(pkg, T=2, N=20)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = hc.noise_options(ol, min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
    plant, sensor = hc.plants(pkg, b, M), mc.biases(pkg, 2, M)
    id0 = np.array([5, 2 ** 33], dtype=np.int64)
    tiled, kw = pkg.mpc.tile_realisations(b, M, plant=plant, noise_id0=id0, sat=hc.SAT, sensor=sensor)
    assert tiled.T == 66 and kw["sensor"].shape == (66, 9)
    got = _run(pkg, solver, tiled, n, R, po, sensor_opts=mc.SIGMAS, latency=1, **kw)
    o = hc.solve_options(ol)
    for t in range(2):
        for m in range(M):
            one_b = b.slice(t, t + 1)
            ref = mc.reference_loop(ol, one_b, o, n, R, 1, po, mc.SIGMAS, sensor[t, m][None], 1, plant[t, m][None], hc.SAT,
                                    id0[t:t + 1] + m, nthreads=1)
            assert np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
            i = t * M + m
            _same(ref, {k: got[k][i:i + 1] for k in KEYS + ("Y_hist",)}, one_b, po)


def test_gpu_bad_arguments_are_codes_and_texts(pkg, ol, solver, case):
    lib, abi = pkg._abi.load(), pkg._abi
    b, po, bias = case["b"], case["po"], case["bias"]
    for kw, word in ((dict(sensor_opts=dict(sigma_gyro=-1.0)), "must be finite and >= 0"),
                     (dict(sensor_opts=dict(sigma_att=float("nan"))), "must be finite and >= 0"),
                     (dict(latency=2), "latency must be 0"),
                     (dict(gm=gc.GM), "Rtab may be NULL only with gm == 0"),
                     (dict(R=0), "replan_every must be >= 1"), (dict(R=20), "min n_knots - 1 = 19")):
        kw = dict(kw)
        with pytest.raises(RuntimeError, match=word):
            _run(pkg, solver, b, 8, kw.pop("R", 3), po, sat=hc.SAT, **kw)
    z = bias.copy()
    z[5, 4] = np.inf
    with pytest.raises(RuntimeError, match=r"non-finite sensor entry at \(t, m\) = \(5, 0\)"):
        _run(pkg, solver, b, 8, 3, po, sat=hc.SAT, sensor=z)
    # s NULL and NULL X_hist: through the C ABI
    o = solver.opts.to_abi(b.N, b.n_tab, 3)
    o.max_outer, o.max_inner = 1, 3
    so = sc.sensor_options(abi, mc.SIGMAS, 0)
    Xh, Uh = np.empty((8, 4, 7)), np.empty((8, 3, 3))
    d = abi.as_dp
    before = lib.tsat_workspace_bytes(solver._h)
    assert lib.tsat_mpc_run_held_sensed(solver._h, C.byref(o), C.byref(po), 3, 0, 3, 1, None, None, None, None, d(Xh), d(Uh), None, None,
                                        None, None, None, 0.0, None, None, None) == -1
    assert b"null sensor options" in lib.tsat_last_error(solver._h)
    assert lib.tsat_mpc_run_held_sensed(solver._h, C.byref(o), C.byref(po), 3, 0, 3, 1, None, None, None, None, None, d(Uh), None, None,
                                        None, None, None, 0.0, C.byref(so), None, None) == -1
    assert b"null array" in lib.tsat_last_error(solver._h)
    assert lib.tsat_workspace_bytes(solver._h) == before                   # a rejected call grows no workspace
    # the handle is as good as before: tsat_mpc_run on it matches the oracle on a 3-step run
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    got = pkg.mpc.receding_horizon(prob, solver, 3, plant_integrator=4)
    ref = ol.mpc_batch(b, hc.solve_options(ol), 3, plant_integrator=4)
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-9 and np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
