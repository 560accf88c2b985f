"""GPU tier of the held re-planning loop behind the magnetometer-updated nine-state filter (tsat_mpc_run_held_model_mag_filtered
through ``mpc.receding_horizon_held_model_mag_filtered``) against the reference loop of tests/mpc_model_mag_filtered_common.py, on
the shapes of tests/test_gpu_mpc_model_filtered.py, the smallest at which these kernels can go wrong; the bars are the project's MPC
bars (mpc_dispersed_common.same), 1e-9 on Y_hist, filt_state and filt_final. Every parity case asserts its conditions on references
alone (mpc_model_mag_filtered_common.conditions) before a kernel result is looked at.

The workload is the parent's (mpc_batch(T=8, N=20, seed=3), all five plant dispersions, plant noise on, ids
``mpc_held_common.IDS``, statistic w_tol 1.25e-4, angle_tol 3.0, min_steps 3) over 12 steps; sensor sigmas ``sensed_common.SIGMAS``,
biases at twice ``sensed_common.BIAS``; filter levels ``model_mag_filtered_common.FILT``; the field table's rows are 10 s apart, 60 s
in the gravity case; the three saturated cases fly the held tests' limits +-0.6 and the gravity case +-3, as behind the parent. ONE
LEVEL DIFFERS FROM THE PARENT'S, chosen on the reference alone: the ragged case flies limits +-1.5, not +-3. Behind this filter all
eight trajectories of that case fail the statistic at +-3 (and at +-6), so ``mpc_held_common.condition`` — arrivals and failures both
present — is not met; at +-1.5 one arrives, seven fail, the smallest margin is 3.6e-2 and every term shows. Measured on the
references (bar gg_common.MOVED = 1e-7), over the five cases: the filter on against off 2.9e-4 .. 6.9e-4, against the
attitude-updated model filter 3.0e-4 .. 6.0e-4, the magnetometer update 2.6e-4 .. 6.9e-4, the row the delayed sample is paired with
1.1e-4 .. 2.7e-4, the clock's off-by-one in predict 1.7e-7 .. 1.3e-6, latency 1 against 0 1.2e-4 .. 3.1e-4, the prediction across
the delay 4.7e-5 .. 9.5e-5: no case leaves a condition to another. Every figure of every case is printed. The measured differences
are in profiles/mpc/model_mag_filtered_differences.txt."""
import ctypes as C

import numpy as np
import pytest

import gg_common as gc
import model_mag_filtered_common as mg
import mpc_held_common as hc
import mpc_model_filtered_common as mf
import mpc_model_mag_filtered_common as mq
import mpc_sensed_common as mc
import sensed_common as sc

pytestmark = pytest.mark.gpu

N_STEPS = 12
KEYS = ("X_hist", "U_hist", "stats", "tracking_stats", "n_clipped")
EST = ("Y_hist", "filt_state", "filt_final")
SAT3 = (np.full(3, -3.0), np.full(3, 3.0))
SAT15 = (np.full(3, -1.5), np.full(3, 1.5))


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
    b = mq.coarse_rows(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    br = mq.coarse_rows(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3))
    br.n_knots = hc.RAGGED.copy()
    bg = mq.coarse_rows(pkg, gc.use_3u(pkg, hc.mpc_batch(pkg, T=8, N=20, seed=3)), 60.0)
    Rtab = gc.orbit(pkg, bg.n_tab, 0.2)[None]
    po = hc.noise_options(ol, min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
    plant, plant_g, bias = hc.plants(pkg, b), hc.plants(pkg, bg), mc.biases(pkg, 8)
    setups = dict(saturated=(b, 0, N_STEPS, None, plant, hc.SAT), ragged=(br, 1, 8, None, plant, SAT15),
                  gravity=(bg, 0, N_STEPS, Rtab, plant_g, SAT3))
    refs = {}

    def ref(name, R, latency):
        if (name, R, latency) not in refs:
            bb, es, n, rt, pl, sat = setups[name]
            o = hc.solve_options(ol, error_state=es)
            kw = dict(Rtab=rt, gm=gc.GM if rt is not None else 0.0, nthreads=8)

            def ref_of(filt=mq.FILT, latency=latency, variant=mq.VARIANT):
                return mq.reference_loop(ol, bb, o, n, R, 1, po, mc.SIGMAS, bias, latency, pl, sat, hc.IDS, filt=filt, variant=variant, **kw)

            def parent():
                return mf.reference_loop(ol, bb, o, n, R, 1, po, mc.SIGMAS, bias, latency, pl, sat, hc.IDS, filt=mf.FILT, **kw)

            refs[(name, R, latency)] = mq.conditions(ref_of, f"{name} R = {R} latency = {latency}", bb, po, parent=parent)
        return refs[(name, R, latency)]

    return dict(b=b, br=br, bg=bg, Rtab=Rtab, po=po, plant=plant, plant_g=plant_g, bias=bias, setups=setups, ref=ref)


def _run(pkg, solver, b, n, R, po, error_state=0, fb=1, filt=mq.FILT, **kw):
    prob = pkg.trajopt.BatchProblem.from_arrays(b, error_state=error_state)
    f = None if filt is None else mg.filter_options(pkg._abi, filt)
    return pkg.mpc.receding_horizon_held_model_mag_filtered(prob, solver, n, R, filter=f, feedback=fb, noise_opts=po, **kw)


def _case_run(pkg, solver, case, name, R, latency, **kw):
    b, es, n, rt, pl, sat = case["setups"][name]
    return _run(pkg, solver, b, n, R, case["po"], error_state=es, sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=latency, Rtab=rt,
                gm=gc.GM if rt is not None else 0.0, plant=pl, sat=sat, noise_id=hc.IDS, **kw)


def _same(ref, got, b, po, plan=False, keys=EST):
    ok = hc.same(ref, got, b, po, plan=plan)
    mq.same_estimates(ref, got, keys)
    return ok


@pytest.mark.parametrize("R,latency", [(3, 0), (3, 1), (5, 1)])
def test_gpu_saturated_case_matches_reference(pkg, ol, solver, case, R, latency):
    """limits +-0.6, gains on: blocks 3 x 4 and 5 + 5 + 2; the last plan, the number of solves, Y_hist and the records with it; Y_hist
    and the records also against the recursion run over the gyro and magnetometer samples of the returned history"""
    ref = case["ref"]("saturated", R, latency)
    got = _case_run(pkg, solver, case, "saturated", R, latency)
    got.update(solver.download(want_K=False))
    assert _same(ref, got, case["b"], case["po"], plan=True).all()
    assert got["n_solves"] == ref["n_solves"] == -(-N_STEPS // R)
    assert np.max(np.abs(got["Y_hist"] - got["X_hist"][:, :-1])) > 1e-4      # X_hist holds true states, Y_hist the estimates
    handed = mq.measured(ol, case["b"], case["po"], got["X_hist"], mc.SIGMAS, case["bias"], latency, hc.IDS)
    Y, S, F = mq.estimates(ol, case["b"], hc.solve_options(ol).u_scale, mq.FILT, handed, got["U_hist"], latency)
    mq.same_estimates(dict(Y_hist=Y, filt_state=S, filt_final=F), got)


def test_gpu_ragged_horizons_with_quaternion_hooks(pkg, solver, case):
    """n_knots (20, 13, 6, 7, 20, 19, 6, 20), error_state = 1, R = 5, latency 1, 8 steps, limits +-1.5"""
    ref = case["ref"]("ragged", 5, 1)
    got = _case_run(pkg, solver, case, "ragged", 5, 1)
    assert _same(ref, got, case["br"], case["po"]).all()


def test_gpu_with_gravity_gradient(pkg, ol, solver, case):
    """the 3U inertia under the orbit table of ``gg_common.orbit``, R = 3, latency 0, limits +-3; the torque shows on the reference
    (against gm = 0), so a kernel that dropped the rows cannot pass. The filter's model has no such term"""
    ref = case["ref"]("gravity", 3, 0)
    bg, es, n, rt, pl, sat = case["setups"]["gravity"]
    no_gm = mq.reference_loop(ol, bg, hc.solve_options(ol), n, 3, 1, case["po"], mc.SIGMAS, case["bias"], 0, pl, sat, hc.IDS,
                              Rtab=rt, gm=0.0, nthreads=8, filt=mq.FILT)
    mc.moved(ref, no_gm, "gravity gradient on against gm = 0")
    got = _case_run(pkg, solver, case, "gravity", 3, 0)
    assert _same(ref, got, bg, case["po"]).all()


def test_gpu_continuation_with_filt_init_equals_one_longer_run(pkg, solver, case):
    """6 + 6 steps with step0 = 6, no new upload and filt_init = the first call's filt_state at R = 3, latency 0, are the 12-step
    run, bit for bit, Y_hist and the records included; without filt_init the second call restarts the filter and its final state
    differs by >= gg_common.MOVED"""
    b = case["b"]
    whole = _case_run(pkg, solver, case, "saturated", 3, 0)
    whole.update(solver.download(want_K=False))
    kw = dict(sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=0, plant=case["plant"], sat=hc.SAT, noise_id=hc.IDS)
    first = _run(pkg, solver, b, 6, 3, case["po"], **kw)
    second = _run(pkg, solver, b, 6, 3, case["po"], step0=6, upload=False, filt_init=first["filt_state"], **kw)
    second.update(solver.download(want_K=False))
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(np.concatenate([first["Y_hist"], second["Y_hist"]], axis=1), whole["Y_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("stats", "X", "U", "filt_state", "filt_final"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)
    np.testing.assert_array_equal(second["X_hist"][:, 0], first["X_hist"][:, -1])
    _run(pkg, solver, b, 6, 3, case["po"], **kw)
    restarted = _run(pkg, solver, b, 6, 3, case["po"], step0=6, upload=False, **kw)
    d = float(np.max(np.abs(restarted["X_hist"][:, -1] - whole["X_hist"][:, -1])))
    print(f"without filt_init the continuation's final state differs from the longer run's by {d:.2e}")
    assert d >= gc.MOVED


def test_gpu_null_filter_is_the_sensed_call(pkg, solver, case):
    """f = NULL against ``receding_horizon_held_sensed``, bit for bit, with and without the gravity rows, latency 1"""
    po = case["po"]
    for b, rt, pl in ((case["b"], None, case["plant"]), (case["bg"], case["Rtab"], case["plant_g"])):
        kw = dict(sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=1, Rtab=rt, gm=gc.GM if rt is not None else 0.0, plant=pl,
                  sat=hc.SAT, noise_id=hc.IDS, noise_opts=po)
        prob = pkg.trajopt.BatchProblem.from_arrays(b)
        old = pkg.mpc.receding_horizon_held_sensed(prob, solver, N_STEPS, 3, **kw)
        old.update(solver.download(want_K=False))
        new = pkg.mpc.receding_horizon_held_model_mag_filtered(prob, solver, N_STEPS, 3, filter=None, **kw)
        new.update(solver.download(want_K=False))
        for k in KEYS + ("Y_hist", "X", "U"):
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)
        assert new["filt_state"] is None and new["filt_final"] is None


def test_gpu_wave_boundary_tiled_batch_is_the_individual_loops(pkg, ol, solver):
    """2 slews x 33 realisations through mpc.tile_realisations with per-realisation biases: T = 66, so the strides of the record and
    of the field's memory cross a wavefront (lane 63 -> 64 inside slew 1, two lanes in the last wavefront), horizons (20, 13), 6
    steps at R = 4 (4 + 2), latency 1; all 66 against one-trajectory reference loops"""
    M, n, R = 33, 6, 4
    b = mq.coarse_rows(pkg, hc.mpc_batch(pkg, T=2, N=20))
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
            ref = mq.reference_loop(ol, one_b, o, n, R, 1, po, mc.SIGMAS, sensor[t, m][None], 1, plant[t, m][None], hc.SAT,
                                    id0[t:t + 1] + m, nthreads=1, filt=mq.FILT)
            assert np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
            i = t * M + m
            _same(ref, {k: got[k][i:i + 1] for k in KEYS + EST}, one_b, po)


def test_gpu_one_step(pkg, ol, solver, case):
    """n_steps = 1: the pack's `first`, one block of one step, the closing predict — to the parity bars against the reference loop,
    and b^ = 0 exactly (no update was made), either latency"""
    b, po = case["b"], case["po"]
    for latency in (0, 1):
        ref = mq.reference_loop(ol, b, hc.solve_options(ol), 1, 3, 1, po, mc.SIGMAS, case["bias"], latency, case["plant"], hc.SAT, hc.IDS,
                                nthreads=8, filt=mq.FILT)
        got = _run(pkg, solver, b, 1, 3, po, sensor_opts=mc.SIGMAS, sensor=case["bias"], latency=latency, plant=case["plant"], sat=hc.SAT,
                   noise_id=hc.IDS)
        dX, dU = float(np.max(np.abs(ref["X_hist"] - got["X_hist"]))), float(np.max(np.abs(ref["U_hist"] - got["U_hist"])))
        print(f"latency {latency}: max|dX_hist| {dX:.2e}  max|dU_hist| {dU:.2e}")
        assert dX < 1e-9 and dU < 1e-8           # the MPC bars; two samples are fewer than the statistic's min_steps: nothing to judge
        assert np.all((ref["n_sure"] <= got["n_clipped"]) & (got["n_clipped"] <= ref["n_maybe"]))
        mq.same_estimates(ref, got)
        np.testing.assert_array_equal(got["filt_final"][:, 0:3], 0.0)
        np.testing.assert_array_equal(got["filt_state"][:, 10:13], got["U_hist"][:, 0])


def test_gpu_bad_arguments_are_codes_and_texts(pkg, ol, solver, case):
    lib, abi = pkg._abi.load(), pkg._abi
    b, po = case["b"], case["po"]
    init = np.tile(np.r_[1.0, np.zeros(57)], (8, 1))
    for kw, word in ((dict(filt=dict(mq.FILT, sigma_m=0.0)), "sigma_m must be > 0"),
                     (dict(filt=dict(mq.FILT, sigma_g=0.0)), "sigma_g must be > 0"),
                     (dict(filt=dict(mq.FILT, sigma_w=float("nan"))), "must be finite and >= 0"),
                     (dict(filt=None, filt_init=init), "must be NULL when f is NULL"),
                     (dict(sensor_opts=dict(sigma_gyro=-1.0)), "must be finite and >= 0"),
                     (dict(latency=2), "latency must be 0"),
                     (dict(gm=gc.GM), "Rtab may be NULL only with gm == 0"),
                     (dict(R=0), "replan_every must be >= 1"), (dict(R=20), "min n_knots - 1 = 19")):
        kw = dict(kw)
        with pytest.raises(RuntimeError, match=word):
            _run(pkg, solver, b, 8, kw.pop("R", 3), po, sat=hc.SAT, **kw)
    z = init.copy()
    z[5, 12] = np.inf
    with pytest.raises(RuntimeError, match="non-finite filt_init entry at t = 5"):
        _run(pkg, solver, b, 8, 3, po, sat=hc.SAT, filt_init=z)
    z = init.copy()
    z[6, 0] = 0.0
    with pytest.raises(RuntimeError, match="zero norm at t = 6"):
        _run(pkg, solver, b, 8, 3, po, sat=hc.SAT, filt_init=z)
    # reserved != 0, f NULL with an output array, NULL X_hist: through the C ABI; a rejected call grows no workspace
    o = solver.opts.to_abi(b.N, b.n_tab, 3)
    o.max_outer, o.max_inner = 1, 3
    so = sc.sensor_options(abi, mc.SIGMAS, 0)
    fo = mg.filter_options(abi, mq.FILT)
    fbad = mg.filter_options(abi, mq.FILT)
    fbad.reserved = 1
    Xh, Uh, fs = np.empty((8, 4, 7)), np.empty((8, 3, 3)), np.empty((8, 58))
    d = abi.as_dp
    before = lib.tsat_workspace_bytes(solver._h)
    head = (solver._h, C.byref(o), C.byref(po), 3, 0, 3, 1, None, None, None, None)
    mid = (None, None, None, None, None, 0.0, C.byref(so), None, None)
    assert lib.tsat_mpc_run_held_model_mag_filtered(*head, d(Xh), d(Uh), *mid, C.byref(fbad), None, None, None) == -1
    assert b"reserved must be 0" in lib.tsat_last_error(solver._h)
    assert lib.tsat_mpc_run_held_model_mag_filtered(*head, d(Xh), d(Uh), *mid, None, None, d(fs), None) == -1
    assert b"must be NULL when f is NULL" in lib.tsat_last_error(solver._h)
    assert lib.tsat_mpc_run_held_model_mag_filtered(*head, None, d(Uh), *mid, C.byref(fo), None, None, None) == -1
    assert b"null array" in lib.tsat_last_error(solver._h)
    assert lib.tsat_workspace_bytes(solver._h) == before
    # the handle is as good as before: tsat_mpc_run on it matches the oracle on a 3-step run
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    got = pkg.mpc.receding_horizon(prob, solver, 3, plant_integrator=4)
    ref = ol.mpc_batch(b, hc.solve_options(ol), 3, plant_integrator=4)
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-9 and np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
