"""GPU tier of tests/test_plant_mp.py: the tracking kernel on every run of tests/golden/plant_mp.npz against the 50-digit results
in the file (bars and the printed table: tests/plant_mp_common.py; E_ref is the oracle's error, measured here), and zero noise
levels at every closed-loop entry point. Reads the file and the oracle only; nothing here imports mpmath."""
import numpy as np
import pytest

import plant_mp_common as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


@pytest.mark.parametrize("name", pm.RUN_NAMES)
def test_gpu_tracking_kernel_against_50_digits(pkg, ol, solver, name):
    ora = pm.run_oracle(ol, pkg, name)
    got = pm.run_gpu(pkg, solver, name)
    pm.check_oracle(name, ora)
    pm.check_impl(name, got, [ora], "kernel")


def test_gpu_zero_noise_levels_tracking(pkg, solver):
    """tsat_tvlqr_batch: noise_mode = 1 with all three levels zero is the noise-free run; sigma_att = 0 alone is array mode fed
    generated_noise(..., sigma_att=0.0)"""
    pm.tvlqr_zero_sigma_checks(pkg, pkg._abi.TvlqrOptions, lambda n, o, nz: pm.run_gpu(pkg, solver, n, o, nz), "kernel")


@pytest.fixture(scope="module")
def ens(pkg):
    return pm.ensemble_case(pkg)


@pytest.mark.parametrize("entry", pm.ENSEMBLES)
def test_gpu_zero_noise_levels_ensembles(pkg, ol, solver, ens, entry):
    """the six TVLQR ensemble entry points (dispersed plants, gravity gradient, the sensors' own noise on): every plant level zero
    is finite and is the limit of a vanishing attitude level; the nominal ensemble with the model's plant is also the oracle's
    noise-free run of every realisation"""
    import sensed_common as sc

    o0, o1 = pm.level_options(pkg._abi.TvlqrOptions, ens["r"]), pm.level_options(pkg._abi.TvlqrOptions, ens["r"], pm.TINY_ATT)
    zero = pm.gpu_ensemble(pkg, solver, entry, ens, o0, sens=sc.SIGMAS)
    tiny = pm.gpu_ensemble(pkg, solver, entry, ens, o1, sens=sc.SIGMAS)
    nk = ens["b"]["n_knots"]
    pm.check_same_limit(zero, tiny, nk, f"tsat_tvlqr_ensemble_{entry}")
    if entry == "ensemble":
        sb, b, s = ens["sb"], ens["b"], pm.script()
        v = np.array(ens["r"]["opts"]); v[s.O_MODE] = 0
        free = [ol.tvlqr_batch(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], ens["x0"][:, m], opts=pm.fill_options(ol.tvlqr_default_options(), v))
                for m in range(ens["x0"].shape[1])]
        free = dict(X_sim=np.stack([f["X_sim"] for f in free], axis=1), stats=np.stack([f["stats"] for f in free], axis=1))
        d = float(np.max(np.abs(free["X_sim"] - zero["X_sim"])))
        print(f"tsat_tvlqr_ensemble, zero levels against the oracle's noise-free runs: |dX_sim| {d:.2e}")
        assert d < 1e-9 and np.array_equal(free["stats"]["slew_index"], zero["stats"]["slew_index"])      # the kernel-against-oracle bar
        assert np.array_equal(free["stats"]["failed"], zero["stats"]["failed"])


def test_gpu_zero_noise_levels_pd(pkg, ol, solver, ens):
    """tsat_pd_ensemble on the same plants under gravity gradient"""
    import pd_common as pc

    lib = pkg._abi.load()
    out = []
    for sa in (0.0, pm.TINY_ATT):
        call = pc.Call(pkg._abi, ens["sb"], pm.level_options(pkg._abi.TvlqrOptions, ens["r"], sa), ens["x0"], 10 * pc.KD, 10 * pc.KP, X=ens["b"]["X"],
                       U=ens["b"]["U"], plant=ens["plant"], Rtab=ens["Rtab"], gm=3.986004418e5)
        rc = lib.tsat_pd_ensemble(solver._h, *call.c_args())
        assert rc == 0, lib.tsat_ensemble_last_error().decode()
        out.append(call.result())
    pm.check_same_limit(out[0], out[1], ens["b"]["n_knots"], "tsat_pd_ensemble")


LOOPS = ("dispersed", "held", "held_sensed", "held_filtered")


@pytest.mark.parametrize("loop", LOOPS)
def test_gpu_zero_noise_levels_loops(pkg, solver, loop):
    """the receding-horizon loops, two control steps of 17-knot solves: generated noise with every plant level zero is the
    noise-free loop (tsat_mpc_run_dispersed, tsat_mpc_run_held; tsat_mpc_run, which has no noise, is the same history again), and
    with the sensors' own noise on (held_sensed, held_filtered) the limit of a vanishing attitude level"""
    import mpc_dispersed_common as mc
    import sensed_common as sc

    b = mc.mpc_batch(pkg, T=2, N=17)
    prob = pkg.trajopt.BatchProblem.from_arrays(b)
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    zero = dict(noise_seed=2019, sigma_gyro=0.0, sigma_att=0.0, field_amp=0.0)
    tiny = dict(zero, sigma_att=pm.TINY_ATT)
    m = pkg.mpc
    if loop == "dispersed":
        run = lambda po: m.receding_horizon_dispersed(prob, solver, 2, noise_opts=po)
    elif loop == "held":
        run = lambda po: m.receding_horizon_held(prob, solver, 2, 2, noise_opts=po)
    elif loop == "held_sensed":
        run = lambda po: m.receding_horizon_held_sensed(prob, solver, 2, 2, sensor_opts=sc.SIGMAS, noise_opts=po)
    else:
        run = lambda po: m.receding_horizon_held_filtered(prob, solver, 2, 2, filter=dict(sigma_v=5e-3, sigma_a=sc.SIGMAS["sigma_att"]),
                                                          sensor_opts=sc.SIGMAS, noise_opts=po)
    z = run(zero)
    measured = loop in ("held_sensed", "held_filtered")            # their sensor draws need the generator on: no noise-free run
    runs = [("a vanishing attitude level", run(tiny)) if measured else ("the noise-free loop", run(None))]
    if loop == "dispersed":
        runs.append(("tsat_mpc_run", m.receding_horizon(prob, solver, 2, plant_integrator=4)))
    assert np.all(np.isfinite(z["X_hist"])) and np.all(np.isfinite(z["U_hist"])), (loop, "zero noise levels give a non-finite history")
    bar = pm.FLOOR_ULPS * pm.ULP * float(np.max(np.abs(z["X_hist"]))) * 2
    for what, r in runs:
        d = float(np.max(np.abs(r["X_hist"] - z["X_hist"])))
        print(f"zero sigmas tsat_mpc_run_{loop} against {what}: |dX_hist| {d:.2e}, bar {bar:.2e}")
        assert d <= bar, (loop, what, d, bar)
        if "tracking_stats" in r:
            assert np.array_equal(r["tracking_stats"]["slew_index"], z["tracking_stats"]["slew_index"])
            assert np.array_equal(r["tracking_stats"]["failed"], z["tracking_stats"]["failed"])


def test_gpu_wrappers_with_sigma_scale_zero_are_finite(pkg, solver, ens):
    """"dispersion only": sigma_scale = 0 through the wrappers of tracking.py, which every one of them multiplies into sigma_att.
    (They keep the field noise, so the run is not the noise-free one; it was a batch of NaN.)"""
    import sensed_common as sc

    tr, sb, b = pkg.tracking, ens["sb"], ens["b"]
    head = (solver, sb, b["X"], b["U"], ens["x0"], b["Qd"], b["Qfd"], b["Rd"], 2019)
    kw = dict(sigma_scale=0.0, want_trajectories=True)
    res = {"ensemble": tr.attitude_ensemble(*head, **kw),
           "dispersed": tr.attitude_ensemble_dispersed(*head, ens["plant"], **kw),
           "gg": tr.attitude_ensemble_gg(*head, ens["plant"], ens["Rtab"], **kw),
           "sensed": tr.attitude_ensemble_sensed(*head, plant=ens["plant"], sigma_gyro=sc.SIGMAS["sigma_gyro"], sigma_att=sc.SIGMAS["sigma_att"], **kw),
           "filtered": tr.attitude_ensemble_filtered(*head, plant=ens["plant"], sigma_gyro=sc.SIGMAS["sigma_gyro"], sigma_att=sc.SIGMAS["sigma_att"], **kw),
           "pd": tr.attitude_ensemble_pd(solver, sb, ens["x0"], 2e-4, 4e-6, 2019, X=b["X"], plant=ens["plant"], **kw)}
    for name, r in res.items():
        assert np.all(np.isfinite(r["X_sim"])) and np.all(np.isfinite(r["stats"]["final_angle"])), name
