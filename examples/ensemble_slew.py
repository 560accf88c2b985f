#!/usr/bin/env python3
"""The single slew of examples/single_slew.py tracked under 256 realisations of the plant noise in one call.

    python examples/ensemble_slew.py            (needs an MI355X; ~1 s)

The reference's Monte-Carlo draws ONE noise realisation per planned slew (src/monte_carlo.jl:199-262). Here the plan is solved
once (as in single_slew.py, src/TortoiseSat.jl:34-199), its TVLQR gains are computed once, and 256 noisy plants are simulated
side by side — one per GPU lane — which gives the failure probability and the slew-time spread of the plan
(tracking.attitude_ensemble -> tsat_tvlqr_ensemble)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import horizon, magnetic, slew_setup as ss, tracking, trajopt as to  # noqa: E402


def plan(solver, say=print, J=None):
    """the plan: examples/single_slew.py, line for line (J: another inertia than its 1P preset). Returns (batch, res, N)."""
    kep = np.array([[0.0, 400.0 + 6371.0, 51.6, 0.0, 0.0, 90.0]])
    t0, tf, N_tab, cutoff, dt = 0.0, 5400.0, 5000, 20.0, 0.2
    B_coarse, _ = magnetic.magnetic_simulation(solver, kep, t0, tf, N_tab)
    idx, _ = horizon.condition_based_time(solver, B_coarse, (tf - t0) / N_tab, cutoff)
    t_final, N = horizon.knots_from_index(idx, tf - t0, N_tab, dt=dt)
    t_final, N = float(t_final[0]), int(N[0])
    B_ECI, _ = magnetic.magnetic_simulation(solver, kep, t0, t_final, N)
    n, m = 8, 3
    J = ss.INERTIA["1P"] if J is None else J
    x0 = np.r_[0.0, 0.0, 0.0, ss.axis_angle_quat([1.0, 0.0, 1.0], np.deg2rad(90.0)), 0.0]
    xf = np.r_[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    model_d = to.rk3(to.Model(to.DerivFunction(J, B_ECI[0]), n, m))
    w_guess, _ = ss.eigen_axis_slew(x0[:7], xf[:7], dt * np.arange(N + 1))
    Qd, Qfd, Rd = ss.bryson_weights(w_guess, J, dt, 10.0, 1.0e3)
    Q = np.zeros((n, n)); Qf = np.zeros((n, n))
    Q[:7, :7], Qf[:7, :7] = np.diag(Qd), np.diag(Qfd)
    constraints = to.Constraints(N)
    for k in range(1, N):
        constraints[k] += to.BoundConstraint(n, m, u_max=1, u_min=-1)
    constraints[N] += to.goal_constraint(xf)
    sat = to.Problem(model_d, to.LQRObjective(Q, np.diag(Rd), Qf, xf, N), constraints=constraints, x0=x0, xf=xf, N=N, dt=dt)
    to.initial_controls_(sat, np.zeros((m, N + 1)))
    opts_al = to.AugmentedLagrangianSolverOptions()
    opts_al.opts_uncon.iterations, opts_al.iterations = 50, 20
    solver.opts = opts_al
    batch = to.BatchProblem([sat])
    res = to.solve_(batch, solver)
    say(f"plan: {N} knots of {dt} s, status {sat.stats['status']}, max violation {sat.stats['c_max']:.2e}")
    return batch, res, N


def main(M=256, sigma_scale=1.0, verbose=True):
    say = print if verbose else (lambda *a, **k: None)
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    # the ensemble ------------------------------------------------------------------------------------------------
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(batch.arrays.x0, M, np.random.default_rng(0))
    ens = tracking.attitude_ensemble(solver, batch.arrays, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, noise_seed=1, sigma_scale=sigma_scale)
    s, nom = ens["summary"][0], ens["nominal"][0]
    say(f"summary row [M, failures, mean / min / max slew time of the arrivals, mean of all, max final angle, max final rate]:\n  {s}")
    say(f"{int(s[1])} of {int(s[0])} realisations fail; slew time {s[2]:.1f} s on average ({s[3]:.1f} .. {s[4]:.1f} s), "
        f"noise-free plant from the plan's own start: {'fails' if nom['failed'] else format(nom['slew_time'], '.1f') + ' s'}")
    solver.close()
    return dict(N=N, summary=s, nominal=nom, stats=ens["stats"][0])


if __name__ == "__main__":
    main()
