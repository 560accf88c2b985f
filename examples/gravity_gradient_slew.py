#!/usr/bin/env python3
"""The single slew of examples/dispersed_slew.py flown by a 3U satellite under 256 dispersed plants, WITH AND WITHOUT GRAVITY-GRADIENT
TORQUE, tracked and re-planned every tenth step.

    python examples/gravity_gradient_slew.py            (needs an MI355X; a few seconds)

Every plant of the other examples feels one torque, m x B. In a 400 km orbit an elongated body also feels the gravity gradient:
3 GM / r^3 = 3.85e-6 s^-2 times the difference of its moments of inertia — for the reference's 3U preset a fifth of what the
magnetorquers of this slew can produce, and ten times what the residual dipole of the dispersed plants adds. Neither the plan nor
the gains know of it. Here the same 256 realisations — inertia, actuator matrix, residual dipole, perturbed start, noise draws —
fly the plan under TVLQR tracking (tracking.attitude_ensemble_gg -> tsat_tvlqr_ensemble_gg) and under the loop that re-plans every
10 control steps with the solver's gains in between (mpc.receding_horizon_held_gg -> tsat_mpc_run_held_gg), once with gm = 0 and
once with the Earth's; the orbit positions are those the field table was evaluated at (magnetic.orbit_rows)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import horizon, magnetic, mpc, slew_setup as ss, tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from replanned_slew import spread  # noqa: E402

R_HOLD = 10


def tables(solver, N):
    """field rows and orbit positions of ensemble_slew.plan over its horizon and over two horizons (same orbit, same row step)"""
    kep = np.array([[0.0, 400.0 + 6371.0, 51.6, 0.0, 0.0, 90.0]])
    t0, tf, N_tab, cutoff, dt = 0.0, 5400.0, 5000, 20.0, 0.2
    B_coarse, _ = magnetic.magnetic_simulation(solver, kep, t0, tf, N_tab)
    idx, _ = horizon.condition_based_time(solver, B_coarse, (tf - t0) / N_tab, cutoff)
    t_final, n = horizon.knots_from_index(idx, tf - t0, N_tab, dt=dt)
    assert int(n[0]) == N
    _, pos = magnetic.magnetic_simulation(solver, kep, t0, float(t_final[0]), N)
    B2, pos2 = magnetic.magnetic_simulation(solver, kep, t0, 2.0 * float(t_final[0]), 2 * N)
    return pos, B2, pos2


def main(M=256, verbose=True):
    say = print if verbose else (lambda *a, **k: None)
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say, J=ss.INERTIA["3U"])
    b = batch.arrays
    pos, B2, pos2 = tables(solver, N)
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    # the loop's batch: the same slew M times on a table of two horizons, warm-started with the plan
    ext = b.slice(0, 1)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B2), B2.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    R1, R2 = magnetic.orbit_rows(pos, b.n_tab), magnetic.orbit_rows(pos2, ext.n_tab)
    out = {}
    say(f"{M} dispersed plants around the 3U inertia, {N} samples of {b.dt[0]} s each:")
    for label, gm in (("m x B alone", 0.0), ("with gravity gradient", tracking.GM_EARTH)):
        tv = tracking.attitude_ensemble_gg(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant, R1, gm, sat=(b.ulo, b.uhi))
        rh = mpc.receding_horizon_held_gg(prob, solver, N - 1, R_HOLD, R2, gm, noise_opts=dict(noise_seed=1), **kw)
        st_tv, st_rh = tv["stats"][0], rh["tracking_stats"]
        say(f"  {label}:")
        say(f"    TVLQR tracking of the plan:        {int(np.count_nonzero(st_tv['failed']))} of {M} fail; {spread(st_tv)}; "
            f"median final error angle {np.median(st_tv['final_angle']):.4f} rad")
        say(f"    re-planned every {R_HOLD} steps, gains on: {int(np.count_nonzero(st_rh['failed']))} of {M} fail; {spread(st_rh)}; "
            f"median final error angle {np.median(st_rh['final_angle']):.4f} rad   ({rh['ms'] / (N - 1):.2f} ms per control step)")
        out[label] = dict(tracking=st_tv, held=st_rh, ms=rh["ms"])
    solver.close()
    return dict(N=N, **out)


if __name__ == "__main__":
    main()
