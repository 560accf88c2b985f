#!/usr/bin/env python3
"""The single slew of examples/dispersed_slew.py under the same 256 dispersed plants, TRACKED and RE-PLANNED side by side.

    python examples/replanned_slew.py            (needs an MI355X; a few seconds)

examples/dispersed_slew.py shows that fixed TVLQR gains around a plan made for the model's satellite do not survive plant / model
mismatch. The obvious reply is to re-plan: here every one of the 256 realisations — same inertia, actuator matrix and residual
dipole, same perturbed start, same noise draws — also flies the receding-horizon loop (mpc.receding_horizon_dispersed ->
tsat_mpc_run_dispersed): the plan's horizon re-solved every control step from the state the dispersed plant actually reached
(1 x 3 budget, warm start = the previous plan shifted by one knot), its first control limited to the plan's box. Failures and the
slew-time spread of both are printed next to each other."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import horizon, magnetic, mpc, tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402


def longer_table(solver, N):
    """the field table of ensemble_slew.plan continued for a second horizon (same orbit, same row step): the loop's clock runs on"""
    kep = np.array([[0.0, 400.0 + 6371.0, 51.6, 0.0, 0.0, 90.0]])
    t0, tf, N_tab, cutoff, dt = 0.0, 5400.0, 5000, 20.0, 0.2
    B_coarse, _ = magnetic.magnetic_simulation(solver, kep, t0, tf, N_tab)
    idx, _ = horizon.condition_based_time(solver, B_coarse, (tf - t0) / N_tab, cutoff)
    t_final, n = horizon.knots_from_index(idx, tf - t0, N_tab, dt=dt)
    assert int(n[0]) == N
    B, _ = magnetic.magnetic_simulation(solver, kep, t0, 2.0 * float(t_final[0]), 2 * N)
    return B


def spread(st):
    ok = st["slew_time"][st["failed"] == 0]
    return "no arrivals" if ok.size == 0 else f"slew time {ok.mean():.1f} s on average ({ok.min():.1f} .. {ok.max():.1f} s)"


def main(M=256, verbose=True):
    say = print if verbose else (lambda *a, **k: None)
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    tv = tracking.attitude_ensemble_dispersed(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant, sat=(b.ulo, b.uhi))
    # the loop: the same slew M times, every realisation from its own perturbed start, warm-started with the plan
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    rh = mpc.receding_horizon_dispersed(prob, solver, N - 1, noise_opts=dict(noise_seed=1), **kw)
    solver.close()
    st_tv, st_rh = tv["stats"][0], rh["tracking_stats"]
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each:")
    say(f"  TVLQR tracking of the plan:   {int(np.count_nonzero(st_tv['failed']))} of {M} fail; {spread(st_tv)}")
    say(f"  receding-horizon re-planning: {int(np.count_nonzero(st_rh['failed']))} of {M} fail; {spread(st_rh)}"
        f"   ({rh['ms'] / (N - 1):.2f} ms per control step for the {M} re-solves)")
    say(f"  median final error angle: tracking {np.median(st_tv['final_angle']):.4f} rad, re-planning {np.median(st_rh['final_angle']):.4f} rad; "
        f"the limit changed the command on {int(rh['n_clipped'].min())} .. {int(rh['n_clipped'].max())} of {N - 1} steps of the loop")
    return dict(N=N, tracking=st_tv, replanned=st_rh, n_clipped=rh["n_clipped"], ms=rh["ms"])


if __name__ == "__main__":
    main()
