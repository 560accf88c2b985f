#!/usr/bin/env python3
"""The slew of examples/replanned_slew.py under the same 256 dispersed plants, RE-PLANNED EVERY R CONTROL STEPS.

    python examples/held_slew.py            (needs an MI355X; some ten seconds)

examples/replanned_slew.py re-solves the horizon at every control step. A magnetorquer-only satellite would re-plan at a low rate
and apply feedback around the current plan at the control rate: here every realisation — same plants, perturbed starts and noise
draws — flies mpc.receding_horizon_held (tsat_mpc_run_held) at a sweep of re-plan intervals R, once with the solver's own gains
around the plan between two solves and once holding the plan's controls open loop. Failures and the mean slew time of the arrivals
are printed per R; R = 1 is the loop of examples/replanned_slew.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import mpc, tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from replanned_slew import longer_table  # noqa: E402


def main(M=256, intervals=(1, 2, 5, 10, 20, 50), verbose=True):
    say = print if verbose else (lambda *a, **k: None)
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    # the loop of examples/replanned_slew.py: the same slew M times, every realisation from its own perturbed start
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; re-planned every R control steps:")
    out = {}
    for R in intervals:
        row = []
        for fb in (True, False):
            r = mpc.receding_horizon_held(prob, solver, N - 1, R, feedback=fb, noise_opts=dict(noise_seed=1), **kw)
            st = r["tracking_stats"]
            ok = st["slew_time"][st["failed"] == 0]
            out[(R, fb)] = st
            row.append(f"gains {'on ' if fb else 'off'}: {int(np.count_nonzero(st['failed'])):3d} of {M} fail, "
                       + (f"mean slew time {ok.mean():6.1f} s" if ok.size else "no arrivals        ")
                       + f" ({r['ms'] / (N - 1):.2f} ms per step)")
        say(f"  R = {R:3d} ({r['n_solves']:4d} solves)   " + "   ".join(row))
    solver.close()
    return out


if __name__ == "__main__":
    main()
