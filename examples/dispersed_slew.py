#!/usr/bin/env python3
"""The single slew of examples/ensemble_slew.py tracked under 256 DISPERSED PLANTS in one call.

    python examples/dispersed_slew.py            (needs an MI355X; ~1 s)

The noise of the reference's plant (src/simulator.jl) hardly decides whether a magnetorquer-only slew arrives; plant / model
mismatch does. Here the plan is solved once and its TVLQR gains are computed once from the MODEL inertia; then every one of
256 realisations flies a satellite of its own — principal moments off by 1 % (1 sigma), principal axes turned by 0.2 deg,
actuator gains off by 1 % behind a mounting misaligned by 0.5 deg, a residual dipole of 2e-4 A m^2 — under the feedback command
limited to the box the plan was solved in (tracking.attitude_ensemble_dispersed -> tsat_tvlqr_ensemble_dispersed). The summary
row is printed next to the one of the undispersed ensemble (tracking.attitude_ensemble)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import tracking, trajopt as to  # noqa: E402
from ensemble_slew import plan  # noqa: E402

LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)


def main(M=256, verbose=True):
    say = print if verbose else (lambda *a, **k: None)
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    ens = tracking.attitude_ensemble(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, noise_seed=1)
    dis = tracking.attitude_ensemble_dispersed(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant, sat=(b.ulo, b.uhi))
    say("summary row [M, failures, mean / min / max slew time of the arrivals, mean of all, max final angle, max final rate]:")
    say(f"  the model's plant:  {ens['summary'][0]}")
    say(f"  dispersed plants:   {dis['summary'][0]}")
    nc = dis["n_clipped"][0]
    say(f"{int(dis['summary'][0, 1])} of {M} dispersed realisations fail ({int(ens['summary'][0, 1])} of {M} on the model's plant); "
        f"the limit changed the command on {int(nc.min())} .. {int(nc.max())} of {N - 1} knots per realisation")
    solver.close()
    return dict(N=N, summary=dis["summary"][0], summary_nominal_plants=ens["summary"][0], n_clipped=nc, stats=dis["stats"][0])


if __name__ == "__main__":
    main()
