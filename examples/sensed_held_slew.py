#!/usr/bin/env python3
"""The slew of examples/held_slew.py — same 256 dispersed plants, perturbed starts and generator ids — RE-PLANNED FROM MEASUREMENTS:
does re-planning still arrive where tracking fails, when each re-solve starts from a 1 deg / 0.38 deg/s measurement and not from
the truth, and how does that depend on the re-plan interval R?

    python examples/sensed_held_slew.py [--out profiles/mpc/sensed_failures.txt]       (needs an MI355X; some ten seconds)

examples/held_slew.py re-plans every R control steps from the plant's true state and flies the solver's gains on it in between.
Here both read the sensor of examples/sensed_slew.py — the reference's noise figures (src/simulator.jl:5,10) UN-SQUARED,
sigma_gyro = 0.38 pi / 180 rad/s on the measured rate and sigma_att = pi / 180 rad on the measured attitude, no biases —
through mpc.receding_horizon_held_sensed (tsat_mpc_run_held_sensed): R = 1, 5 and 20, the gains on and off, each with the ideal
sensor and with the sensor. Printed: failures of 256, next to the sensed TVLQR ensemble (tracking.attitude_ensemble_sensed) on the
same plants, starts and ids."""
import argparse
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

SENSOR = dict(sigma_gyro=tracking.SENSOR_SIGMA_GYRO, sigma_att=tracking.SENSOR_SIGMA_ATT)
SETTINGS = (("ideal sensor", None), ("0.38 deg/s gyro, 1 deg attitude noise", SENSOR))


def main(M=256, intervals=(1, 5, 20), verbose=True, out=None):
    lines = []

    def say(line):
        if verbose:
            print(line, flush=True)
        lines.append(line)

    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; failures of {M}:")
    # the sensed TVLQR ensemble of examples/sensed_slew.py on the same plants, starts and ids (id0 = 0)
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    result = dict(N=N)
    for label, sens in SETTINGS:
        r = tracking.attitude_ensemble_sensed(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant=plant, sat=(b.ulo, b.uhi),
                                              **(sens or {}))
        result[("tvlqr", label)] = r["stats"][0]
        say(f"  TVLQR tracking of the plan, {label}: {fails(r['stats'][0])} of {M} fail")
    # the loop of examples/held_slew.py: the same slew M times, every realisation from its own perturbed start
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    for R in intervals:
        for fb in (True, False):
            row = []
            for label, sens in SETTINGS:
                r = mpc.receding_horizon_held_sensed(prob, solver, N - 1, R, sensor_opts=sens, feedback=fb, noise_opts=dict(noise_seed=1), **kw)
                st = r["tracking_stats"]
                result[(R, fb, label)] = st
                row.append(f"{label}: {fails(st):3d} of {M} fail ({r['ms'] / (N - 1):.2f} ms per step)")
            say(f"  re-planned every R = {R:2d} steps ({r['n_solves']:4d} solves), gains {'on ' if fb else 'off'}   " + "   ".join(row))
    solver.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(out=ap.parse_args().out)
