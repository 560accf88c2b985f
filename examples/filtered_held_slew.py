#!/usr/bin/env python3
"""The slew of examples/sensed_held_slew.py — same 256 dispersed plants, perturbed starts, generator ids and sensor — RE-PLANNED
FROM THE FILTER'S ESTIMATE: every block solve of the held loop starts from one raw 1 deg / 0.38 deg/s sample, and a 1 deg attitude
error in that x0 becomes a plan. Does the multiplicative EKF between sensor and solver pay there, and at which re-plan interval R?

    python examples/filtered_held_slew.py [--out profiles/mpc/filtered_failures.txt]       (needs an MI355X; some ten seconds)

Here the sensor of examples/sensed_held_slew.py (sigma_gyro = 0.38 pi / 180 rad/s, sigma_att = pi / 180 rad, no biases) is read raw
through mpc.receding_horizon_held_sensed and through the filter of examples/filtered_slew.py — the library's default figures, which
are the sensor's own — by mpc.receding_horizon_held_filtered (tsat_mpc_run_held_filtered): R = 1, 5 and 20, the gains on and off.
Printed: failures of 256, raw against filtered, and the filter's own last standard deviations."""
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
from sensed_held_slew import SENSOR  # noqa: E402


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
    filt = tracking.filter_options(tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each, sensor 0.38 deg/s gyro and 1 deg attitude noise; failures of {M}:")
    # the loop of examples/sensed_held_slew.py: the same slew M times, every realisation from its own perturbed start
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    result = dict(N=N)
    for R in intervals:
        for fb in (True, False):
            raw = mpc.receding_horizon_held_sensed(prob, solver, N - 1, R, sensor_opts=SENSOR, feedback=fb, noise_opts=dict(noise_seed=1), **kw)
            est = mpc.receding_horizon_held_filtered(prob, solver, N - 1, R, filter=filt, sensor_opts=SENSOR, feedback=fb,
                                                     noise_opts=dict(noise_seed=1), **kw)
            result[(R, fb, "raw")], result[(R, fb, "filtered")] = raw["tracking_stats"], est["tracking_stats"]
            sd = np.degrees(np.median(est["filt_final"][:, 3:6]))
            say(f"  re-planned every R = {R:2d} steps ({raw['n_solves']:4d} solves), gains {'on ' if fb else 'off'}   "
                f"raw: {fails(raw['tracking_stats']):3d} of {M} fail ({raw['ms'] / (N - 1):.2f} ms per step)   "
                f"filtered: {fails(est['tracking_stats']):3d} of {M} fail ({est['ms'] / (N - 1):.2f} ms per step; "
                f"the filter's last attitude sigma {sd:.2f} deg)")
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
