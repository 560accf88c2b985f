#!/usr/bin/env python3
"""The slew of examples/model_filtered_held_slew.py — same 256 dispersed plants, perturbed starts, generator ids and sensor —
RE-PLANNED FROM THE ESTIMATE OF THE FILTER THE SATELLITE COULD FLY: the nine-state model filter took the held loop's failures from
98 / 20 / 49 of 256 to 14 / 14 / 8, but it is updated by an attitude sensor that hands over a quaternion. Here that update is
replaced by a magnetometer update against the slew's field table, after ONE attitude fix at sample 0. Does the 14 / 14 / 8 survive?

    python examples/model_mag_filtered_held_slew.py [--out profiles/mpc/model_mag_filtered_failures.txt]   (needs an MI355X; some minutes)

Four columns, each at R = 1, 5 and 20 with the gains on:
  raw          mpc.receding_horizon_held_sensed on the 1 deg / 0.38 deg/s sensor of examples/sensed_held_slew.py
  model        mpc.receding_horizon_held_model_filtered at 10 x the measured sigma_w: the 14 / 14 / 8 of
               profiles/mpc/model_filtered_failures.txt
  mag 1 x      mpc.receding_horizon_held_model_mag_filtered (tsat_mpc_run_held_model_mag_filtered): the sensor's own gyro figure,
  mag 10 x     the magnetometer noise of examples/mag_filtered_slew.py, p0_att the accuracy of the one fix (1 deg), sigma_w = 1 x and
               10 x the un-modelled angular acceleration measured on these plants (5.2e-5 rad/s^2)
Printed per row: failures of 256 in each column, and the rms rate (rad/s) and attitude (deg) error of the x0 the solves started
from (Y_hist against X_hist at the block starts)."""
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
from mag_filtered_slew import SIGMA_MAG  # noqa: E402
from model_filtered_held_slew import SIGMA_W, x0_errors  # noqa: E402
from replanned_slew import longer_table  # noqa: E402
from sensed_held_slew import SENSOR  # noqa: E402

COLUMNS = ("raw", "model", "mag 1 x", "mag 10 x")


def main(M=256, intervals=(1, 5, 20), verbose=True, out=None):
    lines = []

    def say(line):
        if verbose:
            print(line, flush=True)
        lines.append(line)
        if out:                                    # line by line: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    sg, sa = tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT
    f9 = tracking.model_filter_options(10.0 * SIGMA_W, sg, sa)
    fm = {s: tracking.model_mag_filter_options(s * SIGMA_W, sg, SIGMA_MAG, p0_att=sa) for s in (1.0, 10.0)}
    sensor = dict(SENSOR, sigma_mag=SIGMA_MAG)
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each, sensor 0.38 deg/s gyro, 1 deg attitude and {SIGMA_MAG:g} T magnetometer "
        f"noise; gains on; per column: failures of {M} [rms rate error rad/s, rms attitude error deg of the x0 at block starts]; "
        f"sigma_w = {SIGMA_W:.1e} rad/s^2; the mag columns read the attitude sensor at sample 0 only")
    # the loop of examples/sensed_held_slew.py: the same slew M times, every realisation from its own perturbed start
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    kw = dict(kw, noise_opts=dict(noise_seed=1), sensor_opts=sensor)
    fly = {
        "raw": lambda R: mpc.receding_horizon_held_sensed(prob, solver, N - 1, R, **kw),
        "model": lambda R: mpc.receding_horizon_held_model_filtered(prob, solver, N - 1, R, filter=f9, **kw),
        "mag 1 x": lambda R: mpc.receding_horizon_held_model_mag_filtered(prob, solver, N - 1, R, filter=fm[1.0], **kw),
        "mag 10 x": lambda R: mpc.receding_horizon_held_model_mag_filtered(prob, solver, N - 1, R, filter=fm[10.0], **kw),
    }
    result = dict(N=N)
    for R in intervals:
        cells = []
        for col in COLUMNS:
            r = fly[col](R)
            dw, da = x0_errors(r, R)
            result[(R, col)] = r["tracking_stats"]
            cells.append(f"{col}: {fails(r['tracking_stats']):3d} [{dw:.2e}, {da:.3f}]")
            if col.startswith("mag"):
                ms = r["ms"] / (N - 1)
        say(f"  R = {R:2d}:   " + "   ".join(cells) + f"   ({ms:.2f} ms per step behind this filter)")
    solver.close()
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(out=ap.parse_args().out)
