#!/usr/bin/env python3
"""The slew of examples/filtered_held_slew.py — same 256 dispersed plants, perturbed starts, generator ids and sensor — RE-PLANNED
FROM THE NINE-STATE FILTER'S ESTIMATE: the six-state filter left the held loop's failures where they were, and the rate in every x0
it hands a solve is still one gyro sample. Is that gyro noise in x0 what makes the held loop fail?

    python examples/model_filtered_held_slew.py [--out profiles/mpc/model_filtered_failures.txt]   (needs an MI355X; some minutes)

Five columns, each at R = 1, 5 and 20 with the gains on and off (a block of one step has no held step, so at R = 1 the gains
cannot act and that row is flown once):
  raw          mpc.receding_horizon_held_sensed on the 1 deg / 0.38 deg/s sensor of examples/sensed_held_slew.py
  six-state    mpc.receding_horizon_held_filtered, the filter of examples/filtered_held_slew.py
  model 1 x    mpc.receding_horizon_held_model_filtered (tsat_mpc_run_held_model_filtered) at the sensor's own figures and
  model 10 x   sigma_w = 1 x and 10 x the un-modelled angular acceleration measured on these plants by
               examples/model_filtered_slew.py (5.2e-5 rad/s^2)
  no gyro      the raw loop with sigma_gyro = 0 in the sensor: the run that says whether the gyro noise is the cause
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
from replanned_slew import longer_table  # noqa: E402
from sensed_held_slew import SENSOR  # noqa: E402

SIGMA_W = 5.2e-5        # rad/s^2: profiles/ensemble/model_filtered_failures.txt
COLUMNS = ("raw", "six-state", "model 1 x", "model 10 x", "no gyro")


def x0_errors(r, R):
    """rms over realisations and block starts of |w_x0 - w| (rad/s) and of the angle between q_x0 and q (deg)"""
    y, x = r["Y_hist"][:, ::R], r["X_hist"][:, :-1][:, ::R]
    dw = np.sqrt(np.mean(np.sum((y[..., 0:3] - x[..., 0:3]) ** 2, axis=-1)))
    c = np.abs(np.sum(y[..., 3:7] * x[..., 3:7], axis=-1)) / (np.linalg.norm(y[..., 3:7], axis=-1) * np.linalg.norm(x[..., 3:7], axis=-1))
    ang = np.sqrt(np.mean((2.0 * np.arccos(np.minimum(c, 1.0))) ** 2))
    return float(dw), float(np.degrees(ang))


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
    f6 = tracking.filter_options(tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
    f9 = {s: tracking.model_filter_options(s * SIGMA_W, tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT) for s in (1.0, 10.0)}
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each, sensor 0.38 deg/s gyro and 1 deg attitude noise; per column: failures "
        f"of {M} [rms rate error rad/s, rms attitude error deg of the x0 at block starts]; sigma_w = {SIGMA_W:.1e} rad/s^2")
    # the loop of examples/sensed_held_slew.py: the same slew M times, every realisation from its own perturbed start
    ext = b.slice(0, 1)
    B = longer_table(solver, N)
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B), B.shape[1], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plant, noise_id0=np.zeros(1, dtype=np.int64), sat=(b.ulo, b.uhi))
    tiled.x0 = np.ascontiguousarray(x0_lqr[0])
    prob = to.BatchProblem.from_arrays(tiled, batch.integrator, batch.terminal_mask, batch.error_state)
    kw = dict(kw, noise_opts=dict(noise_seed=1))
    no_gyro = dict(SENSOR, sigma_gyro=0.0)
    fly = {
        "raw": lambda R, fb: mpc.receding_horizon_held_sensed(prob, solver, N - 1, R, sensor_opts=SENSOR, feedback=fb, **kw),
        "six-state": lambda R, fb: mpc.receding_horizon_held_filtered(prob, solver, N - 1, R, filter=f6, sensor_opts=SENSOR, feedback=fb, **kw),
        "model 1 x": lambda R, fb: mpc.receding_horizon_held_model_filtered(prob, solver, N - 1, R, filter=f9[1.0], sensor_opts=SENSOR,
                                                                            feedback=fb, **kw),
        "model 10 x": lambda R, fb: mpc.receding_horizon_held_model_filtered(prob, solver, N - 1, R, filter=f9[10.0], sensor_opts=SENSOR,
                                                                             feedback=fb, **kw),
        "no gyro": lambda R, fb: mpc.receding_horizon_held_sensed(prob, solver, N - 1, R, sensor_opts=no_gyro, feedback=fb, **kw),
    }
    result = dict(N=N)
    for R in intervals:
        for fb in ((True,) if R == 1 else (True, False)):
            cells = []
            for col in COLUMNS:
                r = fly[col](R, fb)
                dw, da = x0_errors(r, R)
                result[(R, fb, col)] = r["tracking_stats"]
                cells.append(f"{col}: {fails(r['tracking_stats']):3d} [{dw:.2e}, {da:.3f}]")
                if col.startswith("model"):
                    ms = r["ms"] / (N - 1)
            say(f"  R = {R:2d}, gains {'on or off' if R == 1 else ('on ' if fb else 'off')}:   " + "   ".join(cells) + f"   ({ms:.2f} ms per step behind the model filter)")
    solver.close()
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(out=ap.parse_args().out)
