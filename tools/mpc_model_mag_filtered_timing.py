"""Developer tool: what replacing the attitude update of the nine-state filter by the magnetometer's costs in the held re-planning
loop: tsat_mpc_run_held_model_mag_filtered next to its parent tsat_mpc_run_held_model_filtered, in the same run.
  The shape, dispersions, noise, limits and sensor of tools/mpc_model_filtered_timing.py (4096 trajectories x 200-knot horizon, 200
  control steps, 1 x 3 budget, half the plan's box as limits; the reference's un-squared sensor figures, biases of
  tracking.disperse_sensor, latency 1 — the prediction across the delay and the field's one-sample memory live):
  `mpc.receding_horizon_held_model_filtered` (sigma_w = 5.2e-4 rad/s^2) and `mpc.receding_horizon_held_model_mag_filtered` (the same
  figures, sigma_m = the sensor's 5e-7 T, p0_att the attitude sensor's 1 deg) at R in --intervals, gains on. One warm-up of every
  configuration, then `--rounds` rounds alternating the two loops at each R in one process; HIP-event time of the whole loop per
  control step: medians, min, max, and the run-to-run spread (max - min) / median of each loop beside the ratio. There is no bar on
  the ratio: the parent of the same run is the yardstick and the measured ratio is what is written. The two loops solve different
  problems after step 0 (their estimates differ), so the solves' own time may differ: the executed counts of tsat_mpc_tally are
  printed beside each pair.
Everything goes to stdout and, line by line, to `--out`."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from tsat_loader import load_package

pkg = load_package()
if os.environ.get("TSAT_LIB"):            # developer switch: another build of the same library (tools/alternate_builds.py)
    pkg._abi.LIB_NAME = os.environ["TSAT_LIB"]
from tortoisesat_jl_amd import mpc, slew_setup as ss, tracking as tr, trajopt as to

ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=4096)
ap.add_argument("--N", type=int, default=200)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--intervals", type=int, nargs="+", default=[1, 5, 20])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc", "model_mag_filtered_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
BIAS = dict(gyro_bias=1.5e-3, att_bias_deg=0.7)
SIGMA_MAG = 5e-7
SEED = 2019
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
s.opts.opts_uncon.dJ_counter_limit = 1
T, N, steps = args.T, args.N, args.steps
b = ss.workload_monte_carlo(T=T, N=N, seed=20190602)
B = ss.dipole_btable(steps + N + 8, 0.2, 6771.0, 96.6)
b.Btab, b.n_tab = np.ascontiguousarray(B[None]), B.shape[0]
b.dtau[:] = 1.0
prob = to.BatchProblem.from_arrays(b)
plant = np.ascontiguousarray(tr.disperse_plant(b.Jmat, 1, np.random.default_rng(7), **LEVELS)[:, 0])
sensor = np.ascontiguousarray(tr.disperse_sensor(T, 1, np.random.default_rng(11), **BIAS)[:, 0])
kw1 = dict(plant=plant, sat=(0.5 * b.ulo, 0.5 * b.uhi), noise_opts=dict(noise_seed=SEED))
sens = dict(sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=SIGMA_MAG)
mfilt = tr.model_filter_options(5.2e-4, tr.SENSOR_SIGMA_GYRO, tr.SENSOR_SIGMA_ATT, sigma_u=1e-5, p0_bias=BIAS["gyro_bias"])
gfilt = tr.model_mag_filter_options(5.2e-4, tr.SENSOR_SIGMA_GYRO, SIGMA_MAG, sigma_u=1e-5, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=BIAS["gyro_bias"])
lib = pkg._abi.load()


def tally():
    t = np.zeros((T, 4), dtype=np.int64)
    assert lib.tsat_mpc_tally(s._h, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return t.sum(axis=0)


def parent_loop(R, n=steps):
    r = mpc.receding_horizon_held_model_filtered(prob, s, n, R, filter=mfilt, sensor_opts=sens, sensor=sensor, latency=1, **kw1)
    r["tally"] = tally()
    return r


def this_loop(R, n=steps):
    r = mpc.receding_horizon_held_model_mag_filtered(prob, s, n, R, filter=gfilt, sensor_opts=sens, sensor=sensor, latency=1, **kw1)
    r["tally"] = tally()
    return r


for R in args.intervals:                                 # warm-up of every configuration
    parent_loop(R, max(5, R + 1))
    this_loop(R, max(5, R + 1))
S, F = {R: [] for R in args.intervals}, {R: [] for R in args.intervals}
for _ in range(args.rounds):
    for R in args.intervals:
        S[R].append(parent_loop(R))
        F[R].append(this_loop(R))
per = lambda runs: np.array([r["ms"] for r in runs]) / steps
spread = lambda v: float((v.max() - v.min()) / np.median(v))
fmt = lambda v: f"median {np.median(v):.4f} ms (min {v.min():.4f}, max {v.max():.4f}, spread {spread(v):.4f})"
say(f"held loop behind the magnetometer-updated nine-state filter against the held loop behind the attitude-updated one: {T} trajectories x {N}-knot horizon, {steps} control steps, "
    f"1 x 3 budget, 5 dispersions, noise, limits, gains on; sensor 0.38 deg/s, 1 deg, {SIGMA_MAG:g} T, biases, latency 1; {args.rounds} alternating rounds "
    f"after a warm-up; device time of the loop per control step (HIP events); spread = (max - min) / median over the rounds")
for R in args.intervals:
    ms, mf = per(S[R]), per(F[R])
    ratio = float(np.median(mf) / np.median(ms))
    say(f"R = {R:2d} ({S[R][-1]['n_solves']:3d} solves)  tsat_mpc_run_held_model_filtered:     {fmt(ms)}   [backward, forward, dual, inner] {S[R][-1]['tally'].tolist()}")
    say(f"                      tsat_mpc_run_held_model_mag_filtered: {fmt(mf)}   [backward, forward, dual, inner] {F[R][-1]['tally'].tolist()}")
    say(f"                      {ratio:.4f} x the parent loop's time; run-to-run spread {spread(ms):.4f} (parent), {spread(mf):.4f} (this loop)")
s.close()
