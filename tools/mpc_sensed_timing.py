"""Developer tool: what feeding the held re-planning loop measurements (tsat_mpc_run_held_sensed) costs next to the held loop on
the true state (tsat_mpc_run_held), in the same run.
  The shape, dispersions, noise and limits of tools/mpc_held_timing.py part 1 (4096 trajectories x 200-knot horizon, 200 control
  steps, 1 x 3 budget, half the plan's box as limits): `mpc.receding_horizon_held` and `mpc.receding_horizon_held_sensed` (the
  reference's un-squared sensor figures, biases of tracking.disperse_sensor, latency 1 — every path of the sensor live) at R in
  --intervals, gains on. One warm-up of every configuration, then `--rounds` rounds alternating the two loops at each R in one
  process; HIP-event time of the whole loop per control step: medians, min, max. The two loops solve different problems after
  step 0 (the sensed one starts its solves from measurements), so the solves' own time may differ: the executed counts of
  tsat_mpc_tally are printed beside each pair.
Kernel times come from a separate run of this tool under `rocprofv3 --kernel-trace --stats` (tools/README.md).
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc", "sensed_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
BIAS = dict(gyro_bias=1.5e-3, att_bias_deg=0.7)
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
sens = dict(sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT)
lib = pkg._abi.load()


def tally():
    t = np.zeros((T, 4), dtype=np.int64)
    assert lib.tsat_mpc_tally(s._h, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return t.sum(axis=0)


def held(R, n=steps):
    r = mpc.receding_horizon_held(prob, s, n, R, **kw1)
    r["tally"] = tally()
    return r


def sensed(R, n=steps):
    r = mpc.receding_horizon_held_sensed(prob, s, n, R, sensor_opts=sens, sensor=sensor, latency=1, **kw1)
    r["tally"] = tally()
    return r


for R in args.intervals:                                 # warm-up of every configuration
    held(R, max(5, R + 1))
    sensed(R, max(5, R + 1))
H, S = {R: [] for R in args.intervals}, {R: [] for R in args.intervals}
for _ in range(args.rounds):
    for R in args.intervals:
        H[R].append(held(R))
        S[R].append(sensed(R))
per = lambda runs: np.array([r["ms"] for r in runs]) / steps
fmt = lambda v: f"median {np.median(v):.4f} ms (min {v.min():.4f}, max {v.max():.4f})"
say(f"held loop on measurements against the held loop on the true state: {T} trajectories x {N}-knot horizon, {steps} control steps, "
    f"1 x 3 budget, 5 dispersions, noise, limits, gains on; sensor 0.38 deg/s, 1 deg, biases, latency 1; {args.rounds} alternating rounds "
    f"after a warm-up; device time of the loop per control step (HIP events)")
for R in args.intervals:
    mh, ms = per(H[R]), per(S[R])
    say(f"R = {R:2d} ({H[R][-1]['n_solves']:3d} solves)  tsat_mpc_run_held:        {fmt(mh)}   [backward, forward, dual, inner] {H[R][-1]['tally'].tolist()}")
    say(f"                      tsat_mpc_run_held_sensed: {fmt(ms)}   [backward, forward, dual, inner] {S[R][-1]['tally'].tolist()}"
        f"   {np.median(ms) / np.median(mh):.3f} x the held loop's time")
s.close()
