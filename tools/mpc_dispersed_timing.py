"""Developer tool: what the receding-horizon loop on a noisy, dispersed plant with limits costs over the loop on the model's
plant, and the figure the entry point exists for.
  Part 1 — BASELINE.json configs[4] shape on one GPU (4096 trajectories x 200-knot horizon, 200 control steps, 1 x 3 budget), the
  workload of tools/mpc_timing.py:
    (a) `mpc.receding_horizon` (tsat_mpc_run, rk4 plant);
    (b) `mpc.receding_horizon_dispersed` (tsat_mpc_run_dispersed) with all five dispersions
        (disperse_plant(default_rng(7), 0.01, 0.2 deg, 0.01, 0.5 deg, 2e-4 A m^2)), generated noise and half the plan's box as limits.
  One warm-up of both, then `--rounds` alternating rounds in one process; HIP-event time of the whole loop per control step,
  medians, min, max, (b) - (a) as a share of (a), and (a) next to the figure of profiles/r04/mpc_timing.txt.
  Part 2 — the first `--slews` slews of the workload of tools/dispersed_timing.py (1024 x 1000 knots, M = 64 plants per slew, the
  same plants, perturbed starts and generator ids): failures under dispersed TVLQR tracking of the solved plan next to failures
  under the receding-horizon loop (horizon = the plan's 1000 knots, warm start = the plan, 999 control steps, 1 x 3 budget, the
  plan's box as limits), whatever the outcome.
Everything goes to stdout and, line by line, to `--out`."""
import argparse
import os
import re
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
ap.add_argument("--slews", type=int, default=4)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc", "dispersed_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
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

# ---- part 1: cost ------------------------------------------------------------------------------------------------------
T, N, steps = args.T, args.N, args.steps
b = ss.workload_monte_carlo(T=T, N=N, seed=20190602)
B = ss.dipole_btable(steps + N + 8, 0.2, 6771.0, 96.6)
b.Btab, b.n_tab = np.ascontiguousarray(B[None]), B.shape[0]
b.dtau[:] = 1.0
prob = to.BatchProblem.from_arrays(b)
plant = np.ascontiguousarray(tr.disperse_plant(b.Jmat, 1, np.random.default_rng(7), **LEVELS)[:, 0])
sat = (0.5 * b.ulo, 0.5 * b.uhi)
nominal = lambda n=steps: mpc.receding_horizon(prob, s, n, plant_integrator=4)
dispersed = lambda n=steps: mpc.receding_horizon_dispersed(prob, s, n, plant=plant, sat=sat, noise_opts=dict(noise_seed=SEED))
nominal(5); dispersed(5)                               # warm-up of both
A, D = [], []
for _ in range(args.rounds):
    A.append(nominal())
    D.append(dispersed())
ma, md = np.array([r["ms"] for r in A]) / steps, np.array([r["ms"] for r in D]) / steps
fmt = lambda v: f"median {np.median(v):.4f} ms (min {v.min():.4f}, max {v.max():.4f})"
say(f"dispersed receding-horizon timing: {T} trajectories x {N}-knot horizon, {steps} control steps, 1 x 3 budget, "
    f"{args.rounds} alternating rounds after a warm-up; device time of the loop per control step (HIP events)")
say(f"(a) tsat_mpc_run (model's plant, rk4):                        {fmt(ma)}")
say(f"(b) tsat_mpc_run_dispersed (5 dispersions, noise, limits):    {fmt(md)}")
say(f"(b) - (a), medians: {np.median(md) - np.median(ma):+.4f} ms per control step = {100.0 * (np.median(md) / np.median(ma) - 1.0):+.2f} % of (a)")
try:
    txt = open(os.path.join(ROOT, "profiles", "r04", "mpc_timing.txt")).read()
    old = float(re.search(rf"T={T} horizon={N} steps={steps}: .*? = ([0-9.]+) ms/step", txt).group(1))
    say(f"(a) against profiles/r04/mpc_timing.txt ({old:.3f} ms/step for the same shape): {np.median(ma) / old:.3f} x")
except (OSError, AttributeError):
    say("(a): no figure for this shape in profiles/r04/mpc_timing.txt")
last = D[-1]
say(f"(b) last round: clipped steps per trajectory {int(last['n_clipped'].min())} .. {int(last['n_clipped'].max())} of {steps}, "
    f"last inner iterations {last['stats']['inner_iters'].mean():.2f} ((a): {A[-1]['stats']['inner_iters'].mean():.2f})")

# ---- part 2: does re-planning arrive where tracking fails? ----------------------------------------------------------------
T2, N2, M, n = 1024, 1000, args.M, args.slews
full = ss.workload_monte_carlo(T=T2, N=N2)
plants = tr.disperse_plant(full.Jmat, M, np.random.default_rng(7), **LEVELS)[:n]          # the ensemble's plants of these slews
x0s = tr.ensemble_initial_states(full.x0, M, np.random.default_rng(5))[:n]
sub = full.slice(0, n)
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s.opts = opts
res = to.solve_(to.BatchProblem.from_arrays(sub), s, want_K=False)
Qd, Qfd, Rd = tr.tvlqr_weights(n, r=0.5e3)
id0 = np.arange(n, dtype=np.int64) * M
tv = tr.attitude_ensemble_dispersed(s, sub, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED, plants, sat=(sub.ulo, sub.uhi), noise_id0=id0)
# the same slews for the loop: the table continued for another horizon (rows 0 .. N-1 are the plan's), every realisation started
# at its own perturbed state, warm-started with the plan
ext = sub.slice(0, n)
B2 = ss.dipole_btable(2 * N2 + 8, 0.2, ss.R_EARTH_KM + 400.0, 96.6, 0.0, 0.0)
assert np.array_equal(B2[:N2], full.Btab[0][:N2])
ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B2[None]), B2.shape[0], np.ascontiguousarray(res["U"])
tiled, kw = mpc.tile_realisations(ext, M, plant=plants, noise_id0=id0, sat=(sub.ulo, sub.uhi))
tiled.x0 = np.ascontiguousarray(x0s.reshape(n * M, 7))
s.opts = to.AugmentedLagrangianSolverOptions()
s.opts.opts_uncon.dJ_counter_limit = 1
rh = mpc.receding_horizon_dispersed(to.BatchProblem.from_arrays(tiled), s, N2 - 1, noise_opts=dict(noise_seed=SEED), **kw)
s.close()
st_tv, st_rh = tv["stats"].reshape(-1), rh["tracking_stats"]
arr = lambda st: st["slew_time"][st["failed"] == 0]
spread = lambda v: f"slew time of the arrivals mean {v.mean():.1f} s ({v.min():.1f} .. {v.max():.1f})" if v.size else "no arrivals"
say(f"re-planning against tracking: slews 0 .. {n - 1} of the workload of profiles/ensemble/dispersed_timing.txt x {M} plants = {n * M} "
    f"closed loops of {N2} samples, same plants, perturbed starts and generator ids")
say(f"  dispersed TVLQR tracking (tsat_tvlqr_ensemble_dispersed): {int(np.count_nonzero(st_tv['failed']))} of {n * M} fail; {spread(arr(st_tv))}")
say(f"  receding-horizon loop (tsat_mpc_run_dispersed, {N2}-knot horizon, {N2 - 1} steps, {rh['ms'] / (N2 - 1):.3f} ms per step): "
    f"{int(np.count_nonzero(st_rh['failed']))} of {n * M} fail; {spread(arr(st_rh))}")
say(f"  failures per slew, tracking / loop: " + ", ".join(f"{int(a)} / {int(c)}" for a, c in
    zip(tv["summary"][:, 1], st_rh["failed"].reshape(n, M).sum(axis=1))))
say(f"  final error angle, median over the loops: tracking {np.median(st_tv['final_angle']):.4f} rad, loop {np.median(st_rh['final_angle']):.4f} rad; "
    f"clipped steps per loop {int(rh['n_clipped'].min())} .. {int(rh['n_clipped'].max())}")
