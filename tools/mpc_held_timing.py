"""Developer tool: what re-planning every R control steps (tsat_mpc_run_held) costs next to re-planning at every step
(tsat_mpc_run_dispersed), and the figure the entry point exists for: failures against the re-plan interval, gains on and off.
  Part 1 — the shape, dispersions, noise and limits of tools/mpc_dispersed_timing.py (4096 trajectories x 200-knot horizon, 200
  control steps, 1 x 3 budget, half the plan's box as limits): `mpc.receding_horizon_dispersed` and `mpc.receding_horizon_held` at
  R in --intervals, gains on. One warm-up of each, then `--rounds` alternating rounds in one process; HIP-event time of the whole
  loop per control step, medians, min, max, and the number of solves.
  Part 2 (--slews 0 leaves it out) — the 4 slews x 64 plants study of tools/mpc_dispersed_timing.py (same plants, perturbed starts
  and generator ids, 1000-knot horizon, 999 control steps): failures of 256 under dispersed TVLQR tracking of the solved plan, under
  the every-step loop, and under the held loop at R in --study-intervals with the gains on and off.
Kernel times come from a separate run of this tool under `rocprofv3 --kernel-trace --stats` (tools/README.md).
Everything goes to stdout and, line by line, to `--out`."""
import argparse
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
ap.add_argument("--intervals", type=int, nargs="+", default=[1, 2, 5, 10, 20])
ap.add_argument("--slews", type=int, default=4)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--study-intervals", type=int, nargs="+", default=[1, 2, 5, 10, 20, 50])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc", "held_timing.txt"))
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
kw1 = dict(plant=plant, sat=(0.5 * b.ulo, 0.5 * b.uhi), noise_opts=dict(noise_seed=SEED))
every = lambda n=steps: mpc.receding_horizon_dispersed(prob, s, n, **kw1)
held = lambda R, n=steps: mpc.receding_horizon_held(prob, s, n, R, **kw1)
every(5)
for R in args.intervals:
    held(R, max(5, R + 1))                              # warm-up of every configuration
E, H = [], {R: [] for R in args.intervals}
for _ in range(args.rounds):
    E.append(every())
    for R in args.intervals:
        H[R].append(held(R))
per = lambda runs: np.array([r["ms"] for r in runs]) / steps
fmt = lambda v: f"median {np.median(v):.4f} ms (min {v.min():.4f}, max {v.max():.4f})"
say(f"held receding-horizon timing: {T} trajectories x {N}-knot horizon, {steps} control steps, 1 x 3 budget, 5 dispersions, noise, "
    f"limits; {args.rounds} alternating rounds after a warm-up; device time of the loop per control step (HIP events)")
me = per(E)
say(f"tsat_mpc_run_dispersed ({steps} solves):                   {fmt(me)}")
for R in args.intervals:
    mh = per(H[R])
    say(f"tsat_mpc_run_held R = {R:2d}, gains on ({H[R][-1]['n_solves']:3d} solves):          {fmt(mh)}   "
        f"{np.median(me) / np.median(mh):.2f} x the every-step loop's rate")
last = H[args.intervals[-1]][-1]
say(f"R = {args.intervals[-1]}, last round: clipped steps per trajectory {int(last['n_clipped'].min())} .. {int(last['n_clipped'].max())} of "
    f"{steps}, solve statuses {np.unique(last['stats']['status']).tolist()}")

# ---- part 2: failures against the re-plan interval ---------------------------------------------------------------------------
if args.slews > 0:
    T2, N2, M, n = 1024, 1000, args.M, args.slews
    full = ss.workload_monte_carlo(T=T2, N=N2)
    plants = tr.disperse_plant(full.Jmat, M, np.random.default_rng(7), **LEVELS)[:n]
    x0s = tr.ensemble_initial_states(full.x0, M, np.random.default_rng(5))[:n]
    sub = full.slice(0, n)
    opts = to.AugmentedLagrangianSolverOptions()
    opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
    s.opts = opts
    res = to.solve_(to.BatchProblem.from_arrays(sub), s, want_K=False)
    Qd, Qfd, Rd = tr.tvlqr_weights(n, r=0.5e3)
    id0 = np.arange(n, dtype=np.int64) * M
    tv = tr.attitude_ensemble_dispersed(s, sub, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED, plants, sat=(sub.ulo, sub.uhi), noise_id0=id0)
    ext = sub.slice(0, n)
    B2 = ss.dipole_btable(2 * N2 + 8, 0.2, ss.R_EARTH_KM + 400.0, 96.6, 0.0, 0.0)
    assert np.array_equal(B2[:N2], full.Btab[0][:N2])
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(B2[None]), B2.shape[0], np.ascontiguousarray(res["U"])
    tiled, kw = mpc.tile_realisations(ext, M, plant=plants, noise_id0=id0, sat=(sub.ulo, sub.uhi))
    tiled.x0 = np.ascontiguousarray(x0s.reshape(n * M, 7))
    s.opts = to.AugmentedLagrangianSolverOptions()
    s.opts.opts_uncon.dJ_counter_limit = 1
    prob2 = to.BatchProblem.from_arrays(tiled)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    mean_ok = lambda st: (f"{st['slew_time'][st['failed'] == 0].mean():.1f} s" if fails(st) < st.size else "no arrivals")
    say(f"failures against the re-plan interval: slews 0 .. {n - 1} of the workload of profiles/ensemble/dispersed_timing.txt x {M} plants "
        f"= {n * M} closed loops of {N2} samples, same plants, perturbed starts and generator ids as profiles/mpc/dispersed_timing.txt")
    say(f"  dispersed TVLQR tracking of the solved plan: {fails(tv['stats'].reshape(-1))} of {n * M} fail")
    rh = mpc.receding_horizon_dispersed(prob2, s, N2 - 1, noise_opts=dict(noise_seed=SEED), **kw)
    say(f"  every-step loop (tsat_mpc_run_dispersed):    {fails(rh['tracking_stats'])} of {n * M} fail; {rh['ms'] / (N2 - 1):.3f} ms per control step")
    for R in args.study_intervals:
        out = []
        for fb in (True, False):
            r = mpc.receding_horizon_held(prob2, s, N2 - 1, R, feedback=fb, noise_opts=dict(noise_seed=SEED), **kw)
            st = r["tracking_stats"]
            bad = int(np.count_nonzero(r["stats"]["status"] > 1))
            out.append(f"gains {'on ' if fb else 'off'} {fails(st):3d} fail (mean slew time of the arrivals {mean_ok(st)}, {r['ms'] / (N2 - 1):.3f} ms per step"
                       + (f", {bad} last solves REG_FAIL / DIVERGED" if bad else "") + ")")
        say(f"  held loop R = {R:2d} ({r['n_solves']:3d} solves): " + "; ".join(out))
s.close()
