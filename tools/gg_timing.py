"""Developer tool: what the gravity-gradient term costs the dispersed ensemble and the held loop, and the figure the two entry
points exist for — do tracking and re-planning still arrive under a disturbance torque neither of them models?
  Part 1 — the workload of tools/dispersed_timing.py (1024 slews x 1000 knots, solved once, x 64 realisations, all five dispersions,
  the plan's box): one `attitude_ensemble_dispersed` call against one `attitude_ensemble_gg` call. HIP-event times of the kernels
  (the library prints them when TSAT_ENSEMBLE_TIMING=1) and the host clock. One warm-up of both, then `--rounds` alternating rounds
  in one process; medians, min, max and the ratio.
  Part 2 — the shape, plants, noise and limits of tools/mpc_held_timing.py (4096 trajectories x 200-knot horizon, 200 control
  steps): `mpc.receding_horizon_held` against `mpc.receding_horizon_held_gg` at R in --intervals, alternated in the same way; device
  time of the whole loop per control step.
  Part 3 (--slews 0 leaves it out) — slews 0 .. 3 of the configs[1] workload x 64 plants with the 3U inertia as the model's:
  failures of 256 under dispersed TVLQR tracking, under the every-step loop (R = 1) and under the held loop at R = 10, each with
  and without the term.
Parts 1 and 3 go to `--out-ensemble`, parts 2 and 3 to `--out-mpc`, everything to stdout."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TSAT_ENSEMBLE_TIMING"] = "1"
import numpy as np
from tsat_loader import load_package

load_package()
from tortoisesat_jl_amd import mpc, slew_setup as ss, tracking as tr, trajopt as to

ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=1024)
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--held-T", type=int, default=4096)
ap.add_argument("--held-N", type=int, default=200)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--intervals", type=int, nargs="+", default=[1, 5, 10, 20])
ap.add_argument("--slews", type=int, default=4)
ap.add_argument("--out-ensemble", default=os.path.join(ROOT, "profiles", "ensemble", "gg_timing.txt"))
ap.add_argument("--out-mpc", default=os.path.join(ROOT, "profiles", "mpc", "gg_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
SEED, A_KM, INC = 2019, ss.R_EARTH_KM + 400.0, 96.6
GM = tr.GM_EARTH
text = {"ensemble": [], "mpc": []}


def say(line, *where):
    print(line, flush=True)
    for w in where:
        text[w].append(line)
        path = args.out_ensemble if w == "ensemble" else args.out_mpc
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(text[w]) + "\n")


def timed(call):
    """(wall s, {kernel: ms}, result) of one synchronous ensemble call, with what the library wrote to stderr parsed"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            out = call()
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        words = f.read().decode().split()
    ms = {k: float(words[words.index(k + "_kernel_ms") + 1]) for k in ("pack", "gains", "ensemble") if k + "_kernel_ms" in words}
    return wall, ms, out


fmt = lambda v, u: f"median {np.median(v):.4f} {u} (min {v.min():.4f}, max {v.max():.4f})"
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)

# ---- part 1: the ensemble kernel ---------------------------------------------------------------------------------------
T, N, M = args.T, args.N, args.M
b = ss.workload_monte_carlo(T=T, N=N)
Rtab = ss.circular_orbit_rows(b.n_tab, 0.2, A_KM, INC)[None]
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
Qd, Qfd, Rd = tr.tvlqr_weights(T, r=0.5e3)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
head = (s, b, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED, plant)
dispersed = lambda: timed(lambda: tr.attitude_ensemble_dispersed(*head, sat=(b.ulo, b.uhi)))
gravity = lambda: timed(lambda: tr.attitude_ensemble_gg(*head, Rtab, GM, sat=(b.ulo, b.uhi)))
dispersed(); gravity()                               # warm-up of both
A, B = [], []
for _ in range(args.rounds):
    A.append(dispersed())
    B.append(gravity())
col = lambda runs, k: np.array([r[1][k] for r in runs])
wa, wb = np.array([r[0] for r in A]), np.array([r[0] for r in B])
ea, eb = col(A, "ensemble"), col(B, "ensemble")
say(f"gravity-gradient timing, ensemble: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, the workload's inertia, "
    f"{args.rounds} alternating rounds after a warm-up", "ensemble")
say(f"(a) one tsat_tvlqr_ensemble_dispersed call, host clock:  {fmt(wa, 's')}", "ensemble")
say(f"    its ensemble kernel (HIP events):                    {fmt(ea, 'ms')}", "ensemble")
say(f"(b) one tsat_tvlqr_ensemble_gg call, host clock:         {fmt(wb, 's')}", "ensemble")
say(f"    its pack kernels, plants + orbit table (HIP events): {fmt(col(B, 'pack'), 'ms')}", "ensemble")
say(f"    its ensemble kernel (HIP events):                    {fmt(eb, 'ms')}", "ensemble")
say(f"(b) / (a), medians: host clock {np.median(wb) / np.median(wa):.3f} x, ensemble kernel {np.median(eb) / np.median(ea):.3f} x; "
    f"spread of (a)'s own rounds (max / min) {ea.max() / ea.min():.3f} x", "ensemble")
say(f"failures of {T * M}: (a) {int(A[-1][2]['summary'][:, 1].sum())}, (b) {int(B[-1][2]['summary'][:, 1].sum())} "
    f"(isotropic model inertia: the term acts on the dispersion of Jp alone)", "ensemble")

# ---- part 2: the hold ----------------------------------------------------------------------------------------------------
s.opts = to.AugmentedLagrangianSolverOptions()
s.opts.opts_uncon.dJ_counter_limit = 1
T2, N2, steps = args.held_T, args.held_N, args.steps
b2 = ss.workload_monte_carlo(T=T2, N=N2, seed=20190602)
rows = steps + N2 + 8
b2.Btab, b2.n_tab = np.ascontiguousarray(ss.dipole_btable(rows, 0.2, A_KM, INC)[None]), rows
b2.dtau[:] = 1.0
R2 = ss.circular_orbit_rows(rows, 0.2, A_KM, INC)[None]
prob = to.BatchProblem.from_arrays(b2)
plant2 = np.ascontiguousarray(tr.disperse_plant(b2.Jmat, 1, np.random.default_rng(7), **LEVELS)[:, 0])
kw1 = dict(plant=plant2, sat=(0.5 * b2.ulo, 0.5 * b2.uhi), noise_opts=dict(noise_seed=SEED))
held = lambda R, n=steps: mpc.receding_horizon_held(prob, s, n, R, **kw1)
held_gg = lambda R, n=steps: mpc.receding_horizon_held_gg(prob, s, n, R, R2, GM, **kw1)
for R in args.intervals:
    held(R, max(5, R + 1)); held_gg(R, max(5, R + 1))                 # warm-up of every configuration
H, G = {R: [] for R in args.intervals}, {R: [] for R in args.intervals}
for _ in range(args.rounds):
    for R in args.intervals:
        H[R].append(held(R))
        G[R].append(held_gg(R))
per = lambda runs: np.array([r["ms"] for r in runs]) / steps
say(f"gravity-gradient timing, hold: {T2} trajectories x {N2}-knot horizon, {steps} control steps, 1 x 3 budget, 5 dispersions, noise, "
    f"limits; {args.rounds} alternating rounds after a warm-up; device time of the loop per control step (HIP events)", "mpc")
for R in args.intervals:
    mh, mg = per(H[R]), per(G[R])
    say(f"R = {R:2d} ({H[R][-1]['n_solves']:3d} solves): tsat_mpc_run_held {fmt(mh, 'ms')}; tsat_mpc_run_held_gg {fmt(mg, 'ms')}; "
        f"ratio of the medians {np.median(mg) / np.median(mh):.3f} x", "mpc")

# ---- part 3: failures with and without the term ------------------------------------------------------------------------------
if args.slews > 0:
    n, N3 = args.slews, 1000
    full = ss.workload_monte_carlo(T=1024, N=N3)
    sub = full.slice(0, n)
    sub.Jmat[:] = ss.jmat_cm(ss.INERTIA["3U"])
    plants = tr.disperse_plant(sub.Jmat, M, np.random.default_rng(7), **LEVELS)
    x0s3 = tr.ensemble_initial_states(full.x0, M, np.random.default_rng(5))[:n]
    s.opts = opts
    res3 = to.solve_(to.BatchProblem.from_arrays(sub), s, want_K=False)
    Qd3, Qfd3, Rd3 = tr.tvlqr_weights(n, r=0.5e3)
    id0 = np.arange(n, dtype=np.int64) * M
    ext = sub.slice(0, n)
    rows3 = 2 * N3 + 8
    ext.Btab, ext.n_tab, ext.U0 = np.ascontiguousarray(ss.dipole_btable(rows3, 0.2, A_KM, INC)[None]), rows3, np.ascontiguousarray(res3["U"])
    R3 = ss.circular_orbit_rows(rows3, 0.2, A_KM, INC)[None]
    tiled, kw = mpc.tile_realisations(ext, M, plant=plants, noise_id0=id0, sat=(sub.ulo, sub.uhi))
    tiled.x0 = np.ascontiguousarray(x0s3.reshape(n * M, 7))
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"failures with and without the term: slews 0 .. {n - 1} of the configs[1] workload x {M} plants = {n * M} closed loops of {N3} "
        f"samples, the 3U inertia as the model's (weights and box of the workload), all five dispersions, noise, the plan's box; "
        f"gm = {GM} km^3/s^2, 400 km circular orbit", "ensemble", "mpc")
    tv = {}
    for name, gm in (("without", 0.0), ("with", GM)):
        r = tr.attitude_ensemble_gg(s, sub, res3["X"], res3["U"], x0s3, Qd3, Qfd3, Rd3, SEED, plants, R3[:, :sub.n_tab], gm,
                                    sat=(sub.ulo, sub.uhi), noise_id0=id0)
        tv[name] = fails(r["stats"].reshape(-1))
    say(f"  dispersed TVLQR tracking of the solved plan: {tv['without']} of {n * M} fail without the term, {tv['with']} with it", "ensemble", "mpc")
    s.opts = to.AugmentedLagrangianSolverOptions()
    s.opts.opts_uncon.dJ_counter_limit = 1
    prob3 = to.BatchProblem.from_arrays(tiled)
    for R, label in ((1, "every-step loop (R = 1)"), (10, "held loop R = 10, gains on")):
        out = {}
        for name, gm in (("without", 0.0), ("with", GM)):
            r = mpc.receding_horizon_held_gg(prob3, s, N3 - 1, R, R3, gm, noise_opts=dict(noise_seed=SEED), **kw)
            out[name] = (fails(r["tracking_stats"]), r["ms"] / (N3 - 1))
        say(f"  {label}: {out['without'][0]} of {n * M} fail without the term ({out['without'][1]:.3f} ms per step), "
            f"{out['with'][0]} with it ({out['with'][1]:.3f} ms per step)", "ensemble", "mpc")
s.close()
