"""Developer tool: what the dispersed-plant ensemble costs over the nominal one, on the configs[1] workload (1024 slews x 1000
knots, solved once), M = 64 realisations per slew.
  (a) one `attitude_ensemble` call (tsat_tvlqr_ensemble);
  (b) one `attitude_ensemble_dispersed` call (tsat_tvlqr_ensemble_dispersed) with all five dispersions
      (disperse_plant(default_rng(7), 0.01, 0.2 deg, 0.01, 0.5 deg, 2e-4 A m^2)) and the plan's box as limits.
Host clock around the synchronous call, and the HIP-event times of its kernels (pack of the per-lane plant records, gains,
ensemble), which the library prints when TSAT_ENSEMBLE_TIMING=1. One warm-up of both, then `--rounds` alternating rounds in one
process; medians, min, max and (b) / (a) go to stdout and to `--out`.
`--inertia` picks the model: the workload's own (isotropic "1U": the nominal kernel drops w x Jw and folds h / j into the control),
a diagonal preset such as "3U", or "full" (a rotated 3U tensor) — (a) under those tells what a general inertia alone costs the
nominal kernel, the yardstick for (b) / (a)."""
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
from tortoisesat_jl_amd import slew_setup as ss, tracking as tr, trajopt as to

ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=1024)
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--inertia", default="workload")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "dispersed_timing.txt"))
args = ap.parse_args()
T, N, M = args.T, args.N, args.M

b = ss.workload_monte_carlo(T=T, N=N)
if args.inertia != "workload":
    J = np.asarray(ss.INERTIA["3U" if args.inertia == "full" else args.inertia], dtype=np.float64)
    if args.inertia == "full":
        R = tr._rotation(np.deg2rad([20.0, -35.0, 50.0]))
        J = R @ J @ R.T
        J = 0.5 * (J + J.T)
    b.Jmat = np.ascontiguousarray(np.repeat(J.T.reshape(1, 9), T, axis=0))
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
Qd, Qfd, Rd = tr.tvlqr_weights(T, r=0.5e3)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5,
                          residual_dipole=2e-4)
SEED = 2019


def timed(call):
    """(wall s, {kernel: ms}, result) of one synchronous call, with what the library wrote to stderr parsed"""
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


nominal = lambda: timed(lambda: tr.attitude_ensemble(s, b, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED))
dispersed = lambda: timed(lambda: tr.attitude_ensemble_dispersed(s, b, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED, plant, sat=(b.ulo, b.uhi)))
nominal(); dispersed()                               # warm-up of both
A, B = [], []
for _ in range(args.rounds):
    A.append(nominal())
    B.append(dispersed())
s.close()
col = lambda runs, k: np.array([r[1][k] for r in runs])
wa, wb = np.array([r[0] for r in A]), np.array([r[0] for r in B])
fmt = lambda v, u: f"median {np.median(v):.4f} {u} (min {v.min():.4f}, max {v.max():.4f})"
fa, fb = A[-1][2]["summary"][:, 1].sum(), B[-1][2]["summary"][:, 1].sum()
lines = [
    f"dispersed timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, model inertia '{args.inertia}', "
    f"{args.rounds} alternating rounds after a warm-up",
    f"(a) one tsat_tvlqr_ensemble call, host clock:            {fmt(wa, 's')}",
    f"    its gains kernel (HIP events):                       {fmt(col(A, 'gains'), 'ms')}",
    f"    its ensemble kernel (HIP events):                    {fmt(col(A, 'ensemble'), 'ms')}",
    f"(b) one tsat_tvlqr_ensemble_dispersed call, host clock:  {fmt(wb, 's')}",
    f"    its plant pack kernel (HIP events):                  {fmt(col(B, 'pack'), 'ms')}",
    f"    its gains kernel (HIP events):                       {fmt(col(B, 'gains'), 'ms')}",
    f"    its ensemble kernel (HIP events):                    {fmt(col(B, 'ensemble'), 'ms')}",
    f"(b) / (a), medians: host clock {np.median(wb) / np.median(wa):.2f} x, ensemble kernel "
    f"{np.median(col(B, 'ensemble')) / np.median(col(A, 'ensemble')):.2f} x",
    f"failures of {T * M}: (a) {int(fa)}, (b) {int(fb)}; clipped knots in (b): {int(B[-1][2]['n_clipped'].sum())}",
]
print("\n".join(lines))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
