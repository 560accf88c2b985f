"""Developer tool: one ensemble call against the loop it replaces, on the configs[1] workload (1024 slews x 1000 knots, solved
once), M = 64 realisations per slew.
  (a) one `attitude_ensemble` call: host clock around the synchronous call (uploads, gains and both kernels included), and the
      HIP-event times of its gains and ensemble kernels (the library prints them when TSAT_ENSEMBLE_TIMING=1);
  (b) 64 calls of `attitude_simulation` on the RESIDENT batch (tsat_tvlqr_resident: nothing re-uploaded, statistic only) with
      noise_ids = id0 + m — the strongest way to get the same 65 536 statistics without the ensemble entry point.
Both are warmed up, then alternated `--rounds` times in one process; medians and spread go to stdout and to `--out`."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "ensemble_timing.txt"))
args = ap.parse_args()
T, N, M = args.T, args.N, args.M

b = ss.workload_monte_carlo(T=T, N=N)
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
Qd, Qfd, Rd = tr.tvlqr_weights(T, r=0.5e3)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
ids = tr.ensemble_noise_ids(T, M)
SEED = 2019


def ensemble():
    """(wall s, gains kernel ms, ensemble kernel ms, stats)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            out = tr.attitude_ensemble(s, b, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED)
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        words = f.read().decode().split()
    g = float(words[words.index("gains_kernel_ms") + 1])
    e = float(words[words.index("ensemble_kernel_ms") + 1])
    return wall, g, e, out["stats"]


def loop():
    """(wall s, stats) of M calls on the resident batch"""
    st = np.zeros((T, M), dtype=out_dtype)
    t0 = time.perf_counter()
    for m in range(M):
        r = tr.attitude_simulation(s, b, None, None, x0s[:, m], Qd, Qfd, Rd, noise_seed=SEED, noise_ids=ids[:, m], want_K=False,
                                   want_trajectories=False)
        st[:, m] = r["stats"]
    return time.perf_counter() - t0, st


from tortoisesat_jl_amd import _abi
out_dtype = _abi.TVLQR_STATS_DTYPE
ensemble(); loop()                                   # warm-up of both
A, B = [], []
for _ in range(args.rounds):
    A.append(ensemble())
    B.append(loop())
s.close()
same = bool(np.array_equal(A[-1][3]["slew_index"], B[-1][1]["slew_index"]))
wa, wb = np.array([a[0] for a in A]), np.array([x[0] for x in B])
ga, ea = np.array([a[1] for a in A]), np.array([a[2] for a in A])
fmt = lambda v, u: f"median {np.median(v):.4f} {u} (min {v.min():.4f}, max {v.max():.4f})"
lines = [
    f"ensemble timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, {args.rounds} alternating rounds after a warm-up",
    f"(a) one tsat_tvlqr_ensemble call, host clock:        {fmt(wa, 's')}",
    f"    its gains kernel (HIP events):                   {fmt(ga, 'ms')}",
    f"    its ensemble kernel (HIP events):                {fmt(ea, 'ms')}",
    f"(b) {M} tsat_tvlqr_resident calls, host clock:        {fmt(wb, 's')}",
    f"(b) / (a), medians: {np.median(wb) / np.median(wa):.2f} x;  worst round of (a) against best round of (b): {wb.min() / wa.max():.2f} x",
    f"same slew indices from both: {same}",
]
print("\n".join(lines))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
