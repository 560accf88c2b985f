"""Developer tool: what the asymptotic periodic LQR (`tsat_aplqr_gains`, `tsat_aplqr_ensemble`) costs next to the projection PD
baseline, whose roll-out it restates with another command.
  Part 1 — the workload of tools/pd_timing.py (1024 slews x 1000 knots, solved once, x 64 realisations, all five dispersions, the
  plan's box, the orbit table): one `attitude_ensemble_pd` call against one `attitude_ensemble_aplqr` call, both tracking the same
  plan with its feed-forward. HIP-event times of the two roll-out kernels, tsat_pd_gg_kernel and tsat_aplqr_gg_kernel (the library
  prints them when TSAT_ENSEMBLE_TIMING=1), and the host clock. One warm-up of both, then `--rounds` alternating rounds in one
  process; medians, min, max, the ratio and the run-to-run spread of the PD kernel, which is the yardstick: no time is fixed in advance.
  Part 2 — the gains kernel at T = `--T` over the full table: HIP-event time of tsat_aplqr_gains_kernel and the host clock of the
  call, iterations and the worst residual.
Everything goes to `--out` and to stdout."""
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
ap.add_argument("--wn", type=float, default=0.02)
ap.add_argument("--zeta", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "aplqr_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
SEED, A_KM, INC = 2019, ss.R_EARTH_KM + 400.0, 96.6
GM = tr.GM_EARTH
QD, RD = np.array([1.5e-4] * 3 + [1e4] * 3), np.full(3, 8e6)       # the reference's weights (src/comparison/psiaki2001_Period_LQR.jl)
text = []


def say(line):
    print(line, flush=True)
    text.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


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
    ms = {k: float(words[words.index(k + "_kernel_ms") + 1]) for k in ("gains", "pd") if k + "_kernel_ms" in words}
    return wall, ms, out


fmt = lambda v, u: f"median {np.median(v):.4f} {u} (min {v.min():.4f}, max {v.max():.4f})"
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)

T, N, M = args.T, args.N, args.M
b = ss.workload_monte_carlo(T=T, N=N)
Rtab = ss.circular_orbit_rows(b.n_tab, 0.2, A_KM, INC)[None]
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
kd, kp = tr.pd_gains(b.Jmat, args.wn, args.zeta)
sat = (b.ulo, b.uhi)

# ---- part 2 first: the gains the roll-out flies ----------------------------------------------------------------------------
gains = lambda: timed(lambda: tr.aplqr_gains(s, b, QD, RD, allow_failed=True))
gains()
G = [gains() for _ in range(args.rounds)]
Kg, info = G[-1][2]
wg, eg = np.array([r[0] for r in G]), np.array([r[1]["gains"] for r in G])

# ---- part 1: the two roll-out kernels on the same plan ----------------------------------------------------------------------
pd = lambda: timed(lambda: tr.attitude_ensemble_pd(s, b, x0s, kd, kp, SEED, X=res["X"], U=res["U"], plant=plant, Rtab=Rtab, gm=GM, sat=sat))
aq = lambda: timed(lambda: tr.attitude_ensemble_aplqr(s, b, x0s, Kg, RD, SEED, X=res["X"], U=res["U"], plant=plant, Rtab=Rtab, gm=GM, sat=sat))
pd(); aq()                                           # warm-up of both
A, B = [], []
for _ in range(args.rounds):
    A.append(pd())
    B.append(aq())
wa, wb = np.array([r[0] for r in A]), np.array([r[0] for r in B])
ea, eb = np.array([r[1]["pd"] for r in A]), np.array([r[1]["pd"] for r in B])
say(f"APLQR timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, all five dispersions, noise, the plan's box, "
    f"gravity gradient, plan + feed-forward; {args.rounds} alternating rounds after a warm-up")
say(f"(a) one tsat_pd_ensemble call, host clock:                      {fmt(wa, 's')}")
say(f"    its roll-out, tsat_pd_gg_kernel (HIP events):               {fmt(ea, 'ms')}")
say(f"(b) one tsat_aplqr_ensemble call, host clock:                   {fmt(wb, 's')}")
say(f"    its roll-out, tsat_aplqr_gg_kernel (HIP events):            {fmt(eb, 'ms')}")
say(f"(b) / (a), medians: host clock {np.median(wb) / np.median(wa):.3f} x, roll-out kernel {np.median(eb) / np.median(ea):.3f} x; "
    f"run-to-run spread (max / min) of (a)'s kernel {ea.max() / ea.min():.3f} x, of (b)'s {eb.max() / eb.min():.3f} x")
say(f"failures of {T * M}: (a) PD + feed-forward {int(A[-1][2]['summary'][:, 1].sum())}, (b) APLQR + feed-forward {int(B[-1][2]['summary'][:, 1].sum())}")
say(f"gains: tsat_aplqr_gains at T = {T} over the full {b.n_tab}-row table, the reference's weights; {args.rounds} rounds after a warm-up")
say(f"    one call from host arrays, host clock:                      {fmt(wg, 's')}")
say(f"    tsat_aplqr_gains_kernel (HIP events):                       {fmt(eg, 'ms')}")
say(f"    status != 0 on {int(np.count_nonzero(info['status']))} of {T}; iterations {int(info['iterations'].min())} .. {int(info['iterations'].max())}; "
    f"worst residual {float(info['residual'].max()):.2e}; smallest pivot {float(info['pivot_min'].min()):.2e}")
s.close()
