"""Developer tool: what the projection PD baseline (`tsat_pd_ensemble`) costs next to the tracked ensemble it is compared against.
  Part 1 — the workload of tools/gg_timing.py (1024 slews x 1000 knots, solved once, x 64 realisations, all five dispersions, the
  plan's box, the orbit table): one `attitude_ensemble_gg` call against one `attitude_ensemble_pd` call that tracks the same plan
  with its feed-forward. HIP-event times of the two roll-out kernels (the library prints them when TSAT_ENSEMBLE_TIMING=1) and the
  host clock. One warm-up of both, then `--rounds` alternating rounds in one process; medians, min, max and the ratio. The PD call
  launches no gains kernel and reads no gain rows; whether that makes its roll-out faster is what this part measures.
  Part 2 — regulation over one orbit: `--reg-T` slews x `--reg-N` knots (27 000 knots of 0.2 s) x 64 realisations with X = None, from
  host arrays: kernel time and host clock of the call. Nothing of size N is uploaded.
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
ap.add_argument("--reg-T", type=int, default=256)
ap.add_argument("--reg-N", type=int, default=27000)
ap.add_argument("--wn", type=float, default=0.02)
ap.add_argument("--zeta", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "pd_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
SEED, A_KM, INC = 2019, ss.R_EARTH_KM + 400.0, 96.6
GM = tr.GM_EARTH
text = []


def say(line):
    print(line, flush=True)
    text.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


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
    ms = {k: float(words[words.index(k + "_kernel_ms") + 1]) for k in ("pack", "gains", "ensemble", "pd") if k + "_kernel_ms" in words}
    return wall, ms, out


fmt = lambda v, u: f"median {np.median(v):.4f} {u} (min {v.min():.4f}, max {v.max():.4f})"
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)

# ---- part 1: the two roll-out kernels on the same plan ----------------------------------------------------------------------
T, N, M = args.T, args.N, args.M
b = ss.workload_monte_carlo(T=T, N=N)
Rtab = ss.circular_orbit_rows(b.n_tab, 0.2, A_KM, INC)[None]
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
Qd, Qfd, Rd = tr.tvlqr_weights(T, r=0.5e3)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
kd, kp = tr.pd_gains(b.Jmat, args.wn, args.zeta)
sat = (b.ulo, b.uhi)
tvlqr = lambda: timed(lambda: tr.attitude_ensemble_gg(s, b, res["X"], res["U"], x0s, Qd, Qfd, Rd, SEED, plant, Rtab, GM, sat=sat))
pd = lambda: timed(lambda: tr.attitude_ensemble_pd(s, b, x0s, kd, kp, SEED, X=res["X"], U=res["U"], plant=plant, Rtab=Rtab, gm=GM, sat=sat))
tvlqr(); pd()                                        # warm-up of both
A, B = [], []
for _ in range(args.rounds):
    A.append(tvlqr())
    B.append(pd())
wa, wb = np.array([r[0] for r in A]), np.array([r[0] for r in B])
ea, eb = np.array([r[1]["ensemble"] for r in A]), np.array([r[1]["pd"] for r in B])
say(f"PD baseline timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, all five dispersions, noise, the plan's box, "
    f"gravity gradient; PD gains wn = {args.wn} rad/s, zeta = {args.zeta}; {args.rounds} alternating rounds after a warm-up")
say(f"(a) one tsat_tvlqr_ensemble_gg call, host clock:                {fmt(wa, 's')}")
say(f"    its gains kernel (HIP events):                              {fmt(np.array([r[1]['gains'] for r in A]), 'ms')}")
say(f"    its roll-out, tsat_ensemble_gg_kernel (HIP events):         {fmt(ea, 'ms')}")
say(f"(b) one tsat_pd_ensemble call (plan + feed-forward), host clock: {fmt(wb, 's')}")
say(f"    its roll-out, tsat_pd_gg_kernel (HIP events):               {fmt(eb, 'ms')}")
say(f"(b) / (a), medians: host clock {np.median(wb) / np.median(wa):.3f} x, roll-out kernel {np.median(eb) / np.median(ea):.3f} x; "
    f"spread of (a)'s own rounds (max / min) {ea.max() / ea.min():.3f} x")
say(f"failures of {T * M}: (a) TVLQR {int(A[-1][2]['summary'][:, 1].sum())}, (b) PD + feed-forward {int(B[-1][2]['summary'][:, 1].sum())}")

# ---- part 2: regulation over one orbit, nothing of size N uploaded --------------------------------------------------------
T2, N2 = args.reg_T, args.reg_N
full = ss.workload_monte_carlo(T=max(T2, 2), N=2)
b2 = full.slice(0, T2)
b2.N = N2
rows = 2048
dt_row = float(b2.dt[0]) * (N2 - 1) / (rows - 2)
b2.Btab, b2.n_tab = np.ascontiguousarray(ss.dipole_btable(rows, dt_row, A_KM, INC)[None]), rows
b2.btab_idx[:] = 0
b2.tau0[:], b2.dtau[:] = 0.0, float(b2.dt[0]) / dt_row
R2 = ss.circular_orbit_rows(rows, dt_row, A_KM, INC)[None]
x0s2 = tr.ensemble_initial_states(b2.x0, M, np.random.default_rng(5))
plant2 = tr.disperse_plant(b2.Jmat, M, np.random.default_rng(7), **LEVELS)
kd2, kp2 = tr.pd_gains(b2.Jmat, args.wn, args.zeta)
reg = lambda: timed(lambda: tr.attitude_ensemble_pd(s, b2, x0s2, kd2, kp2, SEED, plant=plant2, Rtab=R2, gm=GM, sat=(b2.ulo, b2.uhi),
                                                    limit_mode=1))
reg()
C = [reg() for _ in range(args.rounds)]
wc, ec_ = np.array([r[0] for r in C]), np.array([r[1]["pd"] for r in C])
say(f"regulation over one orbit: {T2} slews x {N2} knots of {float(b2.dt[0])} s x {M} realisations, X = None, a {rows}-row table, "
    f"limit_mode 1; {args.rounds} rounds after a warm-up")
say(f"    one tsat_pd_ensemble call from host arrays, host clock:     {fmt(wc, 's')}")
say(f"    its roll-out kernel (HIP events):                           {fmt(ec_, 'ms')}")
say(f"    failures of {T2 * M}: {int(C[-1][2]['summary'][:, 1].sum())}")
s.close()
