"""Developer tool: run the diagnostic build (libtortoise_hip_prof.so, -DTSAT_PROFILE) on the bench workload and
print where a wavefront spends its shader-clock cycles (forward sweep / Jacobian lanes / Riccati / parallel passes).
The stamped build is slower than the product; read SHARES, not absolute time."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from tsat_loader import load_package
pkg = load_package()
pkg._abi.LIB_NAME = os.environ.get("TSAT_PROF_LIB", "libtortoise_hip_prof.so")
from tortoisesat_jl_amd import trajopt as to, slew_setup as ss

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
variant = int(sys.argv[3]) if len(sys.argv) > 3 else 0      # 0 auto, 1 wide, 2 dense, 3 packed (PK_G trajectories per wave)
es = int(sys.argv[4]) if len(sys.argv) > 4 else 0
prec = int(sys.argv[5]) if len(sys.argv) > 5 else 64      # 32: the mixed-precision builds
base = ss.workload_monte_carlo(T=min(T, 1024), N=N)
if T > 1024:       # larger batches re-use the 1024 draws (tiling) so that host-side setup stays cheap
    k = T // 1024
    rep = lambda a: np.ascontiguousarray(np.concatenate([a] * k))
    b = ss.SlewBatch(base.N, base.n_tab, rep(base.x0), rep(base.xf), base.Btab, rep(base.btab_idx), rep(base.tau0), rep(base.dtau),
                     rep(base.dt), rep(base.Jmat), rep(base.Qd), rep(base.Qfd), rep(base.Rd), rep(base.ulo), rep(base.uhi), rep(base.U0))
    T = b.T
else:
    b = base
opts = to.AugmentedLagrangianSolverOptions(); opts.iterations = 5
opts.opts_uncon.iterations = 10; opts.opts_uncon.dJ_counter_limit = 1
solver = to.AugmentedLagrangianSolver(None, opts)
o = opts.to_abi(b.N, b.n_tab, 3, error_state=es)
o.precision = prec
solver.set_kernel_variant(variant)
solver.set_endgame(0)     # one kernel: the stamps of a wavefront cover its trajectories from start to end
if len(sys.argv) > 7:     # keep rule of the one-trajectory builds' line search (tsat_set_store_policy): few, hold
    solver.set_store_policy(int(sys.argv[6]), int(sys.argv[7]))
    print(f"store policy: few = {sys.argv[6]}, hold = {sys.argv[7]}")
one_traj = not (variant >= 3 or (variant == 0 and T >= 2048))
solver.upload(b, o.max_linesearch); solver.trace(2 if one_traj else 1)
ms = solver.run(o); ms = solver.run(o)
tr_all = solver.trace_download()
tr = tr_all[:, 0, :]
nfw = solver.download(want_K=False)["stats"]["n_forward"].astype(float)
if variant >= 3 or (variant == 0 and T >= 3072):   # the packed builds stamp one row per wavefront (its first trajectory): sums over
    tr = tr[::int(os.environ.get("TSAT_PK_G", "4"))]   # its PK_G trajectories
print(f"T = {T}, variant {variant}, error_state {es}, precision {prec}: {len(tr)} stamped wavefronts")
it = tr[:, 4]; nb = tr[:, 5]
tot = tr[:, :4].sum(1)
print(f"kernel {ms:.2f} ms (stamped build); mean inner its {it.mean():.1f}")
for i, name in enumerate(("forward sweep", "jacobian lanes", "riccati", "parallel passes")):
    print(f"  {name:16s}: {tr[:, i].mean()/1e6:8.2f} Mcycles/wave  ({100*tr[:, i].sum()/tot.sum():5.1f} %)  "
          f"per iteration {np.mean(tr[:, i]/np.maximum(it,1))/1e3:8.1f} kcycles; per knot-iteration {np.mean(tr[:, i]/np.maximum(it,1))/N:7.1f} cycles")
if variant >= 3 or (variant == 0 and T >= 3072):
    for i, name in ((6, "of the passes: copy of the accepted roll-out + gradient"), (7, "of the passes: end of an inner loop (duals, penalty, next outer)")):
        print(f"  {name:66s}: per knot-iteration {np.mean(tr[:, i]/np.maximum(it,1))/N:7.1f} cycles")
if variant >= 3 or (variant == 0 and T >= 3072):   # a sweep serves the whole wavefront: cycles per sweep and knot of the WAVE
    G = int(os.environ.get("TSAT_PK_G", "4"))
    sw = nfw.reshape(-1, G).max(1)
    print(f"  forward sweep, per executed sweep of a wavefront and knot: {np.mean(tr[:, 0] / np.maximum(sw, 1)) / N:7.1f} cycles ({sw.mean():.1f} sweeps per wavefront)")
print(f"  slowest wave: {tot.max()/1e6:.1f} Mcycles, {int(it[np.argmax(tot)])} iterations (the launch ends with it); mean wave {tot.mean()/1e6:.1f}")
if not (variant >= 3 or (variant == 0 and T >= 2048)):
    # The launch ends with its slowest wavefront: what the slowest ten did. A line search takes one forward sweep, and one more
    # whenever the sweep had not kept the roll-out that is accepted (repeated = executed - 1 - iterations); its candidates' costs
    # are evaluated CG at a time, one `cost pass` each (columns 6 and 7 of the stamp row: passes, cycles in them).
    npass, cpass = tr[:, 6], tr[:, 7]
    print(f"  cost passes: {npass.mean():.1f} per wave, {cpass.sum() / max(npass.sum(), 1) / 1e3:.1f} kcycles each, "
          f"{100 * cpass.sum() / tot.sum():.2f} % of the stamped cycles (inside `parallel passes`)")
    if tr_all.shape[1] > 1:
        # row 1, columns 4 and 5: of those cycles, the stage-cost steps (record loads included) and the knot-order sums that
        # are not hidden behind them; what is left is a pass's prologue and epilogue (constants, max reductions, terminal cost)
        # and the caller's accept test
        csteps, csums = tr_all[:, 1, 4], tr_all[:, 1, 5]
        nps = max(npass.sum(), 1)
        print(f"    of a pass: stage-cost steps {csteps.sum() / nps / 1e3:.1f} kcycles, knot-order sums {csums.sum() / nps / 1e3:.1f}, "
              f"prologue + epilogue {(cpass.sum() - csteps.sum() - csums.sum()) / nps / 1e3:.1f}")
    print(f"  executed forward sweeps: {nfw.mean():.2f} per wave, repeated {np.mean(nfw - 1 - it):.3f} (max {int(np.max(nfw - 1 - it))})")
    print("  the ten slowest waves:")
    print("    traj   Mcycles  iterations  sweeps  repeated  cost passes (Mcycles, %)     forward  jacobian   riccati  parallel")
    for t in np.argsort(-tot)[:10]:
        print(f"    {t:4d}  {tot[t]/1e6:8.1f}  {int(it[t]):10d}  {int(nfw[t]):6d}  {int(nfw[t] - 1 - it[t]):8d}  {int(npass[t]):11d} ({cpass[t]/1e6:5.2f}, {100*cpass[t]/tot[t]:4.1f})"
              f"  {tr[t, 0]/1e6:10.1f}  {tr[t, 1]/1e6:8.1f}  {tr[t, 2]/1e6:8.1f}  {tr[t, 3]/1e6:8.1f}")
    print(f"  percentiles of a wave's Mcycles: p50 {np.percentile(tot, 50)/1e6:.1f}, p90 {np.percentile(tot, 90)/1e6:.1f}, p99 {np.percentile(tot, 99)/1e6:.1f}, max {tot.max()/1e6:.1f}")
if one_traj:
    # row 1 of a one-trajectory build: shader cycles and ticks of the 100 MHz counter over the whole solve of the wavefront — the
    # clock it ran at (the chip lowers it under load), as opposed to the GHz-equivalent below, which divides by the KERNEL's time
    cyc, ticks = tr_all[:, 1, 0], tr_all[:, 1, 1]
    ghz = cyc / np.maximum(ticks, 1) * 0.1
    sl = int(np.argmax(tot))
    print(f"  in-kernel clock: median over wavefronts {np.median(ghz):.3f} GHz (min {ghz.min():.3f}, max {ghz.max():.3f}); slowest wavefront "
          f"{ghz[sl]:.3f} GHz ({cyc[sl]/1e6:.1f} Mcycles in {ticks[sl]*1e-5:.2f} ms)")
print(f"  sum of stamped phases {tot.mean()/1e6:.1f} Mcycles/wave = {tot.mean()/ (ms*1e-3)/1e9:.2f} GHz-equivalent of the kernel time")
solver.close()
