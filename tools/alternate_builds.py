"""Developer tool: is one build of the library faster than another on this box, beyond its own run-to-run spread?
Runs a bench workload under two or more builds of libtortoise_hip.so IN TURN — a fresh process per run, the build chosen through
TSAT_LIB (a file name in tortoisesat.jl_amd/csrc), `--pairs` rounds of all builds — so that the chip's temperature and clock
drift fall on every build alike. Reports each build's kernel times (HIP events of the launch, as bench.py's kernel_ms), median and
min-max spread, and for every build after the first whether its median beats the first one's by more than twice that build's spread.

    python tools/alternate_builds.py [--pairs 5] [--workload c1|c2|c3shard] libtortoise_hip_parent.so libtortoise_hip.so ...
    TSAT_LIB=libtortoise_hip.so python tools/alternate_builds.py --child --workload c1      # one run (what rocprofv3 is given)"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def child(workload, reps, warmup):
    from tsat_loader import load_package
    pkg = load_package()
    if os.environ.get("TSAT_LIB"):
        pkg._abi.LIB_NAME = os.environ["TSAT_LIB"]
    from tortoisesat_jl_amd import magnetic as mg, slew_setup as ss, trajopt as to
    solver = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    if workload == "c1":       # bench.py build_workload(1): the headline
        b, precision = ss.workload_monte_carlo(T=1024, N=1000, seed=20190530), 64
    elif workload == "c2":     # bench.py other_configs: configs[2], mixed precision
        b, precision = ss.workload_monte_carlo(T=16384, N=1000, seed=20190531, random_orbit=True, tables=False), 32
    else:                      # the configs[3] shard one of eight GPUs gets
        b, precision = ss.workload_inclination_sweep(T=8192, N=1000, j0=3 * 8192, tables=False), 64
    mg.attach_igrf_tables(solver, b)
    solver.opts.iterations = b.meta["max_outer"]
    solver.opts.opts_uncon.iterations = b.meta["max_inner"]
    solver.opts.opts_uncon.dJ_counter_limit = b.meta["dj_counter_limit"]
    abi = solver.opts.to_abi(b.N, b.n_tab, 3, error_state=1)
    abi.precision = precision
    solver.upload(b, abi.max_linesearch)
    for _ in range(warmup):
        solver.run(abi)
    kms = [solver.run(abi) for _ in range(reps)]
    st = solver.download(want_K=False)["stats"]
    solver.close()
    print(json.dumps({"lib": pkg._abi.LIB_NAME, "workload": workload, "kernel_ms": kms, "inner_iters": int(st["inner_iters"].sum()),
                      "cost_sum": float(st["cost"].sum()), "status": np.bincount(st["status"], minlength=4).tolist()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="timed launches per process")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["c1", "c2", "c3shard"], default="c1")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.workload, args.reps, args.warmup)
    if len(args.libs) < 2:
        ap.error("give at least two builds")
    runs = {lib: [] for lib in args.libs}
    sig = {}
    for r in range(args.pairs):
        for lib in args.libs:
            env = dict(os.environ, TSAT_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--workload", args.workload, "--reps", str(args.reps),
                                "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:          # nothing more is started on the GPU after a failed run
                sys.stderr.write(p.stderr[-2000:])
                raise SystemExit(f"{lib}: run ended with code {p.returncode}")
            d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            runs[lib].append(float(np.mean(d["kernel_ms"])))
            sig.setdefault(lib, (d["inner_iters"], d["cost_sum"], d["status"]))
            print(f"round {r + 1} {lib:36s} kernel_ms {['%.3f' % v for v in d['kernel_ms']]}  mean {runs[lib][-1]:.3f}", flush=True)
    base = args.libs[0]
    print(f"\nworkload {args.workload}: {args.pairs} alternating rounds, {args.reps} launches per process after {args.warmup} warm-up launches")
    for lib in args.libs:
        v = np.array(runs[lib])
        print(f"  {lib:36s} median {np.median(v):8.3f} ms  min {v.min():8.3f}  max {v.max():8.3f}  spread {v.max() - v.min():6.3f} ms "
              f"({100 * (v.max() - v.min()) / np.median(v):.2f} %)   iterations {sig[lib][0]}, statuses {sig[lib][2]}, cost sum {sig[lib][1]!r}")
    b = np.array(runs[base])
    bar = 2 * (b.max() - b.min())
    for lib in args.libs[1:]:
        gain = np.median(b) - np.median(np.array(runs[lib]))
        same = sig[lib] == sig[base]
        print(f"  {lib} against {base}: {gain:+.3f} ms ({100 * gain / np.median(b):+.2f} %), bar 2 x spread of {base} = {bar:.3f} ms: "
              f"{'GAIN' if gain > bar else ('no regression beyond the spread' if gain > -(b.max() - b.min()) else 'REGRESSION')}"
              f"{'' if same else '   RESULTS DIFFER'}")


if __name__ == "__main__":
    main()
