"""Developer tool (CPU): the keep rule of the one-trajectory builds' line search (tsat_set_store_policy) replayed on the
oracle's line-search trace of the headline batch (bench.py configs[1]: 1024 x 1000, IGRF tables, 5 x 10) — repeated forward
sweeps, kept roll-outs per sweep (the HBM writes) and a cycle model of the slowest wavefront under several policies. The
model prices a backward sweep at 1594, a forward sweep at 1526 and a cost pass at 50 kcycles (profiles/r04/phase_clocks_final.txt;
the last one assumed). Takes a few minutes of oracle time.   python tools/keep_rule_replay.py > profiles/line_search/keep_rule_replay.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
import numpy as np
from tsat_loader import load_package
pkg = load_package()
import oracle_lib as ol
ol.build(); ol.load()
import line_search_common as lsc
ss = pkg.slew_setup
b = ss.workload_monte_carlo(T=1024, N=1000, seed=20190530)
kep = np.atleast_2d(np.asarray(b.meta["kep"], dtype=np.float64))
N, dt = b.N, float(b.dt[0])
rows = min(2 * N, N + 8)
B, _ = ol.btable_batch(kep, 0.0, N * dt, N, want_pos=False)
b.Btab = np.ascontiguousarray(B[:, :rows]); b.n_tab = rows
b.btab_idx = np.zeros(b.T, np.int32) if kep.shape[0] == 1 else np.arange(b.T, dtype=np.int32)
b.tau0[:] = 0.0; b.dtau[:] = 1.0
o = ol.default_options()
o.max_outer, o.max_inner, o.dj_counter_limit, o.error_state = 5, 10, 1, 1
ref = ol.solve_batch(b, o, nthreads=min(16, ol.num_procs()), want_K=False, trace_rows=64)
st = ref["stats"]
print("mean inner", st["inner_iters"].mean(), "mean ls_trials", st["ls_trials"].mean())
it = st["inner_iters"]
# cycles model of the issue: backward 1594 k, forward 1526 k, cost pass 50 k (assumed)
def model(few, hold, slots):
    rep, kept, tot = [], [], []
    for t in range(b.T):
        jws = lsc.accepted_indices(ref, t)
        n, since, k, passes = 1, lsc.NEVER_DEEP, 0, 0
        n_slots = min(20, slots)
        for jw in jws:
            keep_all = since < lsc.NEVER_DEEP if hold < 0 else since <= hold
            n_store = n_slots if (keep_all or n_slots < few) else few
            shift = 0
            while shift < 20:
                n += 1
                here = min(20 - shift, n_store); k += here
                hit = 0 <= jw < shift + here
                last = (jw - shift) if hit else here - 1
                passes += last // 2 + 1
                if hit: break
                shift, n_store = shift + n_store, n_slots
            if jw < 0 or jw >= few - 1: since = 0
            elif since < lsc.NEVER_DEEP: since += 1
        rep.append(n - 1 - len(jws)); kept.append(k / max(n - 1, 1))
        tot.append((len(jws) * 1594 + n * 1526 + passes * 50) / 1e3)
    rep, tot = np.array(rep), np.array(tot)
    return rep.mean(), rep.max(), np.mean(kept), tot.mean(), tot.max(), int(it[np.argmax(tot)]), int(rep[np.argmax(tot)])
print("policy (few, hold, slots): repeated sweeps mean / max | kept roll-outs per sweep | modelled Mcycles mean, slowest (its iterations, its repeated sweeps)")
for name, p in (("parent (4, 0) on 12 slots", (4, 0, 12)), ("(4, 0) on 20", (4, 0, 20)), ("(4, 3)", (4, 3, 20)), ("(4, 8)", (4, 8, 20)), ("(4, 15)", (4, 15, 20)),
                ("(4, sticky)", (4, -1, 20)), ("keep all", (20, 0, 20)), ("always 12", (12, 0, 12))):
    r = model(*p)
    print(f"  {name:26s}: {r[0]:.3f} / {r[1]:2d} | {r[2]:5.2f} | {r[3]:.1f}, {r[4]:.1f} ({r[5]}, {r[6]})")
a = np.concatenate([lsc.accepted_indices(ref, t) for t in range(b.T)])
print("accepted index shares:", {k: round(float(np.mean(a == k)), 4) for k in range(0, 6)}, ">=4", float(np.mean(a >= 4)), ">=12 or failed", float(np.mean((a >= 12) | (a < 0))))
