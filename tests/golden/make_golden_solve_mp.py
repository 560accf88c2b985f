#!/usr/bin/env python3
"""Generates tests/golden/solve_mp.npz: inputs of every case of tests/solve_mp_common.py and what tsat_solve_batch computes on them
when no operation rounds — tests/refmath_mp.py::solve_reference at 50 digits, rounded once to the nearest float64 (X, U, K of the
last successful backward sweep, every field of tsat_stats, the trace rows).

Inputs are slew_setup.workload_monte_carlo batches (degenerate_rd = 0.03, as the ragged tests have it) at the horizons where the
solve kernels change path, edited per case as the case says. Nothing is workload size; n below is N - 1.

Every comparison the solve takes is taken by the reference in its own arithmetic and recorded with its margin (solve_reference).
The file holds one array per field, the cases end to end (pack / unpack below).

The script asserts min_margin >= MARGIN on every trajectory (ROBUST on the cases marked robust, which the mixed-precision builds
run): every float64 implementation is then held to the file's statuses, counts and accepted indices exactly. Exempt are the
decisions that are ties by construction of the input, the same in any arithmetic (solve_reference counts them under `exact`):
  * a table argument (k + c) dtau + tau0 that is an integer (dtau = 1 of the workloads, the case dtau = 0.5 / tau0 = 2);
  * a U0 component set equal to uhi or ulo: c == 0, and lambda + mu c == 0 in the dual update that follows if it is still there;
  * dJ == 0 after a line search that accepted nothing: J is J_prev itself.

    python tests/golden/make_golden_solve_mp.py [-j P]            write the file (P processes)
    python tests/golden/make_golden_solve_mp.py --check [-j P]    regenerate everything and require bit equality with the file
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]
import numpy as np  # noqa: E402

from helpers import BATCH_FIELDS, OPT_FIELDS  # noqa: E402

PATH = os.path.join(HERE, "solve_mp.npz")
MARGIN, ROBUST = 1e-7, 1e-3
INT_OPTS = ("integrator", "max_outer", "max_inner", "max_linesearch", "dj_counter_limit", "terminal_mask", "error_state")
DEFAULTS = dict(integrator=3, max_outer=20, max_inner=50, max_linesearch=20, dj_counter_limit=10, cost_tol=1e-4, grad_tol=1e-5,
                constraint_tol=1e-3, penalty_init=1.0, penalty_scale=10.0, penalty_max=1e8, dual_max=1e8, reg_init=0.0, reg_scale=1.6,
                reg_min=1e-8, reg_max=1e8, reg_fp=10.0, ls_lower=1e-8, ls_upper=10.0, max_state=1e8, u_scale=1e-2, terminal_mask=0x7F,
                error_state=0)                                     # tsat_default_options
STAT_INTS = ("status", "outer_iters", "inner_iters", "ls_trials", "n_backward", "n_forward", "bp_restarts", "fp_fails")
STAT_REALS = ("cost", "cost_al", "c_max", "grad")
J_KINDS = (None,                                                   # the workload's own: isotropic 1U
           np.diag([0.0011, 0.00125, 0.0016]) * 4.0,               # diagonal (3U-like)
           np.array([[0.00125, 1.2e-4, -0.8e-4], [1.2e-4, 0.0014, 0.6e-4], [-0.8e-4, 0.6e-4, 0.0011]]) * 2.0)      # full tensor
RAGGED = [97, 2, 3, 16, 17, 18, 33, 5, 96, 49, 64, 65, 4]          # tests/test_gpu_parity.py::test_gpu_packed_builds_ragged_and_tiny_horizons
# max_state of the case C_max_state: between the largest |x|, |u| of the first candidate (alpha = 1) and of the second, asserted below
C_MAX_STATE = 3000.0


def opts_vec(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return np.array([float(o[k]) for k in OPT_FIELDS])


def opts_dict(v):
    return {k: (int(v[i]) if k in INT_OPTS else float(v[i])) for i, k in enumerate(OPT_FIELDS)}


def build_cases(pkg):
    """name -> dict(group, robust, b (SlewBatch), opts (vector in the order of helpers.OPT_FIELDS))"""
    ss = pkg.slew_setup
    C = {}

    def mc(n, seed, T=1):
        return ss.workload_monte_carlo(T=T, N=n + 1, seed=seed, degenerate_rd=0.03)

    def add(name, group, b, robust=False, **o):
        assert name not in C
        C[name] = dict(group=group, robust=robust, b=b, opts=opts_vec(**o))

    def inertia(b, kind):
        if J_KINDS[kind] is not None:
            b.Jmat[:] = ss.jmat_cm(J_KINDS[kind])
        return b

    one = dict(max_outer=1, max_inner=1)
    # ---- A: one sweep ----------------------------------------------------------------------------------------------------
    for n in (1, 2, 63, 64, 65, 129, 15, 16, 32, 33):              # (n = 17: the cross product below)
        add(f"A_es1_rk3_n{n}", "A", mc(n, 1000 + n), robust=n in (1, 32, 64, 65), error_state=1, **one)
    for es in (0, 1):                                              # the two-knot turn once more with a control weight of ordinary size:
        b = mc(1, 1201 + es)                                       # the workload's Bryson R of a two-knot guess is 3e20, K 1e-24
        b.Rd[:] = 0.03
        b.U0 *= 1e4                                              # controls of U(0, 10), inside the box: the step moves the cost by more than the margin
        add(f"A_es{es}_rk3_n1_rd", "A", b, error_state=es, **one)
    for n in (54, 55, 56, 111):
        add(f"A_es0_rk3_n{n}", "A", mc(n, 1000 + n), robust=n in (54, 56), error_state=0, **one)
    add("A_es1_rk4_n65", "A", mc(65, 1165), robust=True, error_state=1, integrator=4, **one)
    add("A_es0_rk4_n56", "A", mc(56, 1156), error_state=0, integrator=4, **one)
    for jk in range(3):
        for es in (0, 1):
            for integ in (3, 4):
                add(f"A17_J{jk}_es{es}_rk{integ}", "A", inertia(mc(17, 1017), jk), error_state=es, integrator=integ, **one)
    # ---- B: paths ----------------------------------------------------------------------------------------------------------
    path = dict(max_outer=2, max_inner=3, dj_counter_limit=1)

    def outside(b, scale):
        """controls of U(0, 1e-3 scale): some outside the box of 19; one exactly on uhi, one exactly on ulo"""
        b.U0 *= scale
        b.U0[0, min(3, b.N - 2), 0] = b.uhi[0, 0]
        b.U0[0, min(5, b.N - 2), 1] = b.ulo[0, 1]
        return b

    add("B_n17_mask0", "B", outside(mc(17, 2017), 3e4), error_state=1, terminal_mask=0, **path)
    add("B_n33_maskq", "B", outside(mc(33, 2033), 3e4), error_state=1, terminal_mask=0b1111000, **path)
    add("B_n65_mask7f", "B", outside(mc(65, 2065), 3e4), error_state=1, terminal_mask=0b1111111, **path)
    add("B_n56_es0", "B", outside(mc(56, 2156), 3e4), error_state=0, terminal_mask=0b1111111, **path)
    add("B_n17_clamps", "B", outside(mc(17, 2300), 3e4), error_state=1, dual_max=2.0, penalty_max=4.0, **path)
    add("B_n17_penalty", "B", outside(mc(17, 2301), 3e4), error_state=1, penalty_init=10.0, penalty_scale=3.0, **path)
    # ---- C: exits and restarts ---------------------------------------------------------------------------------------------
    for n in (65, 129):
        b = mc(n, 3000 + n)
        b.Rd[0, 1] = -1e-4
        add(f"C_negR_n{n}", "C", b, error_state=1, max_outer=1, max_inner=2)
    add("C_ls1_n17", "C", mc(17, 3017), error_state=1, max_linesearch=1, reg_fp=1e-6, max_outer=1, max_inner=5, dj_counter_limit=1)
    add("C_max_state_n17", "C", outside(mc(17, 3117), 3e4), error_state=1, max_state=C_MAX_STATE, max_outer=1, max_inner=2)
    add("C_cost_tol_n17", "C", mc(17, 3217), error_state=1, cost_tol=1e6, max_outer=2, max_inner=3, dj_counter_limit=1)
    add("C_grad_tol_n17", "C", mc(17, 3317), error_state=1, grad_tol=1e9, max_outer=2, max_inner=3, dj_counter_limit=1)
    b = mc(17, 3417)
    b.Rd[0, 1] = -1e-4
    add("C_reg_fail_n17", "C", b, error_state=1, reg_max=1e-6, max_outer=2, max_inner=3)
    b = mc(17, 3517)
    b.U0[:] = 1e12
    add("C_diverged_n17", "C", b, error_state=1, max_outer=2, max_inner=3)
    # ---- D: inputs where one knot goes wrong -------------------------------------------------------------------------------
    knot = dict(max_outer=1, max_inner=2)

    def d_case(name, seed, edit, **o):
        b = mc(17, seed)
        edit(b)
        add(name, "D", b, **dict(knot, **o))

    def neg_scalar(b):
        if b.x0[0, 3] > 0:
            b.x0[0, 3:] *= -1.0

    def scale_q(s):
        def f(b):
            b.x0[0, 3:] *= s
        return f

    def zero_inputs(b):
        b.x0[0, :3] = 0.0
        b.U0[:] = 0.0

    def zero_row(b):
        b.Btab[0, 8] = 0.0

    def clock(dtau, tau0):
        def f(b):
            b.dtau[:], b.tau0[:] = dtau, tau0
        return f

    def zero_r(b):
        b.Rd[0, 2] = 0.0

    d_case("D_neg_scalar", 4001, neg_scalar, error_state=1)
    d_case("D_qnorm_half", 4002, scale_q(0.5), error_state=1)
    d_case("D_qnorm_two", 4003, scale_q(2.0), error_state=0)
    d_case("D_zero_rate_u0", 4004, zero_inputs, error_state=1)
    d_case("D_zero_field_row", 4005, zero_row, error_state=1)
    d_case("D_dtau_037", 4006, clock(0.37, 3.2), error_state=1)
    d_case("D_dtau_19_clamped", 4007, clock(1.9, 0.0), error_state=0)
    d_case("D_dtau_half_exact", 4008, clock(0.5, 2.0), error_state=1)
    d_case("D_zero_Rd", 4009, zero_r, error_state=1)
    # ---- E: one ragged batch -----------------------------------------------------------------------------------------------
    for es in (0, 1):
        b = mc(96, (45, 48)[es], T=13)
        b.n_knots = np.array(RAGGED, dtype=np.int32)
        for t, n in enumerate(RAGGED):
            b.U0[t, n - 1:] = 0.0                                  # ignored beyond a trajectory's horizon
        add(f"E_ragged_es{es}", "E", b, error_state=es, max_outer=2, max_inner=2, dj_counter_limit=1)
    return C


def n_knots(b):
    return np.full(b.T, b.N, dtype=np.int32) if b.n_knots is None else np.asarray(b.n_knots, dtype=np.int32)


def trace_rows(opts):
    o = opts_dict(opts)
    return o["max_outer"] * o["max_inner"]


def compute_traj(arg):
    """the 50-digit results of one trajectory, rounded to float64"""
    import refmath_mp as rmp          # mpmath is needed here alone: the tests that only read the file never import it

    b, t, N, opts = arg
    o = opts_dict(opts)
    ref = rmp.solve_reference(b["x0"][t], b["xf"][t], b["Btab"][b["btab_idx"][t]], b["tau0"][t], b["dtau"][t], b["dt"][t], b["Jmat"][t],
                              b["Qd"][t], b["Qfd"][t], b["Rd"][t], b["ulo"][t], b["uhi"][t], b["U0"][t, :N - 1], trace_rows=trace_rows(opts), **o)
    f = lambda a: np.array(a, dtype=object).astype(np.float64)          # mpf -> nearest float64
    out = dict(X=f(ref["X"]), U=f(ref["U"]), K=None if ref["K"] is None else f(ref["K"]),
               trace=f(ref["trace"]).reshape(-1, 8), margin=float(ref["min_margin"]), margins={k: float(v) for k, v in ref["margins"].items()},
               exact=ref["exact"], ls_log=ref["ls_log"])
    for k in STAT_INTS:
        out[k] = int(ref["stats"][k])
    for k in STAT_REALS:
        out[k] = float(ref["stats"][k])
    return out


def batch_arrays(b):
    d = {k: np.ascontiguousarray(getattr(b, k)) for k in BATCH_FIELDS}
    d["n_knots"] = n_knots(b)
    return d


def assemble(case, per_traj):
    """results of a case in the shapes of the ABI wrappers, zero beyond a ragged horizon"""
    b = case["b"]
    T, N, R = b.T, b.N, trace_rows(case["opts"])
    out = dict(X=np.zeros((T, N, 7)), U=np.zeros((T, N - 1, 3)), K=np.zeros((T, N - 1, 7, 3)), trace=np.zeros((T, R, 8)),
               n_trace=np.zeros(T, dtype=np.int32), has_K=np.zeros(T, dtype=np.int32), margin=np.zeros(T))
    for k in STAT_INTS:
        out[k] = np.zeros(T, dtype=np.int32)
    for k in STAT_REALS:
        out[k] = np.zeros(T)
    for t, (n, r) in enumerate(zip(n_knots(b), per_traj)):
        out["X"][t, :n], out["U"][t, :n - 1] = r["X"], r["U"]
        if r["K"] is not None:
            out["K"][t, :n - 1], out["has_K"][t] = r["K"], 1
        out["trace"][t, :len(r["trace"])], out["n_trace"][t], out["margin"][t] = r["trace"], len(r["trace"]), r["margin"]
        for k in STAT_INTS + STAT_REALS:
            out[k][t] = r[k]
    return out


def check_case(name, case, per_traj):
    need = ROBUST if case["robust"] else MARGIN
    for t, r in enumerate(per_traj):
        assert r["margin"] >= need, (name, t, "a decision sits within the margin: change the inputs (seed, scale)", r["margins"])


def generate(pkg, only=None, procs=1, log=print):
    C = build_cases(pkg)
    names = [n for n in C if only is None or n in only]
    tasks = [(n, batch_arrays(C[n]["b"]), t, int(nk), C[n]["opts"]) for n in names for t, nk in enumerate(n_knots(C[n]["b"]))]
    tasks.sort(key=lambda a: -a[3] * trace_rows(a[4]))
    t0 = time.time()
    if procs > 1:
        import multiprocessing as mpr

        with mpr.get_context("fork").Pool(procs) as pool:
            res = pool.map(compute_traj, [a[1:] for a in tasks], chunksize=1)
    else:
        res = [compute_traj(a[1:]) for a in tasks]
    per = {n: [None] * C[n]["b"].T for n in names}
    for a, r in zip(tasks, res):
        per[a[0]][a[2]] = r
    results = {}
    for n in names:
        results[n] = assemble(C[n], per[n])
        r = results[n]
        kinds = {}
        for p in per[n]:
            for k, v in p["margins"].items():
                kinds[k] = min(kinds.get(k, np.inf), v)
        worst = min(kinds, key=kinds.get)
        log(f"{n:22s} knots {n_knots(C[n]['b']).tolist()} margin {r['margin'].min():.2e} ({worst}{'' if len(per[n]) == 1 else ' ' + ' '.join(f'{m:.0e}' for m in r['margin'])}) status {r['status'].tolist()} inner {r['inner_iters'].tolist()} "
            f"ls {r['ls_trials'].tolist()} restarts {r['bp_restarts'].tolist()} fp_fails {r['fp_fails'].tolist()} accepted {[int(x) for x in r['trace'][0, :r['n_trace'][0], 4]]}")
    log(f"{len(tasks)} trajectories of {len(names)} cases in {time.time() - t0:.0f} s")
    for n in names:
        check_case(n, C[n], per[n])
    return C, results, per


def expectations(results, per):
    """what the cases are there for"""
    R = results
    for n in ("C_negR_n65", "C_negR_n129"):
        assert R[n]["bp_restarts"][0] > 0 and R[n]["status"][0] != 2 and R[n]["inner_iters"][0] == 2, n
    r = R["C_ls1_n17"]
    assert r["fp_fails"][0] == 2 and r["inner_iters"][0] == 2 and r["ls_trials"][0] == 2, "first candidates rejected, then the dJ == 0 counter"
    log = per["C_max_state_n17"][0]["ls_log"]
    first = [e for e in log if e[0] == 1 and e[1] == 1]
    assert not first[0][3] and first[0][4] > C_MAX_STATE and first[1][3] and first[1][4] < C_MAX_STATE, first[:2]
    for n in ("C_cost_tol_n17", "C_grad_tol_n17"):
        assert R[n]["inner_iters"][0] == R[n]["outer_iters"][0] == 2, n
    assert R["C_reg_fail_n17"]["status"][0] == 2 and R["C_diverged_n17"]["status"][0] == 3 and R["C_diverged_n17"]["n_backward"][0] == 0
    r = R["B_n17_clamps"]                                          # a control further outside than dual_max / penalty_init; 10 > penalty_max
    assert r["outer_iters"][0] == 2 and r["c_max"][0] > 2.0
    for n in R:
        if n[0] == "B":
            assert per[n][0]["exact"].get("active_set", 0) >= 2, (n, "the two controls on their bounds")


def flatten(C, results):
    """name of an array ("c/<case>/<field>") -> array"""
    d = {}
    for n, c in C.items():
        for k, v in batch_arrays(c["b"]).items():
            d[f"c/{n}/in_{k}"] = v
        d[f"c/{n}/opts"], d[f"c/{n}/group"], d[f"c/{n}/robust"] = c["opts"], np.array(c["group"]), np.array(int(c["robust"]), dtype=np.int32)
        for k, v in results[n].items():
            d[f"c/{n}/{k}"] = v
    return d


def pack(d):
    """the arrays of the file: per field ONE array, the cases' values raveled end to end, beside the cases' names and the shapes
    (a file of two thousand small arrays spends more bytes on their headers than on their values)"""
    names = sorted({k.split("/")[1] for k in d})
    fields = sorted({k.split("/")[2] for k in d})
    out = {"names": np.array(names)}
    for f in fields:
        vs = [np.asarray(d[f"c/{n}/{f}"]) for n in names]
        assert len({v.dtype for v in vs}) == 1 and all(v.ndim <= 4 for v in vs), f
        out[f"v/{f}"] = np.concatenate([v.ravel() for v in vs])
        out[f"s/{f}"] = np.array([list(v.shape) + [-1] * (4 - v.ndim) for v in vs], dtype=np.int32)
    return out


def unpack(z):
    """pack() undone: name of an array -> array"""
    names = [str(n) for n in z["names"]]
    d = {}
    for key in z.files:
        if not key.startswith("v/"):
            continue
        f = key[2:]
        flat, shapes, at = z[key], z[f"s/{f}"], 0
        for n, sh in zip(names, shapes):
            sh = tuple(int(x) for x in sh if x >= 0)
            size = int(np.prod(sh, dtype=np.int64))
            d[f"c/{n}/{f}"] = flat[at:at + size].reshape(sh)
            at += size
    return d


if __name__ == "__main__":
    from tsat_loader import load_package

    pkg = load_package()
    procs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else 1
    t0 = time.time()
    only = None if "--only" not in sys.argv else [n for n in build_cases(pkg) if n.startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
    C, results, per = generate(pkg, only=only, procs=procs)
    if only is not None:
        sys.exit(0)                                                 # a look at some cases: nothing is written
    expectations(results, per)
    d = pack(flatten(C, results))
    if "--check" in sys.argv:
        z = np.load(PATH)
        assert sorted(z.files) == sorted(d), "the file and the script hold different arrays"
        for k, v in d.items():
            assert np.asarray(v).tobytes() == z[k].tobytes() and np.asarray(v).shape == z[k].shape, k
        print(f"check: {len(d)} arrays of {len(C)} cases regenerated bit for bit in {time.time() - t0:.0f} s")
    else:
        np.savez_compressed(PATH, **d)
        print(f"tests/golden/solve_mp.npz: {os.path.getsize(PATH)} bytes, {len(C)} cases, {time.time() - t0:.0f} s")
