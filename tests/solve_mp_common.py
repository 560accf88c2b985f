"""Shared by tests/test_solve_mp.py (CPU tier: oracle, emulated builds) and tests/test_gpu_solve_mp.py (GPU tier): the cases of
tests/golden/solve_mp.npz — tsat_solve_batch at the horizons where the solve kernels change path (backward
chunks of 64 and 55 knots, packed passes of 16, forward chunks of 32, the two-knot turn), on paths through the AL outer loop, at its
exits and restarts, at the inputs where one knot goes wrong and on one ragged batch — with what the call computes when no operation
rounds (tests/refmath_mp.py::solve_reference, 50 digits, rounded once to float64; written by tests/golden/make_golden_solve_mp.py),
and the assertions every implementation meets on them. Nothing here imports mpmath: the tests read the file.

The bars, per case, trajectory and quantity (X, U, K, the trace columns J_prev, J_new, rho, dV1, dV2, and cost, cost_al, c_max, grad):
  * exact, against the file: status, outer_iters, inner_iters, ls_trials, n_backward, bp_restarts, fp_fails and the trace columns
    outer, inner and accepted index (the script asserts that every decision of the reference keeps a margin of 1e-7);
  * the oracle against the file: |dX| < 1e-9, |dU| < 1e-9 max(1, |U|), |dK| < 1e-9 max(1, |K|), J and dV of the trace to rtol 1e-9, row by row —
    the figures of conftest.assert_same_solution, here against something that shares no formula with the oracle;
  * E_ref = the larger error of two oracle builds against the file (the shipped one and oracle/_ref/liboracle_nofma.so: the same
    source, -ffp-contract=off), measured where the test runs; an implementation (emulator, kernel) is within
    FACTOR[group] max(E_ref, floor) of the file. FACTOR = 4 is the factor of tests/stage_edges_common.py for the same formulas summed in
    another order with another math library; floor = FLOOR_ULPS = 8 units in the last place of the quantity's largest magnitude on
    the trajectory, per knot travelled, per sweep the result has passed through (inner_iters + 1; 1 in group A);
  * the implementation against the oracle: conftest.assert_same_solution, unchanged;
  * zero beyond a ragged horizon; K column 6 zero in error-state mode; every output finite.
A DIVERGED case is held to its status alone (X and U hold the overflowed roll-out), a REG_FAIL case to status, counts, X and U (its K
is the torso of the abandoned sweep).
"""
import functools
import importlib.util
import os
import subprocess

import numpy as np

from conftest import COUNT_FIELDS, assert_same_solution
from helpers import BATCH_FIELDS, OPT_FIELDS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATH = os.path.join(HERE, "golden", "solve_mp.npz")
FLOOR_ULPS, ULP = 8.0, 2.0 ** -52
FACTOR = dict(A=4.0, B=4.0, C=4.0, D=4.0, E=4.0)
ARRAYS = ("X", "U", "K")
TRACE_COLS = dict(J_prev=2, J_new=3, rho=5, dV1=6, dV2=7)
STAT_REALS = ("cost", "cost_al", "c_max", "grad")
QUANTITIES = ARRAYS + tuple(TRACE_COLS) + STAT_REALS
ST_REG_FAIL, ST_DIVERGED = 2, 3
MIXED_BAR = 1e-3          # |dX|, |dU| / scale of the mixed-precision builds


@functools.lru_cache(maxsize=None)
def script():
    """tests/golden/make_golden_solve_mp.py as a module (the CPU test regenerates the short cases with it)"""
    spec = importlib.util.spec_from_file_location("make_golden_solve_mp", os.path.join(HERE, "golden", "make_golden_solve_mp.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def fixture():
    """name -> arrays of the case; never modified"""
    C = {}
    with np.load(PATH) as z:
        for k, v in script().unpack(z).items():
            _, name, field = k.split("/")
            C.setdefault(name, {})[field] = v
    return C


CASE_NAMES = tuple(sorted(fixture()))


def group(name):
    return str(fixture()[name]["group"])


def robust(name):
    return bool(fixture()[name]["robust"])


def n_max(name):
    return int(np.max(fixture()[name]["in_n_knots"])) - 1


def options(name):
    c = fixture()[name]
    return {k: (int(c["opts"][i]) if isinstance(_DEFAULT_TYPES[k], int) else float(c["opts"][i])) for i, k in enumerate(OPT_FIELDS)}


_DEFAULT_TYPES = dict(integrator=3, max_outer=1, max_inner=1, max_linesearch=1, dj_counter_limit=1, cost_tol=0.0, grad_tol=0.0, constraint_tol=0.0,
                      penalty_init=0.0, penalty_scale=0.0, penalty_max=0.0, dual_max=0.0, reg_init=0.0, reg_scale=0.0, reg_min=0.0, reg_max=0.0,
                      reg_fp=0.0, ls_lower=0.0, ls_upper=0.0, max_state=0.0, u_scale=0.0, terminal_mask=1, error_state=1)


def trace_rows(name):
    o = options(name)
    return o["max_outer"] * o["max_inner"]


def case(pkg, ol, name, precision=64):
    """-> (SlewBatch, option block, arrays of the case)"""
    c = fixture()[name]
    nk = c["in_n_knots"]
    N = c["in_U0"].shape[1] + 1
    b = pkg.slew_setup.SlewBatch(N=N, n_tab=c["in_Btab"].shape[1], **{k: np.ascontiguousarray(c[f"in_{k}"]) for k in BATCH_FIELDS},
                                 n_knots=None if np.all(nk == N) else nk.copy())
    o = ol.default_options()
    for k, v in options(name).items():
        setattr(o, k, v)
    o.n_knots, o.n_tab, o.precision = N, b.n_tab, precision
    return b, o, c


# ---- the implementations ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nofma_lib():
    """the oracle built with -ffp-contract=off (every product rounded), by the recipe of oracle/Makefile"""
    import ctypes as C

    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/liboracle_nofma.so"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "liboracle_nofma.so"))
    lib.orc_solve_batch.restype = C.c_int
    return lib


def run_oracle(pkg, ol, name, nofma=False):
    b, o, _ = case(pkg, ol, name)
    return ol.solve_batch(b, o, trace_rows=trace_rows(name), lib=nofma_lib() if nofma else None)


_ORACLES = {}


def oracles(pkg, ol, name):
    """the two oracle builds E_ref is measured on: computed once per case, shared by the tests and left unchanged"""
    if name not in _ORACLES:
        _ORACLES[name] = [run_oracle(pkg, ol, name), run_oracle(pkg, ol, name, nofma=True)]
    return _ORACLES[name]


def run_emu(emu, pkg, ol, name, precision=64):
    b, o, _ = case(pkg, ol, name, precision)
    return emu.solve(b, o, trace_rows=trace_rows(name))


def run_gpu(pkg, ol, solver, name, precision=64):
    """tsat_batch_* on the resident batch, trace rows on"""
    b, o, _ = case(pkg, ol, name, precision)
    solver.upload(b, o.max_linesearch)
    solver.trace(trace_rows(name))
    solver.run(o)
    res = solver.download()
    res["trace"] = solver.trace_download()
    return res


# ---- errors and bars ------------------------------------------------------------------------------------------------------
def compared(name, t):
    """the quantities a trajectory of the case is held to"""
    c = fixture()[name]
    if c["status"][t] == ST_DIVERGED:
        return ()
    if c["status"][t] == ST_REG_FAIL:
        return ("X", "U")
    return QUANTITIES if c["has_K"][t] else tuple(q for q in QUANTITIES if q != "K")


def _pair(c, got, q, t, n):
    if q in ARRAYS:
        m = n if q == "X" else n - 1
        return c[q][t, :m], got[q][t, :m]
    if q in TRACE_COLS:
        r = int(c["n_trace"][t])
        return c["trace"][t, :r, TRACE_COLS[q]], got["trace"][t, :r, TRACE_COLS[q]]
    return np.asarray(c[q][t]), np.asarray(got["stats"][q][t])


def errors(name, got):
    """per trajectory and quantity: (worst absolute error against the file, floor of the bar, largest magnitude)"""
    c = fixture()[name]
    out = []
    for t, n in enumerate(c["in_n_knots"]):
        sweeps = 1 if group(name) == "A" else int(c["inner_iters"][t]) + 1
        row = {}
        for q in compared(name, t):
            ref, g = _pair(c, got, q, t, int(n))
            e = float(np.max(np.abs(g - ref))) if np.all(np.isfinite(g)) else np.inf
            mag = float(np.max(np.abs(ref))) if ref.size else 0.0
            row[q] = (e, FLOOR_ULPS * ULP * mag * (int(n) - 1) * sweeps, mag)
        out.append(row)
    return out


def check_exact(name, got, who):
    c = fixture()[name]
    for f in COUNT_FIELDS:
        assert np.array_equal(got["stats"][f], c[f]), (name, who, f, got["stats"][f].tolist(), c[f].tolist())
    for t in range(len(c["in_n_knots"])):
        r = int(c["n_trace"][t])
        for col in (0, 1, 4):
            assert np.array_equal(got["trace"][t, :r, col], c["trace"][t, :r, col]), (name, who, t, "trace column", col, got["trace"][t, :r, col], c["trace"][t, :r, col])


def check_shape(name, got, who):
    """zero beyond a ragged horizon, K column 6 zero in error-state mode, every output finite"""
    c = fixture()[name]
    for t, n in enumerate(c["in_n_knots"]):
        if c["status"][t] == ST_DIVERGED:
            continue
        assert np.all(got["X"][t, n:] == 0) and np.all(got["U"][t, n - 1:] == 0), (name, who, t, "not zero beyond the horizon")
        assert np.all(np.isfinite(got["X"][t])) and np.all(np.isfinite(got["U"][t])), (name, who, t, "non-finite output")
        for f in STAT_REALS:
            assert np.isfinite(got["stats"][f][t]), (name, who, t, f)
        if c["has_K"][t] and c["status"][t] != ST_REG_FAIL:
            assert np.all(np.isfinite(got["K"][t])) and np.all(got["K"][t, n - 1:] == 0), (name, who, t, "K")
            if options(name)["error_state"]:
                assert np.all(got["K"][t, :, 6, :] == 0), (name, who, t, "K column 6")


def check_oracle(name, ora):
    """the oracle against the file. Returns its errors."""
    check_exact(name, ora, "oracle")
    check_shape(name, ora, "oracle")
    E = errors(name, ora)
    for t, row in enumerate(E):
        for q, (e, _, mag) in row.items():
            if q == "X":
                bar = 1e-9
            elif q in ("U", "K"):
                bar = 1e-9 * max(1.0, mag)
            else:
                continue
            assert e < bar or e == 0.0, (name, "oracle", t, q, e, bar)
    c = fixture()[name]
    for t in range(len(c["in_n_knots"])):                              # J and dV of the trace: rtol 1e-9, row by row
        if compared(name, t) and "J_prev" in compared(name, t):
            r = int(c["n_trace"][t])
            for q in ("J_prev", "J_new", "dV1", "dV2"):
                np.testing.assert_allclose(ora["trace"][t, :r, TRACE_COLS[q]], c["trace"][t, :r, TRACE_COLS[q]], rtol=1e-9, atol=0.0,
                                           err_msg=f"{name} oracle [{t}] {q}")
    return E


def same_as_oracle(name, ora, got):
    """conftest.assert_same_solution on the trajectories that have a solution to compare"""
    c = fixture()[name]
    keep = np.flatnonzero(c["status"] != ST_DIVERGED)
    for f in COUNT_FIELDS:
        assert np.array_equal(ora["stats"][f], got["stats"][f]), (name, f)
    if len(keep):
        pick = lambda r: dict(X=r["X"][keep], U=r["U"][keep], stats=r["stats"][keep])
        assert_same_solution(pick(ora), pick(got))


def check_impl(name, got, ora, who):
    """an implementation against the file, with E_ref the larger error of the given oracle builds; prints the table rows and
    returns the largest share of a bar used"""
    E = errors(name, got)
    Eo = [errors(name, o) for o in ora]
    factor = FACTOR[group(name)]
    lines, worst, bad = [], 0.0, []
    for t, row in enumerate(E):
        for q, (e, floor, _) in row.items():
            e_ref = max(eo[t][q][0] for eo in Eo)
            bar = factor * max(e_ref, floor)
            part = 0.0 if e == 0 else e / bar if bar > 0 else np.inf     # an all-zero quantity: the bar is zero too
            worst = max(worst, part)
            lines.append(f"solve_mp {name}[{t}] {q:7s}: E_ref {' / '.join(f'{eo[t][q][0]:.2e}' for eo in Eo)} floor {floor:.2e} | {who} {e:.2e} "
                         f"bar {bar:.2e} ({part:.2f} of it)")
            if part > 1.0:
                bad.append((t, q, e, bar))
    print("\n".join(lines))
    check_exact(name, got, who)
    check_shape(name, got, who)
    assert not bad, (name, who, bad)
    same_as_oracle(name, ora[0], got)
    return worst


def check_mixed(name, got, who):
    """a mixed-precision build (float linearisation) on a robust case: the file's statuses, counts and accepted indices, and
    SURVEY §8d's 1e-3 on X and on U / scale; prints the errors"""
    assert robust(name), name
    check_exact(name, got, who)
    check_shape(name, got, who)
    c = fixture()[name]
    for t, n in enumerate(c["in_n_knots"]):
        dX = float(np.max(np.abs(got["X"][t, :n] - c["X"][t, :n])))
        dU = float(np.max(np.abs(got["U"][t, :n - 1] - c["U"][t, :n - 1]))) / max(1.0, float(np.max(np.abs(c["U"][t, :n - 1]))))
        print(f"solve_mp {name}[{t}] {who}: |dX| {dX:.2e} |dU| / scale {dU:.2e} (bar {MIXED_BAR:.0e})")
        assert dX < MIXED_BAR and dU < MIXED_BAR, (name, who, t, dX, dU)
