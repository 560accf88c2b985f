"""Shared by the cost-pass tests (CPU tier: test_cost_pass.py, GPU tier: test_gpu_cost_pass.py): the inputs and their oracle
solves with the per-iteration trace, computed once per session."""
import numpy as np

import line_search_common as lsc
from conftest import oracle_options

# N - 1: a lone knot, two; 63 | 64 | 65 around a 64-knot step; 255 | 256 | 257 around a summed block; 320: a last block of one step
RAGGED = (2, 3, 64, 65, 66, 256, 257, 258, 321)

_cases = {}


def cached(key, make):
    """an input and its oracle solve, computed once and left unchanged"""
    if key not in _cases:
        b, o, ref = make()
        for a in (ref["X"], ref["U"], ref["K"], ref["stats"], ref["trace"]):
            a.setflags(write=False)
        _cases[key] = (b, o, ref)
    return _cases[key]


def ragged_case(pkg, ol):
    def make():
        b = pkg.slew_setup.workload_monte_carlo(T=len(RAGGED), N=max(RAGGED), seed=811)
        b.n_knots = np.array(RAGGED, dtype=np.int32)
        o = oracle_options(ol, max_outer=2, max_inner=3, dj_counter_limit=1, error_state=1)
        return b, o, ol.solve_batch(b, o, nthreads=4, trace_rows=16)
    return cached("ragged", make)


def odd_case(pkg, ol, max_ls):
    def make():
        b = pkg.slew_setup.workload_monte_carlo(T=4, N=300, seed=811)
        o = oracle_options(ol, max_outer=2, max_inner=4, dj_counter_limit=1, error_state=1, max_linesearch=max_ls)
        return b, o, ol.solve_batch(b, o, nthreads=4, trace_rows=16)
    return cached(("odd", max_ls), make)


BOUND = 20.0      # |u| reaches 20 .. 29 on these slews (units of u_scale), |x| < 1: the bound cuts into the first candidates' controls


def bound_case(pkg, ol):
    def make():
        b = pkg.slew_setup.workload_monte_carlo(T=6, N=70, seed=20190530)
        o = oracle_options(ol, max_outer=2, max_inner=5, dj_counter_limit=1, error_state=1, max_state=BOUND)
        return b, o, ol.solve_batch(b, o, nthreads=4, trace_rows=16)
    return cached("bound", make)


def both_lanes_case(pkg, ol):
    """the fewest trajectories of line_search_common.case whose searches end on every index that occurs there"""
    b, o, ref = lsc.case(pkg, ol)
    want, idx = set(range(17)) | {18}, []
    while want:
        t = max(range(lsc.T), key=lambda t: (len(want & set(lsc.accepted_indices(ref, t).tolist())), -int(ref["stats"]["inner_iters"][t])))
        got = want & set(lsc.accepted_indices(ref, t).tolist())
        assert got, want
        idx.append(t)
        want -= got
    idx.sort()
    sub = dict(X=ref["X"][idx], U=ref["U"][idx], K=ref["K"][idx], stats=ref["stats"][idx])
    return lsc.pick(pkg, b, idx), o, sub
