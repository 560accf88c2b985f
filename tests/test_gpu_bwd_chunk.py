"""GPU tier (`pytest -m gpu`): the backward sweep of the wide build runs the Jacobian lanes of a chunk inlined into
backward_sweep (no register save per chunk), so the chunk loop, the Jacobian lanes and the call of riccati_rows share one register
allocation: the chunk bounds, the accumulated expected reductions and the restart flag now live in backward_sweep's registers
across the Jacobian lanes of every chunk. None of it may change a bit: the wide and the dense build are compared with
the oracle at the fp64 bar and, bit for bit, with the packed4w build forced onto the same batch, whose backward sweep is other code
(tsat_packed.hpp; its endgame is off, so that no trajectory is handed to the one-trajectory mapping). The horizons sit on the
edges of the backward chunk — 64 knots with the error state, 55 in the full state — and of the two-knot turn inside it; the
restart cases drive failing sweeps across a chunk boundary with the store guard in force."""
import numpy as np
import pytest

import helpers
from conftest import assert_same_solution, oracle_options

pytestmark = pytest.mark.gpu

WIDE, DENSE, PACKED4W = 1, 2, 7          # tsat_set_kernel_variant


@pytest.fixture()
def solver(pkg):
    import torch

    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    s = pkg.trajopt.AugmentedLagrangianSolver(None, None, device=0)
    yield s
    s.close()


def solve(pkg, solver, b, o, variant):
    a = helpers.abi_options_like(o, pkg, b.N, b.n_tab)
    solver.set_kernel_variant(variant)
    solver.set_endgame(0)
    solver.upload(b, a.max_linesearch)
    solver.run(a)
    return solver.download()


def same_bits(a, b, what, abi):
    """X, U and every statistic except n_forward, bit for bit; K where the solve did not end REG_FAIL (there it is undefined)"""
    for k in ("X", "U"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for f in a["stats"].dtype.names:
        assert f == "n_forward" or np.array_equal(a["stats"][f], b["stats"][f]), (what, f)
    ok = a["stats"]["status"] != abi.TSAT_REG_FAIL
    assert np.array_equal(a["K"][ok], b["K"][ok]), (what, "K")


T = 4
# (error_state, N - 1, integrator, indefinite Rd on the second half of the batch)
CASES = ([(1, n, 3, False) for n in (1, 2, 63, 64, 65, 129)]      # one knot | a whole turn | the odd knot | one chunk | a second call
         + [(0, n, 3, False) for n in (54, 55, 56, 111)]          # of one knot | three calls, odd;  full state: 55-knot chunks
         + [(1, 65, 4, False)]
         + [(1, n, 3, True) for n in (65, 129)])
_cache = {}


def case(pkg, ol, solver, key):
    """(batch, options, oracle result, packed4w result) of a case, computed once and left unchanged"""
    if key not in _cache:
        es, n, integ, indefinite = key
        b = pkg.slew_setup.workload_monte_carlo(T=T, N=n + 1, seed=900 + n + 1000 * es, degenerate_rd=0.03 if indefinite else None)
        if indefinite:
            b.Rd[T // 2:, 2] = -1e-4
        o = oracle_options(ol, max_outer=2, max_inner=3, dj_counter_limit=1, error_state=es, integrator=integ)
        ref = ol.solve_batch(b, o, nthreads=4)
        packed = solve(pkg, solver, b, o, PACKED4W)
        for r in (ref, packed):
            for a in (r["X"], r["U"], r["K"], r["stats"]):
                a.setflags(write=False)
        _cache[key] = (b, o, ref, packed)
    return _cache[key]


@pytest.mark.parametrize("variant", [WIDE, DENSE])
@pytest.mark.parametrize("key", CASES, ids=lambda k: f"es{k[0]}-n{k[1]}-rk{k[2]}{'-indef' if k[3] else ''}")
def test_gpu_bwd_chunk_edges(pkg, ol, solver, variant, key):
    b, o, ref, packed = case(pkg, ol, solver, key)
    if key[3]:
        assert ref["stats"]["bp_restarts"].sum() > 0        # sweeps fail and restart at this length
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)                          # equal counts, |dX|, |dU| < 1e-9 of the control scale
    assert np.array_equal(ref["stats"]["bp_restarts"], got["stats"]["bp_restarts"])
    same_bits(packed, got, (key, variant), pkg._abi)
