"""GPU tier (`pytest -m gpu`): the closed-loop forward sweep of the wide build takes a knot's gains K, d through DPP — every
lane reads one 16-byte unit of the staged record, and `v_fmac_f64_dpp row_newbcast:n` names the lane that holds a term's
multiplicand (TSAT_FG_6 / TSAT_FG_7, tsat_riccati_dpp.inc) — instead of eleven wave-uniform LDS reads a knot. The terms run in the
order of the plain loop, so nothing a solve returns may move by a bit: the wide build, and the dense build, whose sweep keeps the
broadcast reads, are compared, bit for bit, with the packed4w build forced onto the same batch, whose forward sweep is other code
(tsat_packed.hpp: a trajectory is a DPP row there; its endgame is off, so that no trajectory is handed to the one-trajectory
mapping), and with the oracle at the fp64 bar.

The forward chunk is 32 knots and a turn of the loop two: N - 1 = 1 (one knot), 2 (a whole turn), 3 (an odd tail), 32 (exactly one
chunk), 33 (a chunk and one knot: the lane address of a second chunk buffer) and 65 (two chunks and one knot: back in the first
buffer); full state (seven gain columns a row, TSAT_FG_7) and error state (six, TSAT_FG_6)."""
import numpy as np
import pytest

import helpers
from conftest import assert_same_solution, oracle_options

pytestmark = pytest.mark.gpu

WIDE, DENSE, PACKED4W = 1, 2, 7          # tsat_set_kernel_variant
T = 4
LENGTHS = (2, 3, 4, 33, 34, 66)
CASES = [(n, es, 3) for es in (0, 1) for n in LENGTHS] + [(34, 1, 4)]


@pytest.fixture(scope="module")
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


_case = {}


def case(pkg, ol, solver, n, es, integ):
    """batch, oracle result and packed4w result of a case: computed once, left unchanged"""
    key = (n, es, integ)
    if key not in _case:
        b = pkg.slew_setup.workload_monte_carlo(T=T, N=n, seed=4100 + 10 * n + es, degenerate_rd=0.03)
        o = oracle_options(ol, max_outer=2, max_inner=3, dj_counter_limit=1, error_state=es, integrator=integ)
        ref = ol.solve_batch(b, o)
        packed = solve(pkg, solver, b, o, PACKED4W)
        for r in (ref, packed):
            for k in ("X", "U", "K", "stats"):
                if k in r:
                    r[k].setflags(write=False)
        _case[key] = (b, o, ref, packed)
    return _case[key]


@pytest.mark.parametrize("variant", [WIDE, DENSE])
@pytest.mark.parametrize("n,es,integ", CASES)
def test_gpu_forward_gains_through_dpp(pkg, ol, solver, variant, n, es, integ):
    b, o, ref, packed = case(pkg, ol, solver, n, es, integ)
    assert ref["stats"]["ls_trials"].sum() > 0           # closed-loop sweeps ran
    got = solve(pkg, solver, b, o, variant)
    # bit for bit with the packed4w build: X, U, K and every statistic except n_forward
    for k in ("X", "U"):
        assert np.array_equal(packed[k], got[k]), k
    for f in packed["stats"].dtype.names:
        assert f == "n_forward" or np.array_equal(packed["stats"][f], got["stats"][f]), f
    ok = packed["stats"]["status"] != pkg._abi.TSAT_REG_FAIL      # (K is undefined where a solve ended REG_FAIL)
    assert np.array_equal(packed["K"][ok], got["K"][ok]), "K"
    # and each build at the short-budget bar of the oracle: equal counts, |dX| < 1e-9, |dU| < 1e-9 of the control scale
    assert_same_solution(ref, packed)
    assert_same_solution(ref, got)
