"""GPU tier (`pytest -m gpu`): the line search's cost pass (candidate_costs in tsat_device.hpp) on the wide and the dense build,
the batches of the CPU tier (test_cost_pass.py). Each solve is held to two references: the oracle at the fp64 bar, and, bit for
bit, the packed4w build forced onto the same batch with its endgame off — that build computes the costs inside its sequential
sweep, knot by knot, which is other code (tsat_packed.hpp). Everything but n_forward has to be the same bits."""
import numpy as np
import pytest

import cost_pass_common as cp
import helpers
import line_search_common as lsc
from conftest import assert_same_solution

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


_packed = {}


def packed_reference(pkg, solver, key, b, o):
    """the packed4w solve of a case, computed once and left unchanged"""
    if key not in _packed:
        r = solve(pkg, solver, b, o, PACKED4W)
        for a in (r["X"], r["U"], r["K"], r["stats"]):
            a.setflags(write=False)
        _packed[key] = r
    return _packed[key]


@pytest.mark.parametrize("variant", [WIDE, DENSE])
def test_gpu_ragged_horizons(pkg, ol, solver, variant):
    """N - 1 = 1, 2, 63 | 64 | 65, 255 | 256 | 257, 320 in one batch, budget 2 x 3"""
    b, o, ref = cp.ragged_case(pkg, ol)
    packed = packed_reference(pkg, solver, "ragged", b, o)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)
    lsc.assert_same_bits(packed, got, ("ragged", variant))
    assert np.array_equal(got["stats"]["n_forward"], lsc.expected_n_forward(ref, lsc.FEW, lsc.HOLD_DEFAULT, lsc.MAX_LS))


@pytest.mark.parametrize("variant", [WIDE, DENSE])
@pytest.mark.parametrize("max_ls", [3, 5])
def test_gpu_a_pass_of_one_behind_a_pass_of_two(pkg, ol, solver, variant, max_ls):
    """max_linesearch = 3 and 5 under the policy (3, 0): a sweep keeps three roll-outs, evaluated as a pair and a lone candidate"""
    b, o, ref = cp.odd_case(pkg, ol, max_ls)
    packed = packed_reference(pkg, solver, ("odd", max_ls), b, o)
    solver.set_store_policy(3, 0)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)
    lsc.assert_same_bits(packed, got, ("odd", max_ls, variant))
    want = np.array([lsc.expected_sweeps(lsc.accepted_indices(ref, t), 3, 0, max_ls, max_ls) for t in range(b.T)], dtype=np.int32)
    assert np.array_equal(got["stats"]["n_forward"], want)


@pytest.mark.parametrize("variant", [WIDE, DENSE])
def test_gpu_both_lanes_of_a_pass_win(pkg, ol, solver, variant):
    """searches that end on every index 0 .. 16 and 18: either candidate of a pass is the accepted one"""
    b, o, sub = cp.both_lanes_case(pkg, ol)
    assert b.T <= 18
    packed = packed_reference(pkg, solver, "lanes", b, o)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(sub, got)
    lsc.assert_same_bits(packed, got, ("lanes", variant))


@pytest.mark.parametrize("variant", [WIDE, DENSE])
def test_gpu_candidates_rejected_by_the_validity_bound(pkg, ol, solver, variant):
    """max_state below the first candidates' controls: they fall to the bound, a later candidate is accepted"""
    b, o, ref = cp.bound_case(pkg, ol)
    packed = packed_reference(pkg, solver, "bound", b, o)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)
    lsc.assert_same_bits(packed, got, ("bound", variant))
