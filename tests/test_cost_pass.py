"""CPU tier: the line search's cost pass (candidate_costs in tsat_device.hpp) on the lane emulator, wide and dense layout,
against the oracle — equal counts and the fp64 bar. The pass reads every stored candidate with lanes = knots, 64 knots a step,
adds a candidate's costs in knot order 256 knots (a block) at a time, and takes one or two candidates a pass (an instance of
its own each): the cases sit on the edges of a step and of a block, put a pass of one candidate behind a pass of two, let
either lane of a pass win, and reject candidates by the validity bound instead of by their cost."""
import numpy as np
import pytest

import cost_pass_common as cp
import line_search_common as lsc
from conftest import assert_same_solution

BUILDS = ["emu", "emu_dense"]


def test_the_inputs_reach_what_they_are_for(pkg, ol):
    _, _, ref = cp.ragged_case(pkg, ol)
    assert np.all(ref["stats"]["inner_iters"] >= 3)
    for max_ls, lone in ((3, 2), (5, 2)):
        _, _, ref = cp.odd_case(pkg, ol, max_ls)
        acc = np.concatenate([lsc.accepted_indices(ref, t) for t in range(4)])
        # under the policy (3, 0) a sweep keeps three roll-outs: index 2 is the pass of one candidate behind the pass of two,
        # a failed search (-1) runs every pass, and with five candidates a second sweep holds the pair (3, 4)
        assert lone in acc and -1 in acc and 0 in acc and 1 in acc
        assert max_ls == 3 or (3 in acc and 4 in acc)
    # the bound: the same slews without it accept an earlier candidate at the first search that differs, so the candidates
    # before the accepted one were rejected by the bound and not by their cost — and one is still accepted
    b, o, ref = cp.bound_case(pkg, ol)
    free = o.copy()
    free.max_state = 1e8
    ref_free = ol.solve_batch(b, free, nthreads=4, trace_rows=16)
    later = 0
    for t in range(b.T):
        jb, jf = lsc.accepted_indices(ref, t), lsc.accepted_indices(ref_free, t)
        d = [i for i in range(min(len(jb), len(jf))) if jb[i] != jf[i]]
        if d and jb[d[0]] > jf[d[0]] >= 0:
            later += 1
    assert later >= 1
    assert float(np.max(np.abs(ref["U"]))) <= cp.BOUND


@pytest.mark.parametrize("build", BUILDS)
def test_ragged_horizons(pkg, ol, build):
    b, o, ref = cp.ragged_case(pkg, ol)
    got = lsc.emulator(pkg, dense=build == "emu_dense").solve(b, o)
    assert_same_solution(ref, got)
    # (the oracle counts sequential roll-outs; a build's sweeps are what the keep rule says for the accepted indices)
    assert np.array_equal(got["stats"]["n_forward"], lsc.expected_n_forward(ref, lsc.FEW, lsc.HOLD_DEFAULT, lsc.MAX_LS))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("max_ls", [3, 5])
def test_a_pass_of_one_behind_a_pass_of_two(pkg, ol, build, max_ls):
    b, o, ref = cp.odd_case(pkg, ol, max_ls)
    e = lsc.emulator(pkg, dense=build == "emu_dense")
    try:
        assert e.lib.emu_set_store_policy(3, 0, 0) == 0
        got = e.solve(b, o)
    finally:
        e.lib.emu_reset_store_policy()
    assert_same_solution(ref, got)
    want = np.array([lsc.expected_sweeps(lsc.accepted_indices(ref, t), 3, 0, max_ls, max_ls) for t in range(b.T)], dtype=np.int32)
    assert np.array_equal(got["stats"]["n_forward"], want)


@pytest.mark.parametrize("build", BUILDS)
def test_both_lanes_of_a_pass_win(pkg, ol, build):
    b, o, sub = cp.both_lanes_case(pkg, ol)
    got = lsc.emulator(pkg, dense=build == "emu_dense").solve(b, o)
    assert_same_solution(sub, got)


@pytest.mark.parametrize("build", BUILDS)
def test_candidates_rejected_by_the_validity_bound(pkg, ol, build):
    b, o, ref = cp.bound_case(pkg, ol)
    got = lsc.emulator(pkg, dense=build == "emu_dense").solve(b, o)
    assert_same_solution(ref, got)
