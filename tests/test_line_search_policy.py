"""CPU tier: the keep rule of the one-trajectory builds' line search (tsat_set_store_policy, solve_trajectory in
tsat_device.hpp) on the lane emulator. How many roll-outs a forward sweep keeps decides whether a deep search needs another
sweep, never which candidate is accepted: X, U, K and every statistic except n_forward are the same bits under every policy,
and n_forward is exactly what the rule, replayed on the oracle's line-search trace, says."""
import numpy as np
import pytest

import line_search_common as lsc
from conftest import assert_same_solution


def test_the_input_reaches_every_branch_of_the_rule(pkg, ol):
    """what the other tests rest on: accepted indices 0 .. 16 and 18, a failed search, every trajectory searching past index 3,
    and a good part of them past the 12 roll-outs a sweep kept before every candidate had a slot"""
    _, _, ref = lsc.case(pkg, ol)
    jw = [lsc.accepted_indices(ref, t) for t in range(lsc.T)]
    allj = np.concatenate(jw)
    assert set(range(17)) | {18} <= set(allj.tolist())       # (17 and 19 are the two indices no search of this input ends on)
    assert int(np.sum(allj < 0)) == 1 and int(ref["stats"]["fp_fails"].sum()) == 1
    assert all(np.any(j >= 4) for j in jw)
    assert len(lsc.deep_trajectories(ref)) == 19
    # the policies differ on it, in the order the rule promises: no repeated sweep when every roll-out is kept, fewer with a hold
    nf = {p: lsc.expected_n_forward(ref, *p, slots=lsc.MAX_LS) for p in ((4, 0), (lsc.FEW, lsc.HOLD_DEFAULT), (4, -1), (1, 0), lsc.KEEP_ALL)}
    assert np.array_equal(nf[lsc.KEEP_ALL], 1 + ref["stats"]["inner_iters"])
    assert np.all(nf[(lsc.FEW, lsc.HOLD_DEFAULT)] <= nf[(4, 0)]) and nf[(lsc.FEW, lsc.HOLD_DEFAULT)].sum() < nf[(4, 0)].sum()
    assert np.all(nf[(4, -1)] <= nf[(lsc.FEW, lsc.HOLD_DEFAULT)])
    assert nf[(1, 0)].sum() < nf[(4, 0)].sum()      # few = 1: every search counts as deep, only a trajectory's first sweeps keep one


def test_host_sizes_the_slabs_by_batch_and_rejects_a_bad_policy(pkg):
    """tsat_batch_reserve's sizing and tsat_set_store_policy's check are host functions of tsat_host_pack.hpp: a slab for every
    candidate below 2048 trajectories (one-trajectory builds), 12 at most from there on (the packed builds)"""
    lib = lsc.emulator(pkg, dense=False).lib
    assert [lib.emu_reserved_slots(t, 20) for t in (1, 64, 1024, 2047, 2048, 65536)] == [20, 20, 20, 20, 12, 12]
    assert [lib.emu_reserved_slots(t, 32) for t in (64, 2048)] == [32, 12]
    assert [lib.emu_reserved_slots(t, 5) for t in (64, 2048)] == [5, 5]
    try:
        assert lib.emu_set_store_policy(0, 0, 0) == -1 and lib.emu_set_store_policy(-3, 8, 0) == -1
        assert lib.emu_set_store_policy(1, -1, 0) == 0 and lib.emu_set_store_policy(32, 0, 3) == 0
    finally:
        lib.emu_reset_store_policy()


@pytest.fixture(scope="module")
def deep_case(pkg, ol):
    """at most four of the deep trajectories: the one whose search fails, then the shortest solves with a search past index 11"""
    b, o, ref = lsc.case(pkg, ol)
    deep = lsc.deep_trajectories(ref)
    failed = [t for t in deep if np.any(lsc.accepted_indices(ref, t) < 0)]
    rest = sorted((t for t in deep if t not in failed), key=lambda t: int(ref["stats"]["inner_iters"][t]))
    idx = sorted(failed[:1] + rest[:2])
    sub = dict(X=ref["X"][idx], U=ref["U"][idx], K=ref["K"][idx], stats=ref["stats"][idx])
    return lsc.pick(pkg, b, idx), o, ref, idx, sub


@pytest.mark.parametrize("build", ["emu", "emu_dense"])
def test_emulated_builds_same_bits_under_every_policy(pkg, deep_case, build):
    e = lsc.emulator(pkg, dense=build == "emu_dense")
    b, o, ref, idx, sub = deep_case
    a = o.copy()
    assert a.max_linesearch == 20
    got = {}
    try:
        # (few, hold, reserved slots): today's rule, keep-all — both with a slab per candidate, more than the former 12 in use —
        # and the default rule on FIVE reserved slabs: a search past index 4 falls back to repeated sweeps of five
        for pol in ((4, 0, 0), lsc.KEEP_ALL + (0,), (lsc.FEW, lsc.HOLD_DEFAULT, 5)):
            assert e.lib.emu_set_store_policy(*pol) == 0
            got[pol] = e.solve(b, a)
    finally:
        e.lib.emu_reset_store_policy()
    base = got[(4, 0, 0)]
    assert_same_solution(sub, base)
    for pol, g in got.items():
        lsc.assert_same_bits(base, g, (build, pol))
        slots = pol[2] or lsc.MAX_LS
        assert np.array_equal(g["stats"]["n_forward"], lsc.expected_n_forward(ref, pol[0], pol[1], slots, idx)), (build, pol)
    keep = got[lsc.KEEP_ALL + (0,)]["stats"]
    assert np.array_equal(keep["n_forward"], 1 + keep["inner_iters"])
    few5 = got[(lsc.FEW, lsc.HOLD_DEFAULT, 5)]["stats"]
    assert np.all(few5["n_forward"] > 1 + few5["inner_iters"])       # every one of them has a search past five slots
