"""GPU tier (`pytest -m gpu`): the keep rule of the line search in the one-trajectory builds (tsat_set_store_policy) and the
candidate slabs tsat_batch_reserve sizes for it. The rule decides how many forward sweeps a solve executes, never what it
computes: X, U, K and every statistic but n_forward are the same bits under every policy and in every build, equal to the
oracle at the fp64 bar, and n_forward is what the rule replayed on the oracle's line-search trace says."""
import numpy as np
import pytest

import helpers
import line_search_common as lsc
from conftest import assert_same_solution

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver(pkg):
    """a handle of its own for every test: the keep rule it starts with is the library's default"""
    import torch

    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    s = pkg.trajopt.AugmentedLagrangianSolver(None, None, device=0)
    yield s
    s.close()


def solve(pkg, solver, b, o):
    a = helpers.abi_options_like(o, pkg, b.N, b.n_tab)
    solver.upload(b, a.max_linesearch)
    solver.run(a)
    return solver.download()


@pytest.mark.parametrize("variant", [1, 2])
def test_gpu_policies_are_the_same_solve(pkg, ol, solver, variant):
    b, o, ref = lsc.case(pkg, ol)
    solver.set_kernel_variant(variant)
    got = {"default": solve(pkg, solver, b, o)}           # the handle's own rule: nothing has been set yet
    for pol in ((4, 0), (1, 0), lsc.KEEP_ALL):
        solver.set_store_policy(*pol)
        got[pol] = solve(pkg, solver, b, o)
    base = got[(4, 0)]
    assert_same_solution(ref, base)                        # equal counts, |dX|, |dU| < 1e-9 of the control scale
    for pol, g in got.items():
        lsc.assert_same_bits(base, g, (variant, pol))
    nf = {pol: g["stats"]["n_forward"] for pol, g in got.items()}
    print("n_forward totals:", {str(p): int(v.sum()) for p, v in nf.items()}, "1 + inner_iters:", int((1 + base["stats"]["inner_iters"]).sum()))
    assert np.array_equal(nf[lsc.KEEP_ALL], 1 + base["stats"]["inner_iters"])
    assert np.all(nf["default"] <= nf[(4, 0)]) and nf["default"].sum() < nf[(4, 0)].sum()
    # sweep for sweep what the rule says, with a slab for each of the 20 candidates at this batch size
    assert np.array_equal(nf["default"], lsc.expected_n_forward(ref, lsc.FEW, lsc.HOLD_DEFAULT, lsc.MAX_LS))
    for pol in ((4, 0), (1, 0)):
        assert np.array_equal(nf[pol], lsc.expected_n_forward(ref, *pol, slots=lsc.MAX_LS)), pol


@pytest.mark.parametrize("variant,at", [(3, 40), (7, 64)])
def test_gpu_hand_over_carries_the_rule(pkg, ol, solver, variant, at):
    """a packed launch with the endgame on: wavefronts down to one live trajectory hand it to the one-trajectory mapping, and
    at `at` live trajectories the rest is parked for the resume kernel — the Resume record carries the rule's counter. Same bits
    as the plain wide solve; n_forward is the only field that may differ."""
    b, o, ref = lsc.case(pkg, ol)
    solver.set_kernel_variant(1)
    wide = solve(pkg, solver, b, o)
    solver.set_kernel_variant(variant)
    solver.set_endgame(at)
    packed = solve(pkg, solver, b, o)
    lsc.assert_same_bits(wide, packed, (variant, at))
    assert_same_solution(ref, packed)


def test_gpu_reserve_sizes_the_slabs_by_batch(pkg, solver):
    """tsat_batch_reserve: a slab for each of the max_linesearch candidates where a one-trajectory build runs (fewer than 2048
    trajectories), the former 12 at most above; tsat_set_store_policy rejects few < 1"""
    lib, h, n, n_tab = solver._lib, solver._h, 16, 20
    slab = n * 10 * 8                      # [N][10] doubles

    def slabs(T, max_ls):                  # candidate slabs per trajectory: what max_ls adds to a reservation of one
        by = []
        for m in (1, max_ls):
            assert lib.tsat_batch_reserve(h, T, n, n_tab, 1, m) == 0
            by.append(int(lib.tsat_batch_bytes(h)))
        assert (by[1] - by[0]) % (T * slab) == 0
        return 1 + (by[1] - by[0]) // (T * slab)

    assert [slabs(T, 20) for T in (64, 2047, 2048)] == [20, 20, 12]
    assert slabs(64, 32) == 32 and slabs(2048, 7) == 7
    for few in (0, -1):
        with pytest.raises(RuntimeError, match="few must be >= 1"):
            solver.set_store_policy(few, 8)
    solver.set_store_policy(1, -1)
    assert lib.tsat_set_store_policy(None, 4, 8) != 0
