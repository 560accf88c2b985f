"""GPU tier (`pytest -m gpu`): the Riccati loop of the one-trajectory builds (riccati_rows) runs on DPP row 0 alone — the three
other rows would repeat the same trajectory and nobody reads them — looks at the Sylvester test once per chunk instead of once
per knot, and steps its record and K,d pointers. None of it may change a bit of what a solve returns: the wide and the dense build
are compared with the oracle at the fp64 bar and, bit for bit, with the packed4w build forced onto the same batch, whose forward
sweep and Riccati loop are other code (tsat_packed.hpp; its endgame is off, so that no trajectory is handed to the one-trajectory
mapping). The keep-rule cases vary how many lanes of the forward sweep store their roll-out (n_cand) across the 16-lane row
boundary; the restart and ragged cases drive failing sweeps, one-knot chunks and odd knot counts through the new loop."""
import numpy as np
import pytest

import helpers
import line_search_common as lsc
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
@pytest.mark.parametrize("few", [4, 16, 17, 20])
def test_gpu_keep_rule_boundaries(pkg, ol, solver, variant, few):
    """n_cand = few while the searches end early and 20 after a deep one: 4 (one row), 16 (the row boundary), 17 (the first lane
    of the second row), 20 (every candidate, always) — accepted indices 0 .. 16 and 18 occur in this input"""
    b, o, ref = lsc.case(pkg, ol)
    acc = np.concatenate([lsc.accepted_indices(ref, t) for t in range(lsc.T)])
    assert set(range(17)) | {18} <= set(acc.tolist())
    packed = packed_reference(pkg, solver, "keep", b, o)
    solver.set_store_policy(few, lsc.HOLD_DEFAULT)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)                  # equal counts, |dX|, |dU| < 1e-9 of the control scale
    lsc.assert_same_bits(packed, got, (variant, few))


def restart_cases(pkg, ol):
    """(name, batch, options, oracle result): the committed golden cases with regularisation restarts, and the REG_FAIL case"""
    out = []
    for name in helpers.golden_cases():
        b, o, ref = helpers.load_case(name, pkg, ol)
        if ref["stats"]["bp_restarts"].sum() > 0:
            out.append((name, b, o, ref))
    assert out, "no golden case restarts its backward sweep"
    b = pkg.slew_setup.workload_monte_carlo(T=2, N=40, seed=5)
    b.Rd[:] = -1e-4                                  # Quu indefinite and rho may not grow: REG_FAIL
    o = oracle_options(ol, max_outer=2, max_inner=3, reg_max=1e-6)
    ref = ol.solve_batch(b, o)
    assert np.all(ref["stats"]["status"] == pkg._abi.TSAT_REG_FAIL) and ref["stats"]["bp_restarts"].sum() > 0
    out.append(("reg_fail", b, o, ref))
    return out


@pytest.mark.parametrize("variant", [WIDE, DENSE])
def test_gpu_restarts_and_reg_fail(pkg, ol, solver, variant):
    """a failed backward sweep runs on to the end of its chunk, storing nothing behind the failing knot: the same restarts, the
    same results"""
    for name, b, o, ref in restart_cases(pkg, ol):
        packed = packed_reference(pkg, solver, name, b, o)
        got = solve(pkg, solver, b, o, variant)
        assert_same_solution(ref, got)
        assert np.array_equal(ref["stats"]["bp_restarts"], got["stats"]["bp_restarts"]), name
        same_bits(packed, got, (name, variant), pkg._abi)
        ok = ref["stats"]["status"] != pkg._abi.TSAT_REG_FAIL
        if ok.any():
            scale = max(float(np.max(np.abs(ref["K"][ok]))), 1.0)
            assert np.max(np.abs(ref["K"][ok] - got["K"][ok])) < 1e-9 * scale, name


RAGGED = (2, 3, 34, 66, 130)


@pytest.mark.parametrize("variant", [WIDE, DENSE])
@pytest.mark.parametrize("es", [0, 1])
def test_gpu_ragged_lengths(pkg, ol, solver, variant, es):
    """per-trajectory horizons with N - 1 = 1, 2 (one-knot chunks, the odd knot of a two-knot turn), 33 (a second forward chunk
    of one knot), 65 (a second 64-knot Riccati chunk of one knot), 129 (odd, several chunks of both loops) in one batch; each
    length twice, the second time with an indefinite R, so that backward sweeps fail and restart at these lengths too"""
    b = pkg.slew_setup.workload_monte_carlo(T=2 * len(RAGGED), N=max(RAGGED), seed=700 + es, degenerate_rd=0.03)
    b.n_knots = np.array(RAGGED * 2, dtype=np.int32)
    b.Rd[len(RAGGED):, 2] = -1e-4
    o = oracle_options(ol, max_outer=2, max_inner=3, dj_counter_limit=1, error_state=es)
    ref = ol.solve_batch(b, o, nthreads=4)
    assert ref["stats"]["bp_restarts"][len(RAGGED):].sum() > 0
    packed = packed_reference(pkg, solver, ("ragged", es), b, o)
    got = solve(pkg, solver, b, o, variant)
    assert_same_solution(ref, got)
    assert np.array_equal(ref["stats"]["bp_restarts"], got["stats"]["bp_restarts"])
    same_bits(packed, got, (es, variant), pkg._abi)
