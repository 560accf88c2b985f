"""GPU tier of tests/test_solve_mp.py: the solve kernels on the cases of tests/golden/solve_mp.npz against the
50-digit results in the file (bars and the printed table: tests/solve_mp_common.py; E_ref is the error of two oracle builds,
measured here): every case through tsat_batch_* in the wide and the dense build, the ragged batch and the 17-step cases in the packed
builds too, the robust cases with precision = 32. Reads the file and the oracle only; nothing here imports mpmath."""
import pytest

import solve_mp_common as sm

pytestmark = pytest.mark.gpu

N17 = [n for n in sm.CASE_NAMES if sm.n_max(n) == 17]
RAGGED = [n for n in sm.CASE_NAMES if sm.group(n) == "E"]
ROBUST = [n for n in sm.CASE_NAMES if sm.robust(n)]


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    yield s
    s.close()


@pytest.fixture(scope="module")
def oracles(pkg, ol):
    """the two oracle builds on every case (solve_mp_common keeps them: computed once)"""
    return {n: sm.oracles(pkg, ol, n) for n in sm.CASE_NAMES}


def _run(pkg, ol, solver, oracles, variant, names, precision=64):
    solver.set_kernel_variant(variant)
    solver.set_endgame(0)
    try:
        for name in names:
            got = sm.run_gpu(pkg, ol, solver, name, precision)
            if precision == 32:
                sm.check_mixed(name, got, f"kernel variant {variant} precision 32")
            else:
                sm.check_impl(name, got, oracles[name], f"kernel variant {variant}")
    finally:
        solver.set_kernel_variant(0)
        solver.set_endgame(-1)


def test_gpu_oracle_builds_against_50_digits(oracles):
    for name, ora in oracles.items():
        sm.check_oracle(name, ora[0])
        sm.check_exact(name, ora[1], "oracle -ffp-contract=off")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("grp", ["A", "B", "C", "D", "E"])
def test_gpu_one_trajectory_builds_against_50_digits(pkg, ol, solver, oracles, variant, grp):
    """every case in the wide (1) and the dense (2) build"""
    _run(pkg, ol, solver, oracles, variant, [n for n in sm.CASE_NAMES if sm.group(n) == grp])


@pytest.mark.parametrize("variant", [3, 4, 5, 6, 7])
def test_gpu_packed_builds_against_50_digits(pkg, ol, solver, oracles, variant):
    """the ragged batch and the 17-step cases in the packed builds"""
    _run(pkg, ol, solver, oracles, variant, RAGGED + N17)


@pytest.mark.parametrize("variant", [2, 3])
def test_gpu_mixed_precision_on_the_robust_cases(pkg, ol, solver, oracles, variant):
    """precision = 32 (float linearisation): the file's statuses, counts and accepted indices; 1e-3 on X and U / scale"""
    _run(pkg, ol, solver, oracles, variant, ROBUST, precision=32)
