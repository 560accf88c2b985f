"""The AL-iLQR solve (backward sweep, forward sweep and line search, the AL outer loop) against a 50-digit reference, CPU tier: the
oracle on every case of tests/golden/solve_mp.npz, the emulated wide build on every case of at most 65 steps,
the other emulated fp64 builds on the ragged batch and the 17-step cases, the emulated mixed-precision builds on the robust cases
(cases, bars and the table the tests print: tests/solve_mp_common.py), and the file itself regenerated on its short cases."""
import numpy as np
import pytest

import solve_mp_common as sm

SHORT = 17        # the cases regenerated in-process: at most this many steps
WIDE_MAX = 65     # the emulated wide build runs the cases of at most this many steps

N17 = [n for n in sm.CASE_NAMES if sm.n_max(n) == 17]
RAGGED = [n for n in sm.CASE_NAMES if sm.group(n) == "E"]
ROBUST = [n for n in sm.CASE_NAMES if sm.robust(n)]


@pytest.mark.parametrize("name", [n for n in sm.CASE_NAMES if sm.n_max(n) <= SHORT])
def test_file_is_the_50_digit_reference(pkg, name):
    """tests/refmath_mp.py::solve_reference on the file's inputs, rounded to float64: the file's outputs, bit for bit"""
    s = sm.script()
    case = s.build_cases(pkg)[name]
    c = sm.fixture()[name]
    for k, v in s.batch_arrays(case["b"]).items():
        assert v.tobytes() == c[f"in_{k}"].tobytes(), (name, "input", k)
    assert case["opts"].tobytes() == c["opts"].tobytes()
    b = s.batch_arrays(case["b"])
    per = [s.compute_traj((b, t, int(n), case["opts"])) for t, n in enumerate(b["n_knots"])]
    s.check_case(name, case, per)
    for k, v in s.assemble(case, per).items():
        assert v.dtype == c[k].dtype and v.tobytes() == c[k].tobytes(), (name, k)


def test_cases_reach_what_they_are_there_for():
    """the horizons, modes, integrators and inertia kinds of the groups; restarts, failed searches, the exits and the two failure
    statuses; margins as the script asserts them"""
    C = sm.fixture()
    s = sm.script()
    have = {(sm.group(n), sm.n_max(n), sm.options(n)["error_state"], sm.options(n)["integrator"]) for n in sm.CASE_NAMES}
    for n in (1, 2, 63, 64, 65, 129, 15, 16, 17, 32, 33):
        assert ("A", n, 1, 3) in have, n
    for n in (54, 55, 56, 111):
        assert ("A", n, 0, 3) in have, n
    assert ("A", 65, 1, 4) in have and ("A", 56, 0, 4) in have
    assert len([n for n in N17 if sm.group(n) == "A"]) == 12
    for n in sm.CASE_NAMES:
        c = C[n]
        assert np.all(c["margin"] >= (s.ROBUST if sm.robust(n) else s.MARGIN)), n
        if sm.group(n) == "A":
            assert np.all(c["inner_iters"] == 1) and np.all(c["n_backward"] == 1), n
    assert {sm.options(n)["terminal_mask"] for n in sm.CASE_NAMES if sm.group(n) == "B"} == {0, 0b1111000, 0b1111111}
    for n in ("C_negR_n65", "C_negR_n129"):
        assert C[n]["bp_restarts"][0] > 0 and C[n]["status"][0] == 1
    assert C["C_ls1_n17"]["fp_fails"][0] == 2 and C["C_reg_fail_n17"]["status"][0] == sm.ST_REG_FAIL and C["C_diverged_n17"]["status"][0] == sm.ST_DIVERGED
    for n in RAGGED:
        assert C[n]["in_n_knots"].tolist() == s.RAGGED and len(C[n]["in_n_knots"]) == 13
    assert len(ROBUST) >= 4


@pytest.mark.parametrize("name", sm.CASE_NAMES)
def test_oracle_and_emulated_wide_build_against_50_digits(pkg, ol, emu, name):
    ora = sm.oracles(pkg, ol, name)
    sm.check_oracle(name, ora[0])
    sm.check_exact(name, ora[1], "oracle -ffp-contract=off")
    if sm.n_max(name) <= WIDE_MAX:
        sm.check_impl(name, sm.run_emu(emu, pkg, ol, name), ora, "emu")


@pytest.mark.parametrize("build", ["emu_dense", "emu_packed", "emu_packed8", "emu_packed4w", "emu_packed8w", "emu_packed16w"])
def test_emulated_builds_against_50_digits(pkg, ol, request, build):
    """the ragged batch and the 17-step cases through the other fp64 builds"""
    e = request.getfixturevalue(build)
    for name in RAGGED + N17:
        sm.check_impl(name, sm.run_emu(e, pkg, ol, name), sm.oracles(pkg, ol, name), build)


@pytest.mark.parametrize("build", ["emu_mixed", "emu_packed_mixed"])
def test_emulated_mixed_builds_on_the_robust_cases(pkg, ol, request, build):
    e = request.getfixturevalue(build)
    for name in ROBUST:
        sm.check_mixed(name, sm.run_emu(e, pkg, ol, name, precision=32), build)
