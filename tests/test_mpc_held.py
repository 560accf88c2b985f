"""CPU tier of the loop that re-plans every R control steps (tsat_mpc_run_held): the reference loop of tests/mpc_held_common.py
pinned at R = 1 to the every-step reference, the hold and shift source under the lane emulator against that reference and, at
R = 1, bit-equal to the emulated every-step loop, and what the entry point rejects (the library's own validation function)."""
import numpy as np
import pytest

import mpc_dispersed_common as mc
import mpc_held_common as hc


@pytest.fixture(scope="module")
def emu_mh(pkg):
    return hc.EmuMpcHeld(pkg._abi)


def _ragged_pair(pkg, ol):
    """T = 2, N = 20, horizons (20, 13): all five dispersions, noise on, limits +-0.6, generator ids given"""
    b = hc.mpc_batch(pkg)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    return b, hc.noise_options(ol, min_steps=1), hc.plants(pkg, b), np.array([7, 2 ** 33 + 1], dtype=np.int64)


def test_reference_at_r1_is_the_every_step_reference(pkg, ol):
    """the held reference's own pin: R = 1 is mc.reference_loop for either value of feedback — bar 1e-12, measured 0"""
    b, po, plant, ids = _ragged_pair(pkg, ol)
    for es in (0, 1):
        o = hc.solve_options(ol, error_state=es)
        ref = mc.reference_loop(ol, b, o, 6, po, plant, hc.SAT, ids, step0=2)
        for fb in (0, 1):
            got = hc.reference_loop(ol, b, o, 6, 1, fb, po, plant, hc.SAT, ids, step0=2)
            d = max(float(np.max(np.abs(ref[k] - got[k]))) for k in ("X_hist", "U_hist", "X", "U"))
            print(f"error_state {es} feedback {fb}: max|d| against the every-step reference {d:.2e}")
            assert d < 1e-12
            for k in ("inner_iters", "ls_trials", "status", "outer_iters", "n_backward"):
                assert np.array_equal(ref["stats"][k], got["stats"][k]), k
            assert np.array_equal(ref["n_sure"], got["n_sure"]) and np.array_equal(ref["n_maybe"], got["n_maybe"])
            assert np.array_equal(ref["tracking_stats"], got["tracking_stats"]) and got["n_solves"] == 6


@pytest.mark.parametrize("error_state", [0, 1])
def test_emulated_hold_matches_reference(pkg, ol, emu_mh, error_state):
    """T = 2, ragged, R = 3, 7 steps (blocks 3 + 3 + 1), both feedback values, to the project's MPC bars; the gains are really in
    the loop (the two histories differ) and the held steps are not the every-step loop's"""
    b, po, plant, ids = _ragged_pair(pkg, ol)
    o = hc.solve_options(ol, error_state=error_state)
    got = {}
    for fb in (1, 0):
        ref = hc.reference_loop(ol, b, o, 7, 3, fb, po, plant, hc.SAT, ids)
        assert ref["n_solves"] == 3 and np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
        got[fb] = emu_mh.run(b, o, po, 7, 3, fb, plant, hc.SAT, ids)
        hc.same(ref, got[fb], b, po, plan=True)
    dU = float(np.max(np.abs(got[1]["U_hist"] - got[0]["U_hist"])))
    every = emu_mh.run(b, o, po, 7, 1, 1, plant, hc.SAT, ids)
    print(f"gains on against off: max|dU_hist| {dU:.2e}; R = 3 against R = 1: {np.max(np.abs(every['U_hist'] - got[1]['U_hist'])):.2e}")
    assert dU > 1e-6
    assert np.array_equal(got[1]["U_hist"][:, 0], got[0]["U_hist"][:, 0])          # j = 0 evaluates no gain product
    assert np.max(np.abs(every["U_hist"] - got[1]["U_hist"])) > 1e-6


def test_emulated_hold_with_wide_limits_flies_the_gains(pkg, ol, emu_mh):
    """no clip in the way (limits +-25): the commands of the held steps are U_j + K_j dx to the bar, and differ from U_j"""
    b, po, plant, ids = _ragged_pair(pkg, ol)
    o = hc.solve_options(ol)
    ref = hc.reference_loop(ol, b, o, 5, 5, 1, po, plant, hc.WIDE, ids)
    got = emu_mh.run(b, o, po, 5, 5, 1, plant, hc.WIDE, ids)
    hc.same(ref, got, b, po, plan=True)
    assert np.array_equal(got["n_clipped"], [0, 0])
    hold = emu_mh.run(b, o, po, 5, 5, 0, plant, hc.WIDE, ids)
    assert np.max(np.abs(hold["U_hist"][:, 1:] - got["U_hist"][:, 1:])) > 1e-6


@pytest.mark.parametrize("error_state", [0, 1])
def test_emulated_r1_is_bit_equal_to_the_every_step_loop(pkg, ol, emu_mh, error_state):
    b, po, plant, ids = _ragged_pair(pkg, ol)
    o = hc.solve_options(ol, error_state=error_state)
    old = mc.EmuMpcDispersed(pkg._abi).run(b, o, po, 5, plant, hc.SAT, ids, step0=3)
    for fb in (0, 1):
        new = emu_mh.run(b, o, po, 5, 1, fb, plant, hc.SAT, ids, step0=3)
        for k in ("X_hist", "U_hist", "stats", "X", "U", "tracking_stats", "n_clipped"):
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)


def test_rejected_arguments(pkg, emu_mh):
    """check_mpc_held, which the entry point calls after tsat_mpc_run_dispersed's checks"""
    assert emu_mh.check(1, 0, 2) == (0, "") and emu_mh.check(19, 1, 20) == (0, "")
    for args, word in (((0, 1, 20), "replan_every must be >= 1"), ((-3, 1, 20), "replan_every must be >= 1"),
                       ((20, 1, 20), "min n_knots - 1 = 19"), ((6, 1, 6), "min n_knots - 1 = 5"), ((3, 2, 20), "feedback"),
                       ((3, -1, 20), "feedback")):
        rc, text = emu_mh.check(*args)
        assert rc == -1 and word in text, (args, text)
    # without a handle the entry point itself is a code, not a crash
    lib = pkg._abi.load()
    assert lib.tsat_mpc_run_held(None, None, None, 1, 0, 1, 1, None, None, None, None, None, None, None, None, None, None) == -1
