"""CPU tier of the held re-planning loop fed measurements (tsat_mpc_run_held_sensed): the reference loop of
tests/mpc_sensed_common.py pinned with the ideal sensor to the held references, the source of
tortoisesat.jl_amd/csrc/tsat_mpc_sensed.hpp under the lane emulator against that reference, Y_hist checked two ways, the ideal
sensor bit-equal to the emulated parents, the state the call leaves behind, and what the entry point rejects (the library's own
validation function).

The case: T = 2, N = 20, horizons (20, 13), all five plant dispersions, plant noise on, generator ids (7, 2^33 + 1), R = 3 over 7
steps (blocks 3 + 3 + 1); sensor sigmas ``sensed_common.SIGMAS`` (3e-4 rad/s, 0.3 deg), biases at twice ``sensed_common.BIAS``
(3e-3 rad/s, 1.5 deg; see mpc_sensed_common). Limits +-5: under the held tests' +-0.6 every component of every command clips, and
the attitude bias then moves the reference's final state by exactly 0.0 (a condition failed: the level of the LIMIT was changed,
not the condition); under +-5 every step still clips a component (n_sure = 7 of 7, 5 of 7 with the gains off) and the others pass.
Statistic: min_steps = 1, w_tol = 1e-2, angle_tol = 3.7, chosen on the reference alone: its rate norms stay an order below w_tol (they reach 1e-3) and its
angles at 4.195 (trajectory 0, fails) and 3.290 (trajectory 1, arrives at sample 2), so both outcomes are present with margin 0.11.
Measured on the reference over the five parametrised cases: every block solve ends TSAT_MAX_OUTER; sensor noise moves the final
state by 3.4e-6 (gains off) .. 2.3e-3, the gyro bias by 1.2e-4 .. 5.8e-4, the attitude bias by 1.4e-5 .. 1.0e-4, latency 1 against
0 by 3.5e-6 (gains off) .. 1.7e-3 (bar gg_common.MOVED = 1e-7). Measured on the emulator against it: max |dX_hist| 5.4e-16,
|dU_hist| 1.1e-11, |dY_hist| 1.1e-16; Y_hist against ``measure`` of the returned X_hist 1.1e-16; sensor on against off in
U_hist[j > 0] under limits nothing reaches: 4.0e2 (commands up to 4.1e2)."""
import math

import numpy as np
import pytest

import gg_common as gc
import mpc_held_common as hc
import mpc_sensed_common as mc
import sensed_common as sc

N_STEPS, R = 7, 3
W_TOL, ANGLE_TOL = 1e-2, 3.7
Y_BAR = 1e-9                 # the state bar of tests/test_sensed.py (dispersed_common.compare on X_sim)
LIMITS = (np.full(3, -5.0), np.full(3, 5.0))      # inside the workload's commands (up to 20): some components clip, some do not
WIDE = (np.full(3, -1e4), np.full(3, 1e4))         # limits no command of the case reaches (the gains on a 1e-2 measurement error
                                                   # command a few hundred; mpc_held_common.WIDE, +-25, would clip them)
_CASE = object()


@pytest.fixture(scope="module")
def emu_ms(pkg):
    return mc.EmuMpcSensed(pkg._abi)


@pytest.fixture(scope="module")
def pair(pkg, ol):
    """the case, and its references by (error_state, latency, feedback, sens on, limits), each computed once and left unchanged"""
    b = hc.mpc_batch(pkg)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = hc.noise_options(ol, min_steps=1, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant, ids, bias = hc.plants(pkg, b), np.array([7, 2 ** 33 + 1], dtype=np.int64), mc.biases(pkg, 2)
    refs = {}

    def ref(es, latency, fb=1, sens=mc.SIGMAS, bias=bias, sat=LIMITS):
        key = (es, latency, fb, tuple(sorted(sens.items())), None if bias is None else bias.tobytes(), sat[0][0])
        if key not in refs:
            refs[key] = mc.reference_loop(ol, b, hc.solve_options(ol, error_state=es), N_STEPS, R, fb, po, sens, bias, latency, plant, sat, ids)
        return refs[key]

    return dict(b=b, po=po, plant=plant, ids=ids, bias=bias, ref=ref)


def _emu(emu_ms, ol, p, es, latency, fb=1, sens=mc.SIGMAS, bias=_CASE, sat=LIMITS, **kw):
    return emu_ms.run(p["b"], hc.solve_options(ol, error_state=es), p["po"], N_STEPS, R, fb, sens, p["bias"] if bias is _CASE else bias, latency,
                      p["plant"], sat, p["ids"], **kw)


def test_reference_with_the_ideal_sensor_is_the_held_reference(pkg, ol, pair):
    """the reference's own pin: no biases, zero sigmas, latency 0 — max |d| = 0 against mpc_held_common.reference_loop and, with an
    orbit table, against gg_common.held_loop; Y_hist is then X_hist"""
    b, po, plant, ids = pair["b"], pair["po"], pair["plant"], pair["ids"]
    for es in (0, 1):
        o = hc.solve_options(ol, error_state=es)
        for fb in (0, 1):
            old = hc.reference_loop(ol, b, o, N_STEPS, R, fb, po, plant, hc.SAT, ids, step0=2)
            new = mc.reference_loop(ol, b, o, N_STEPS, R, fb, po, None, None, 0, plant, hc.SAT, ids, step0=2)
            d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_hist", "U_hist", "X", "U"))
            print(f"error_state {es} feedback {fb}: max|d| against the held reference {d:.2e}")
            assert d == 0.0
            assert np.array_equal(new["Y_hist"], new["X_hist"][:, :-1])
            assert np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["tracking_stats"], new["tracking_stats"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["tally"], new["tally"])
    bg = gc.use_3u(pkg, hc.mpc_batch(pkg))
    Rtab = gc.orbit(pkg, bg.n_tab, 0.2)[None]
    o = hc.solve_options(ol)
    old = gc.held_loop(ol, bg, o, 4, R, 1, po, Rtab, gc.GM, plant, hc.SAT, ids)
    new = mc.reference_loop(ol, bg, o, 4, R, 1, po, None, np.zeros((2, 9)), 0, plant, hc.SAT, ids, Rtab=Rtab, gm=gc.GM)
    d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_hist", "U_hist", "X", "U"))
    print(f"with the orbit table: max|d| against the gravity-gradient held reference {d:.2e}")
    assert d == 0.0


@pytest.mark.parametrize("error_state,latency,feedback", [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 1, 0)])
def test_emulated_loop_matches_reference(pkg, ol, emu_ms, pair, error_state, latency, feedback):
    """R = 3, 7 steps (blocks 3 + 3 + 1) to the project's MPC bars, the last plan with them; Y_hist to the state bar. The conditions
    of the case are asserted on references alone first."""
    b, po, bias = pair["b"], pair["po"], pair["bias"]
    ref = mc.conditions(lambda **over: pair["ref"](error_state, **{"latency": latency, "fb": feedback, **over}), bias,
                        f"error_state {error_state} latency {latency} feedback {feedback}", b, po)
    assert ref["n_solves"] == 3
    got = _emu(emu_ms, ol, pair, error_state, latency, feedback)
    hc.same(ref, got, b, po, plan=True)
    dY = float(np.max(np.abs(ref["Y_hist"] - got["Y_hist"])))
    print(f"max|dY_hist| {dY:.2e}")
    assert dY < Y_BAR


@pytest.mark.parametrize("latency", [0, 1])
def test_y_hist_is_the_measurement_of_the_returned_true_states(pkg, ol, emu_ms, pair, latency):
    """Y_hist = measure(X_hist) with the latency shift, to the state bar; and X_hist holds TRUE states: it is not Y_hist"""
    got = _emu(emu_ms, ol, pair, 0, latency)
    want = mc.measured(ol, pair["b"], pair["po"], got["X_hist"], mc.SIGMAS, pair["bias"], latency, pair["ids"])
    d = float(np.max(np.abs(want - got["Y_hist"])))
    off = float(np.max(np.abs(got["Y_hist"] - got["X_hist"][:, :-1])))
    print(f"latency {latency}: max|Y_hist - measure(X_hist)| {d:.2e}; max|Y_hist - X_hist| {off:.2e}")
    assert d < Y_BAR
    assert off > 1e-4
    if latency:
        assert np.array_equal(got["Y_hist"][:, 1], got["Y_hist"][:, 0])   # the first step of a call sees its own measurement, m_0


def test_the_gains_read_the_measurement(pkg, ol, emu_ms, pair):
    """feedback 1, limits +-1e4 (nothing clips), so U_hist of the held steps is U_j + K_j dx itself and is held to the reference,
    whose dx is taken from y_s, at the 1e-8 bar; U_hist[j > 0] differs between sensor on and off by more than 1e-6, and the gains
    are really in the loop (against the open-loop hold under the same sensor)"""
    b, po = pair["b"], pair["po"]
    ref = pair["ref"](0, 0, sat=WIDE)
    assert np.array_equal(ref["n_maybe"], [0, 0]), "a step of the wide-limits case is near a limit"
    on = _emu(emu_ms, ol, pair, 0, 0, sat=WIDE)
    print(f"max|U_hist| {np.max(np.abs(ref['U_hist'])):.1f}")
    hc.same(ref, on, b, po, plan=True)
    assert np.array_equal(on["n_clipped"], [0, 0])
    off = _emu(emu_ms, ol, pair, 0, 0, sens=mc.IDEAL, bias=None, sat=WIDE)
    dU = float(np.max(np.abs(on["U_hist"][:, 1:] - off["U_hist"][:, 1:])))
    print(f"sensor on against off: max|dU_hist[j > 0]| {dU:.2e}")
    assert dU > 1e-6
    hold = _emu(emu_ms, ol, pair, 0, 0, fb=0, sat=WIDE)
    dK = float(np.max(np.abs(on["U_hist"][:, 1:3] - hold["U_hist"][:, 1:3])))
    print(f"gains on against off under the same sensor, block 0: max|dU_hist| {dK:.2e}")
    assert np.array_equal(on["U_hist"][:, 0], hold["U_hist"][:, 0])              # j = 0 evaluates no gain product
    assert dK > 1e-6


@pytest.mark.parametrize("error_state", [0, 1])
def test_emulated_ideal_sensor_is_bit_equal_to_the_emulated_parents(pkg, ol, emu_ms, pair, error_state):
    """sensor NULL, zero sigmas, latency 0: X_hist, U_hist, stats, the plan and n_clipped of emu tsat_mpc_run_held (Rtab NULL) and,
    with an orbit table, of emu tsat_mpc_run_held_gg — byte for byte; Y_hist is X_hist"""
    b, po, plant, ids = pair["b"], pair["po"], pair["plant"], pair["ids"]
    o = hc.solve_options(ol, error_state=error_state)
    keys = ("X_hist", "U_hist", "stats", "X", "U", "tracking_stats", "n_clipped")
    old = hc.EmuMpcHeld(pkg._abi).run(b, o, po, N_STEPS, R, 1, plant, hc.SAT, ids, step0=3)
    new = emu_ms.run(b, o, po, N_STEPS, R, 1, None, None, 0, plant, hc.SAT, ids, step0=3)
    for k in keys:
        np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    np.testing.assert_array_equal(new["Y_hist"], new["X_hist"][:, :-1])
    zeros = emu_ms.run(b, o, po, N_STEPS, R, 1, mc.IDEAL, np.zeros((2, 9)), 0, plant, hc.SAT, ids, step0=3)
    for k in keys + ("Y_hist",):
        np.testing.assert_array_equal(new[k], zeros[k], err_msg=k)
    bg = gc.use_3u(pkg, hc.mpc_batch(pkg))
    bg.n_knots = b.n_knots
    Rtab = gc.orbit(pkg, bg.n_tab, 0.2)[None]
    oldg = gc.EmuGg(pkg._abi).held(bg, o, po, N_STEPS, R, 1, Rtab, gc.GM, plant, hc.SAT, ids)
    newg = emu_ms.run(bg, o, po, N_STEPS, R, 1, None, None, 0, plant, hc.SAT, ids, Rtab=Rtab, gm=gc.GM)
    for k in keys:
        np.testing.assert_array_equal(oldg[k], newg[k], err_msg="gg " + k)
    assert np.max(np.abs(oldg["X_hist"] - hc.EmuMpcHeld(pkg._abi).run(bg, o, po, N_STEPS, R, 1, plant, hc.SAT, ids)["X_hist"])) > 0.0


@pytest.mark.parametrize("latency", [0, 1])
def test_the_call_leaves_the_true_state_behind(pkg, ol, emu_ms, pair, latency):
    """after the call x0 of the parameter records is the TRUE x_{n_steps} (the last row of X_hist), not the measurement the loop
    kept there while it ran — a continuation, tsat_batch_run or tsat_tvlqr_resident start from it"""
    got = _emu(emu_ms, ol, pair, 0, latency)
    np.testing.assert_array_equal(got["x0_after"], got["X_hist"][:, -1])
    m_last = mc.measured(ol, pair["b"], pair["po"], np.concatenate([got["X_hist"][:, -1:], got["X_hist"][:, -1:]], axis=1), mc.SIGMAS,
                         pair["bias"], 0, pair["ids"], step0=N_STEPS)[:, 0]
    print(f"latency {latency}: the state left differs from its own measurement by {np.max(np.abs(got['x0_after'] - m_last)):.2e}")
    assert np.max(np.abs(got["x0_after"] - m_last)) > 1e-4


def test_rejected_arguments(pkg, emu_ms):
    """check_mpc_sensed, which the entry point calls beside its parents' checks: check_sensor with M = 1, and the Rtab / gm rule"""
    abi = pkg._abi
    good = sc.sensor_options(abi, mc.SIGMAS, 1)
    sensor = np.zeros((4, 9))
    Rtab = np.ones((1, 5, 3))
    assert emu_ms.check(good, sensor, 4) == (0, "") and emu_ms.check(good, None, 4) == (0, "")
    assert emu_ms.check(good, sensor, 4, Rtab, 0.0) == (0, "") and emu_ms.check(good, sensor, 4, Rtab, gc.GM) == (0, "")

    def so(**kw):
        o = abi.SensorOptions.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad(idx, val):
        z = sensor.copy()
        z[idx] = val
        return z

    for label, args, word in (
            ("s NULL", (None, sensor, 4), "null sensor options"),
            ("sigma_gyro negative", (so(sigma_gyro=-1e-9), sensor, 4), "must be finite and >= 0"),
            ("sigma_att NaN", (so(sigma_att=math.nan), sensor, 4), "must be finite and >= 0"),
            ("sigma_mag inf", (so(sigma_mag=math.inf), sensor, 4), "must be finite and >= 0"),
            ("latency 2", (so(latency=2), sensor, 4), "latency must be 0"),
            ("latency -1", (so(latency=-1), sensor, 4), "latency must be 0"),
            ("bias NaN", (good, bad((2, 4), np.nan), 4), "non-finite sensor entry at (t, m) = (2, 0)"),
            ("bias inf", (good, bad((3, 8), np.inf), 4), "non-finite sensor entry at (t, m) = (3, 0)"),
            ("Rtab NULL with gm", (good, sensor, 4, None, gc.GM), "Rtab may be NULL only with gm == 0"),
            ("Rtab NULL with gm NaN", (good, sensor, 4, None, math.nan), "Rtab may be NULL only with gm == 0")):
        rc, text = emu_ms.check(*args)
        assert rc == -1 and word in text, (label, text)
    # without a handle the entry point itself is a code, not a crash
    lib = abi.load()
    assert lib.tsat_mpc_run_held_sensed(None, None, None, 1, 0, 1, 1, None, None, None, None, None, None, None, None, None, None, None, 0.0,
                                        None, None, None) == -1
