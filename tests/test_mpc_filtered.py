"""CPU tier of the held re-planning loop behind the filter (tsat_mpc_run_held_filtered): the reference loop of
tests/mpc_filtered_common.py pinned with the filter off to the sensed reference, the source of
tortoisesat.jl_amd/csrc/tsat_mpc_filtered.hpp under the lane emulator against that reference, Y_hist and the filter's records checked
against the recursion run over the measurements of the returned true states (no solve involved), the continuation through
filt_init, f = NULL byte-equal to the emulated sensed loop, the state the call leaves behind, and what the entry point rejects (the
library's own validation function).

The case is that of tests/test_mpc_sensed.py: T = 2, N = 20, horizons (20, 13), all five plant dispersions, plant noise on,
generator ids (7, 2^33 + 1), R = 3 over 7 steps (blocks 3 + 3 + 1), sensor sigmas ``sensed_common.SIGMAS``, biases at twice
``sensed_common.BIAS``, limits +-5, statistic min_steps = 1, w_tol = 1e-2, angle_tol = 3.7; the filter levels are
``filtered_common.FILT``. Every parity case first asserts its conditions on references alone (mpc_filtered_common.conditions).
Measured on the reference over the five parametrised cases: margin 0.11, one of two fails, every block solve ends TSAT_MAX_OUTER; the
filter on against off moves the final state by 2.0e-5 (gains off) .. 1.1e-3, the gyro bias by 9.7e-5 .. 7.0e-4, latency 1 against 0
by 1.4e-6 (gains off) .. 1.0e-3, the prediction across the delay by 9.9e-7 (gains off) .. 5.1e-4 (bar gg_common.MOVED = 1e-7).
Measured on the emulator against it: max |dX_hist| 1.7e-16, |dU_hist| 5.4e-12, |dY_hist| 3.3e-16, |dfilt_state| 2.2e-16,
|dfilt_final| 4.0e-17; against the recursion over ``measure`` of the returned X_hist 2.2e-16; the continuation through filt_init
bit-equal, without it 3.2e-4 off."""
import ctypes as C
import math

import numpy as np
import pytest

import filtered_common as fc
import gg_common as gc
import mpc_filtered_common as mf
import mpc_held_common as hc
import mpc_sensed_common as mc

N_STEPS, R = 7, 3
W_TOL, ANGLE_TOL = 1e-2, 3.7
LIMITS = (np.full(3, -5.0), np.full(3, 5.0))


@pytest.fixture(scope="module")
def emu_mf(pkg):
    return mf.EmuMpcFiltered(pkg._abi)


@pytest.fixture(scope="module")
def pair(pkg, ol):
    """the case, and its references by their arguments, each computed once and left unchanged"""
    b = hc.mpc_batch(pkg)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = hc.noise_options(ol, min_steps=1, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant, ids, bias = hc.plants(pkg, b), np.array([7, 2 ** 33 + 1], dtype=np.int64), mc.biases(pkg, 2)
    refs = {}

    def ref(es, latency, fb=1, filt=mf.FILT, bias=bias, predict=True, n=N_STEPS, R=R, filt_init=None, step0=0, batch=b):
        key = (es, latency, fb, None if filt is None else tuple(sorted(filt.items())), bias.tobytes(), predict, n, R,
               None if filt_init is None else filt_init.tobytes(), step0, batch.x0.tobytes())
        if key not in refs:
            refs[key] = mf.reference_loop(ol, batch, hc.solve_options(ol, error_state=es), n, R, fb, po, mc.SIGMAS, bias, latency, plant,
                                          LIMITS, ids, step0=step0, filt=filt, filt_init=filt_init, predict=predict)
        return refs[key]

    return dict(b=b, po=po, plant=plant, ids=ids, bias=bias, ref=ref)


def _emu(emu_mf, ol, p, es, latency, fb=1, n=N_STEPS, R=R, batch=None, **kw):
    return emu_mf.run(p["b"] if batch is None else batch, hc.solve_options(ol, error_state=es), p["po"], n, R, fb, mc.SIGMAS, p["bias"], latency,
                      p["plant"], LIMITS, p["ids"], **kw)


def test_reference_with_the_filter_off_is_the_sensed_reference(pkg, ol, pair):
    """the reference's own pin: filt = None — max |d| = 0 against mpc_sensed_common.reference_loop, either latency, with step0"""
    b, po, plant, ids, bias = pair["b"], pair["po"], pair["plant"], pair["ids"], pair["bias"]
    for es, latency, fb in ((0, 0, 1), (1, 1, 1), (0, 1, 0)):
        o = hc.solve_options(ol, error_state=es)
        old = mc.reference_loop(ol, b, o, N_STEPS, R, fb, po, mc.SIGMAS, bias, latency, plant, LIMITS, ids, step0=2)
        new = mf.reference_loop(ol, b, o, N_STEPS, R, fb, po, mc.SIGMAS, bias, latency, plant, LIMITS, ids, step0=2, filt=None)
        d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_hist", "U_hist", "Y_hist", "X", "U"))
        print(f"error_state {es} latency {latency} feedback {fb}: max|d| against the sensed reference {d:.2e}")
        assert d == 0.0
        assert np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["tracking_stats"], new["tracking_stats"])
        assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["tally"], new["tally"])


@pytest.mark.parametrize("error_state,latency,feedback", [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 1, 0)])
def test_emulated_loop_matches_reference(pkg, ol, emu_mf, pair, error_state, latency, feedback):
    """R = 3, 7 steps (blocks 3 + 3 + 1) to the project's MPC bars, the last plan with them; Y_hist and the filter's records to 1e-9.
    The conditions of the case are asserted on references alone first."""
    b, po, bias = pair["b"], pair["po"], pair["bias"]
    ref = mf.conditions(lambda **over: pair["ref"](error_state, **{"latency": latency, "fb": feedback, **over}), bias,
                        f"error_state {error_state} latency {latency} feedback {feedback}", b, po)
    assert ref["n_solves"] == 3
    got = _emu(emu_mf, ol, pair, error_state, latency, feedback)
    hc.same(ref, got, b, po, plan=True)
    mf.same_estimates(ref, got)


@pytest.mark.parametrize("latency", [0, 1])
def test_y_hist_is_the_filter_run_over_the_measurements_of_the_returned_true_states(pkg, ol, emu_mf, pair, latency):
    """Y_hist, filt_state and filt_final = the Ekf over measure(X_hist) with the latency shift, to 1e-9: no solve is involved. The
    estimate is neither the true state nor the raw measurement, and at latency 1 the steps 0 and 1 share the filter's sample 0"""
    got = _emu(emu_mf, ol, pair, 0, latency, step0=4)
    handed = mc.measured(ol, pair["b"], pair["po"], got["X_hist"], mc.SIGMAS, pair["bias"], latency, pair["ids"], step0=4)
    Y, S, F = mf.estimates(ol, pair["b"], mf.FILT, handed, latency)
    mf.same_estimates(dict(Y_hist=Y, filt_state=S, filt_final=F), got)
    off_true = float(np.max(np.abs(got["Y_hist"] - got["X_hist"][:, :-1])))
    off_raw = float(np.max(np.abs(got["Y_hist"][:, 1:] - handed[:, 1:])))
    print(f"latency {latency}: max|Y_hist - X_hist| {off_true:.2e}, max|Y_hist - raw| after step 0 {off_raw:.2e}")
    assert off_true > 1e-4 and off_raw > 1e-6
    np.testing.assert_array_equal(got["Y_hist"][:, 0, 0:3], handed[:, 0, 0:3])          # `first`: w^ = w_m
    if latency:
        np.testing.assert_array_equal(got["Y_hist"][:, 1, 0:3], got["Y_hist"][:, 0, 0:3])   # s = 1: no step, w^ unchanged
        assert np.max(np.abs(got["Y_hist"][:, 1, 3:7] - got["Y_hist"][:, 0, 3:7])) > 0.0   # but the attitude is predicted


def _continued(b, first, r_len):
    """the resident batch as the first call leaves it: the true state, the clock advanced by one rounded addition per step, the
    last plan shifted by the last block's steps inside each trajectory's own horizon"""
    b2 = b.slice(0, b.T)
    n = first["X_hist"].shape[1] - 1
    tau = b.tau0.copy()
    for _ in range(n):
        tau = tau + b.dtau
    U0 = b.U0.copy()
    for t in range(b.T):
        nt = int(b.n_knots[t])
        U0[t, :nt - 1] = first["U"][t, np.minimum(np.arange(nt - 1) + r_len, nt - 2)]
    b2.x0, b2.tau0, b2.U0 = np.ascontiguousarray(first["x0_after"]), np.ascontiguousarray(tau), np.ascontiguousarray(U0)
    return b2


def test_continuation_with_filt_init_is_the_longer_run(pkg, ol, emu_mf, pair):
    """6 + 6 steps at R = 3, latency 0, step0 = 6, filt_init = the first call's filt_state: the 12-step run, bit for bit, records
    included. Without filt_init the second call restarts the filter and differs by >= gg_common.MOVED (asserted on the references
    first, then seen on the emulator)."""
    b = pair["b"]
    ref12 = pair["ref"](0, 0, n=12)
    ref6 = pair["ref"](0, 0, n=6)
    b2r = _continued(b, dict(ref6, x0_after=ref6["X_hist"][:, -1]), 3)
    with_init = pair["ref"](0, 0, n=6, step0=6, filt_init=ref6["filt_state"], batch=b2r)
    without = pair["ref"](0, 0, n=6, step0=6, batch=b2r)
    assert np.max(np.abs(with_init["X_hist"][:, -1] - ref12["X_hist"][:, -1])) < 1e-9
    mc.moved(with_init, without, "continuation: filt_init given against a restarted filter")
    whole = _emu(emu_mf, ol, pair, 0, 0, n=12)
    first = _emu(emu_mf, ol, pair, 0, 0, n=6)
    np.testing.assert_array_equal(first["x0_after"], first["X_hist"][:, -1])
    b2 = _continued(b, first, 3)
    second = _emu(emu_mf, ol, pair, 0, 0, n=6, batch=b2, step0=6, filt_init=first["filt_state"])
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(np.concatenate([first["Y_hist"], second["Y_hist"]], axis=1), whole["Y_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("filt_state", "filt_final", "X", "U", "stats"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)
    restarted = _emu(emu_mf, ol, pair, 0, 0, n=6, batch=b2, step0=6)
    d = float(np.max(np.abs(restarted["X_hist"][:, -1] - whole["X_hist"][:, -1])))
    print(f"without filt_init the continuation's final state differs from the longer run's by {d:.2e}")
    assert d >= gc.MOVED
    hc.same(without, restarted, b2, pair["po"])
    mf.same_estimates(without, restarted)


@pytest.mark.parametrize("error_state,latency", [(0, 0), (1, 1)])
def test_null_filter_is_byte_equal_to_the_emulated_sensed_loop(pkg, ol, emu_mf, pair, error_state, latency):
    """f = NULL: every output of emu tsat_mpc_run_held_sensed, byte for byte; no filter outputs"""
    b, po = pair["b"], pair["po"]
    o = hc.solve_options(ol, error_state=error_state)
    old = mc.EmuMpcSensed(pkg._abi).run(b, o, po, N_STEPS, R, 1, mc.SIGMAS, pair["bias"], latency, pair["plant"], LIMITS, pair["ids"], step0=3)
    new = _emu(emu_mf, ol, pair, error_state, latency, step0=3, filt=None)
    for k in ("X_hist", "U_hist", "Y_hist", "stats", "X", "U", "tracking_stats", "n_clipped", "x0_after"):
        np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    assert new["filt_state"] is None and new["filt_final"] is None
    on = _emu(emu_mf, ol, pair, error_state, latency, step0=3)
    assert np.max(np.abs(on["X_hist"][:, -1] - new["X_hist"][:, -1])) >= gc.MOVED      # the filter is not a no-op on this case


@pytest.mark.parametrize("latency", [0, 1])
def test_the_call_leaves_the_true_state_behind(pkg, ol, emu_mf, pair, latency):
    """after the call x0 of the parameter records is the TRUE x_{n_steps} (the last row of X_hist), not the estimate the loop kept
    there while it ran"""
    got = _emu(emu_mf, ol, pair, 0, latency)
    np.testing.assert_array_equal(got["x0_after"], got["X_hist"][:, -1])
    d = float(np.max(np.abs(got["x0_after"] - got["Y_hist"][:, -1])))
    print(f"latency {latency}: the state left differs from the last estimate by {d:.2e}")
    assert d > 1e-4


def test_rejected_arguments(pkg, emu_mf):
    """check_mpc_filtered, which the entry point calls beside its parents' checks: check_filter, the f = NULL rule, filt_init"""
    abi = pkg._abi
    good = fc.filter_options(abi, mf.FILT)
    init = np.tile(np.r_[1.0, np.zeros(30)], (4, 1))
    out31, out9 = np.zeros((4, 31)), np.zeros((4, 9))
    assert emu_mf.check(good, None, 4) == (0, "") and emu_mf.check(good, init, 4, out31, out9) == (0, "")
    assert emu_mf.check(None, None, 4) == (0, "")

    def fo(**kw):
        o = abi.FilterOptions.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad(idx, val):
        z = init.copy()
        z[idx] = val
        return z

    for label, args, word in (
            ("sigma_v NaN", (fo(sigma_v=math.nan), None, 4), "must be finite and >= 0"),
            ("sigma_u inf", (fo(sigma_u=math.inf), None, 4), "must be finite and >= 0"),
            ("sigma_a negative", (fo(sigma_a=-1e-3), None, 4), "must be finite and >= 0"),
            ("p0_att negative", (fo(p0_att=-1.0), None, 4), "must be finite and >= 0"),
            ("p0_bias NaN", (fo(p0_bias=math.nan), None, 4), "must be finite and >= 0"),
            ("sigma_a zero", (fo(sigma_a=0.0), None, 4), "sigma_a must be > 0"),
            ("reserved 1", (fo(reserved=1), None, 4), "reserved must be 0"),
            ("f NULL with filt_init", (None, init, 4), "must be NULL when f is NULL"),
            ("f NULL with filt_state", (None, None, 4, out31), "must be NULL when f is NULL"),
            ("f NULL with filt_final", (None, None, 4, None, out9), "must be NULL when f is NULL"),
            ("filt_init NaN", (good, bad((2, 17), math.nan), 4), "non-finite filt_init entry at t = 2"),
            ("filt_init inf", (good, bad((3, 30), math.inf), 4), "non-finite filt_init entry at t = 3"),
            ("q^ of zero norm", (good, bad((1, 0), 0.0), 4), "q^ of zero norm at t = 1")):
        rc, text = emu_mf.check(*args)
        assert rc == -1 and word in text, (label, text)
    # without a handle the entry point itself is a code, not a crash: with f, and with f NULL (the sensed call)
    lib = abi.load()
    tail = (None,) * 11 + (0.0, None, None, None)
    assert lib.tsat_mpc_run_held_filtered(None, None, None, 1, 0, 1, 1, *tail, C.byref(good), None, None, None) == -1
    assert lib.tsat_mpc_run_held_filtered(None, None, None, 1, 0, 1, 1, *tail, None, None, None, None) == -1
