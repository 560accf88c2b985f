"""CPU tier of the held re-planning loop behind the magnetometer-updated nine-state filter (tsat_mpc_run_held_model_mag_filtered):
the reference loop of tests/mpc_model_mag_filtered_common.py pinned to the sensed and the model-filtered references, the source of
tortoisesat.jl_amd/csrc/tsat_mpc_model_mag_filtered.hpp under the lane emulator against that reference, Y_hist and the filter's
records checked against the recursion run over the gyro and magnetometer samples of the returned true states with the returned
commands and the clock's own rows (no solve involved), one step and the steps without an update, the continuation through filt_init,
f = NULL byte-equal to the emulated sensed loop, the state the call leaves behind, zero field rows, what the entry point rejects
(the library's own validation function) and the host layer's argument handling.

The case is that of tests/test_mpc_model_filtered.py: T = 2, N = 20, horizons (20, 13), the ``coarse_rows`` table (rows 10 s
apart), all five plant dispersions, plant noise on, generator ids (7, 2^33 + 1), R = 3 over 7 steps (blocks 3 + 3 + 1), limits +-12,
sensor sigmas ``sensed_common.SIGMAS``, biases at twice ``sensed_common.BIAS``, statistic min_steps = 1, w_tol = 1e-2, angle_tol =
3.7; the filter levels are ``model_mag_filtered_common.FILT``. Every parity case first asserts its conditions on references alone
(mpc_model_mag_filtered_common.conditions; every figure is printed). The measured figures are in
profiles/mpc/model_mag_filtered_differences.txt."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import dispersed_common as dc
import gg_common as gc
import model_filtered_common as mm
import model_mag_filtered_common as mg
import mpc_held_common as hc
import mpc_model_filtered_common as mf
import mpc_model_mag_filtered_common as mq
import mpc_sensed_common as mc

N_STEPS, R = 7, 3
W_TOL, ANGLE_TOL = 1e-2, 3.7
LIMITS = (np.full(3, -12.0), np.full(3, 12.0))
# with the gains off the estimate acts through the x0 of the solves at steps 3 and 6 alone: the clock's off-by-one moves the final
# state by 3e-9 there, as it does behind the parent, which leaves it to the four cases with the gains on (1e-5 .. 5e-5); so does this
# test
GAINS_OFF_SKIP = (mq.ROWS,)


@pytest.fixture(scope="module")
def emu_mq(pkg):
    return mq.EmuMpcModelMagFiltered(pkg._abi)


@pytest.fixture(scope="module")
def pair(pkg, ol):
    """the case, and its references by their arguments, each computed once and left unchanged"""
    b = mq.coarse_rows(pkg, hc.mpc_batch(pkg))
    b.n_knots = np.array([20, 13], dtype=np.int32)
    po = hc.noise_options(ol, min_steps=1, w_tol=W_TOL, angle_tol=ANGLE_TOL)
    plant, ids, bias = hc.plants(pkg, b), np.array([7, 2 ** 33 + 1], dtype=np.int64), mc.biases(pkg, 2)
    refs = {}

    def ref(es, latency, fb=1, filt=mq.FILT, variant=mq.VARIANT, n=N_STEPS, R=R, filt_init=None, step0=0, batch=b):
        key = (es, latency, fb, None if filt is None else tuple(sorted(filt.items())), tuple(sorted(variant.items())), n, R,
               None if filt_init is None else filt_init.tobytes(), step0, batch.x0.tobytes(), batch.Btab.tobytes())
        if key not in refs:
            refs[key] = mq.reference_loop(ol, batch, hc.solve_options(ol, error_state=es), n, R, fb, po, mc.SIGMAS, bias, latency, plant,
                                          LIMITS, ids, step0=step0, filt=filt, filt_init=filt_init, variant=variant)
        return refs[key]

    def parent(es, latency, fb=1):
        return mf.reference_loop(ol, b, hc.solve_options(ol, error_state=es), N_STEPS, R, fb, po, mc.SIGMAS, bias, latency, plant, LIMITS,
                                 ids, filt=mf.FILT)

    return dict(b=b, po=po, plant=plant, ids=ids, bias=bias, ref=ref, parent=parent)


def _emu(emu_mq, ol, p, es, latency, fb=1, n=N_STEPS, R=R, batch=None, **kw):
    return emu_mq.run(p["b"] if batch is None else batch, hc.solve_options(ol, error_state=es), p["po"], n, R, fb, mc.SIGMAS, p["bias"], latency,
                      p["plant"], LIMITS, p["ids"], **kw)


def test_reference_is_pinned_to_the_sensed_and_the_model_filtered_references(pkg, ol, pair):
    """the new loop's own pin, max |d| = 0, both latencies, step0 = 2: with no estimator against
    mpc_sensed_common.reference_loop; with the attitude-updated ``reference_rollout.ModelState`` (which ignores b_m) as estimator
    against mpc_model_filtered_common.reference_loop"""
    b, po, plant, ids, bias = pair["b"], pair["po"], pair["plant"], pair["ids"], pair["bias"]
    for es, latency, fb in ((0, 0, 1), (1, 1, 1), (0, 1, 0)):
        o = hc.solve_options(ol, error_state=es)
        args = (ol, b, o, N_STEPS, R, fb, po, mc.SIGMAS, bias, latency, plant, LIMITS, ids)
        for name, old, new in (
                ("sensed", mc.reference_loop(*args, step0=2), mq.reference_loop(*args, step0=2, filt=None)),
                ("model-filtered", mf.reference_loop(*args, step0=2, filt=mf.FILT),
                 mq.reference_loop(*args, step0=2, est=mf.estimator(ol, b, float(o.u_scale), mf.FILT, plant)))):
            keys = ("X_hist", "U_hist", "Y_hist", "X", "U") + (("filt_state", "filt_final") if name == "model-filtered" else ())
            d = max(float(np.max(np.abs(old[k] - new[k]))) for k in keys)
            print(f"error_state {es} latency {latency} feedback {fb}: max|d| against the {name} reference {d:.2e}")
            assert d == 0.0
            assert np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["tracking_stats"], new["tracking_stats"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["tally"], new["tally"])


@pytest.mark.parametrize("error_state,latency,feedback", [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 1, 0)])
def test_emulated_loop_matches_reference(pkg, ol, emu_mq, pair, error_state, latency, feedback):
    """R = 3, 7 steps (blocks 3 + 3 + 1) to the project's MPC bars, the last plan with them; Y_hist and the filter's records to 1e-9;
    U_hist 1e-8 where nothing clips. The conditions of the case are asserted on references alone first. Every trajectory is
    compared."""
    b, po = pair["b"], pair["po"]
    ref = mq.conditions(lambda **over: pair["ref"](error_state, **{"latency": latency, "fb": feedback, **over}),
                        f"error_state {error_state} latency {latency} feedback {feedback}", b, po,
                        parent=lambda: pair["parent"](error_state, latency, feedback), skip=() if feedback else GAINS_OFF_SKIP)
    assert ref["n_solves"] == 3
    got = _emu(emu_mq, ol, pair, error_state, latency, feedback)
    assert hc.same(ref, got, b, po, plan=True).all()
    mq.same_estimates(ref, got)
    free = (ref["n_maybe"] == 0)
    if free.any():
        dU = float(np.max(np.abs(ref["U_hist"][free] - got["U_hist"][free])))
        print(f"max|dU_hist| where nothing clips {dU:.2e}")
        assert dU < 1e-8


@pytest.mark.parametrize("latency", [0, 1])
def test_y_hist_is_the_filter_run_over_the_measurements_of_the_returned_true_states(pkg, ol, emu_mq, pair, latency):
    """Y_hist, filt_state and filt_final = the ModelMagEkf over the gyro and magnetometer samples of X_hist — the field against the
    clock's own stage-0 rows, the Philox knot step0 + s —, the returned U_hist and the clock's rows, to 1e-9, step0 = 4: no solve is
    involved. A wrong row, a wrong knot in the counter or a sample taken from the estimate fails here. The estimate is neither the
    true state nor the raw measurement"""
    got = _emu(emu_mq, ol, pair, 0, latency, step0=4)
    handed = mq.measured(ol, pair["b"], pair["po"], got["X_hist"], mc.SIGMAS, pair["bias"], latency, pair["ids"], step0=4)
    Y, S, F = mq.estimates(ol, pair["b"], hc.solve_options(ol).u_scale, mq.FILT, handed, got["U_hist"], latency)
    mq.same_estimates(dict(Y_hist=Y, filt_state=S, filt_final=F), got)
    off_true = float(np.max(np.abs(got["Y_hist"] - got["X_hist"][:, :-1])))
    off_raw = float(np.max(np.abs(got["Y_hist"][:, 1:] - handed[0][:, 1:])))
    print(f"latency {latency}: max|Y_hist - X_hist| {off_true:.2e}, max|Y_hist - raw| after step 0 {off_raw:.2e}")
    assert off_true > 1e-4 and off_raw > 1e-6
    np.testing.assert_array_equal(got["Y_hist"][:, 0, 0:3], handed[0][:, 0, 0:3])          # `first`: w^ = w_m
    np.testing.assert_array_equal(got["filt_state"][:, 10:13], got["U_hist"][:, -1])      # the record's command: the closing predict's
    # the wrong knot or the wrong row would show: the recursion over samples drawn at knot s (not step0 + s) is off the bar
    wrong = mq.measured(ol, pair["b"], pair["po"], got["X_hist"], mc.SIGMAS, pair["bias"], latency, pair["ids"], step0=0)
    Yw, _, _ = mq.estimates(ol, pair["b"], hc.solve_options(ol).u_scale, mq.FILT, wrong, got["U_hist"], latency)
    assert np.max(np.abs(Yw - got["Y_hist"])) > mq.EST_BAR


def test_one_step_leaves_first_plus_one_predict(pkg, ol, emu_mq, pair):
    """n_steps = 1: the record left is first(m_0) carried across step 0 by the closing predict, either latency: no update is made,
    b^ = 0 and P_tt has grown"""
    for latency in (0, 1):
        ref = pair["ref"](0, latency, n=1)
        got = _emu(emu_mq, ol, pair, 0, latency, n=1)
        mq.same_estimates(ref, got)
        handed = mq.measured(ol, pair["b"], pair["po"], got["X_hist"], mc.SIGMAS, pair["bias"], latency, pair["ids"])
        Y, S, F = mq.estimates(ol, pair["b"], hc.solve_options(ol).u_scale, mq.FILT, handed, got["U_hist"], latency)
        mq.same_estimates(dict(Y_hist=Y, filt_state=S, filt_final=F), got)
        first = mg.first_record(mq.FILT)
        np.testing.assert_array_equal(got["filt_final"][:, 0:3], 0.0)                       # b^ = 0: no update was made
        assert np.all(got["filt_final"][:, 3:6] > first[3:6])                              # P_tt grew across the step
        np.testing.assert_array_equal(got["filt_state"][:, 10:13], got["U_hist"][:, 0])


def test_two_steps_at_latency_1_make_no_update(pkg, ol, emu_mq, pair):
    """n_steps = 2 at latency 1: m_0 is handed over twice, the record is first(m_0) and two predicts — b^ = 0 still — and y_1 is the
    model prediction, which differs from y_0 in the rate too"""
    ref = pair["ref"](0, 1, n=2, R=2)
    got = _emu(emu_mq, ol, pair, 0, 1, n=2, R=2)
    mq.same_estimates(ref, got)
    np.testing.assert_array_equal(got["filt_final"][:, 0:3], 0.0)
    assert np.max(np.abs(got["Y_hist"][:, 1, 0:3] - got["Y_hist"][:, 0, 0:3])) > 0.0
    np.testing.assert_array_equal(got["filt_state"][:, 10:13], got["U_hist"][:, 1])


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


def test_continuation_with_filt_init_is_the_longer_run(pkg, ol, emu_mq, pair):
    """6 + 6 steps at R = 3, latency 0, step0 = 6, filt_init = the first call's filt_state: the 12-step run, bit for bit — X_hist,
    U_hist, Y_hist, the records, the last plan and its stats. Without filt_init the second call restarts the filter and differs by
    >= gg_common.MOVED (asserted on the references first, then seen on the emulator)."""
    b = pair["b"]
    ref12 = pair["ref"](0, 0, n=12)
    ref6 = pair["ref"](0, 0, n=6)
    b2r = _continued(b, dict(ref6, x0_after=ref6["X_hist"][:, -1]), 3)
    with_init = pair["ref"](0, 0, n=6, step0=6, filt_init=ref6["filt_state"], batch=b2r)
    without = pair["ref"](0, 0, n=6, step0=6, batch=b2r)
    assert np.max(np.abs(with_init["X_hist"][:, -1] - ref12["X_hist"][:, -1])) < 1e-9
    mc.moved(with_init, without, "continuation: filt_init given against a restarted filter")
    whole = _emu(emu_mq, ol, pair, 0, 0, n=12)
    first = _emu(emu_mq, ol, pair, 0, 0, n=6)
    np.testing.assert_array_equal(first["x0_after"], first["X_hist"][:, -1])
    b2 = _continued(b, first, 3)
    second = _emu(emu_mq, ol, pair, 0, 0, n=6, batch=b2, step0=6, filt_init=first["filt_state"])
    np.testing.assert_array_equal(np.concatenate([first["X_hist"][:, :-1], second["X_hist"]], axis=1), whole["X_hist"])
    np.testing.assert_array_equal(np.concatenate([first["U_hist"], second["U_hist"]], axis=1), whole["U_hist"])
    np.testing.assert_array_equal(np.concatenate([first["Y_hist"], second["Y_hist"]], axis=1), whole["Y_hist"])
    np.testing.assert_array_equal(first["n_clipped"] + second["n_clipped"], whole["n_clipped"])
    for k in ("filt_state", "filt_final", "X", "U", "stats"):
        np.testing.assert_array_equal(second[k], whole[k], err_msg=k)
    restarted = _emu(emu_mq, ol, pair, 0, 0, n=6, batch=b2, step0=6)
    d = float(np.max(np.abs(restarted["X_hist"][:, -1] - whole["X_hist"][:, -1])))
    print(f"without filt_init the continuation's final state differs from the longer run's by {d:.2e}")
    assert d >= gc.MOVED
    hc.same(without, restarted, b2, pair["po"])
    mq.same_estimates(without, restarted)


@pytest.mark.parametrize("error_state,latency", [(0, 0), (1, 1)])
def test_null_filter_is_byte_equal_to_the_emulated_sensed_loop(pkg, ol, emu_mq, pair, error_state, latency):
    """f = NULL: every output of emu tsat_mpc_run_held_sensed, byte for byte; no filter outputs"""
    b, po = pair["b"], pair["po"]
    o = hc.solve_options(ol, error_state=error_state)
    old = mc.EmuMpcSensed(pkg._abi).run(b, o, po, N_STEPS, R, 1, mc.SIGMAS, pair["bias"], latency, pair["plant"], LIMITS, pair["ids"], step0=3)
    new = _emu(emu_mq, ol, pair, error_state, latency, step0=3, filt=None)
    for k in ("X_hist", "U_hist", "Y_hist", "stats", "X", "U", "tracking_stats", "n_clipped", "x0_after"):
        np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    assert new["filt_state"] is None and new["filt_final"] is None
    on = _emu(emu_mq, ol, pair, error_state, latency, step0=3)
    assert np.max(np.abs(on["X_hist"][:, -1] - new["X_hist"][:, -1])) >= gc.MOVED      # the filter is not a no-op on this case


@pytest.mark.parametrize("latency", [0, 1])
def test_the_call_leaves_the_true_state_behind(pkg, ol, emu_mq, pair, latency):
    """after the call x0 of the parameter records is the TRUE x_{n_steps} (the last row of X_hist), not the estimate the loop kept
    there while it ran"""
    got = _emu(emu_mq, ol, pair, 0, latency)
    np.testing.assert_array_equal(got["x0_after"], got["X_hist"][:, -1])
    d = float(np.max(np.abs(got["x0_after"] - got["Y_hist"][:, -1])))
    print(f"latency {latency}: the state left differs from the last estimate by {d:.2e}")
    assert d > 1e-4


@pytest.mark.parametrize("latency", [0, 1])
def test_zero_field_rows(pkg, ol, emu_mq, pair, latency):
    """``model_mag_filtered_common.zero_row_batch``'s device on the held clock: the table rows that are the stage-0 rows of steps 2
    and 3 set to zero. Hm = 0 and K = 0 there — an update that changes nothing, without a branch: reference parity
    holds and nothing is non-finite"""
    b = pair["b"]
    Bt = b.Btab.copy()
    Bt[0, 2:4] = 0.0                  # the case's clock reads one row a step from row 0: rows 2 and 3 are r_2 and r_3
    bz = dataclasses.replace(b, Btab=np.ascontiguousarray(Bt))
    for s in (2, 3):
        assert np.array_equal(dc._row(dataclasses.replace(bz, tau0=bz.tau0 + s * bz.dtau), 0, 0, 0.0), np.zeros(3))
    ref = pair["ref"](0, latency, batch=bz)
    got = _emu(emu_mq, ol, pair, 0, latency, batch=bz)
    for k in ("X_hist", "U_hist", "Y_hist", "filt_state", "filt_final"):
        assert np.isfinite(got[k]).all() and np.isfinite(ref[k]).all(), k
    hc.same(ref, got, bz, pair["po"])
    mq.same_estimates(ref, got)
    assert np.max(np.abs(ref["X_hist"][:, -1] - pair["ref"](0, latency)["X_hist"][:, -1])) > 0.0      # the zero rows are read


def test_rejected_arguments(pkg, emu_mq):
    """check_mpc_model_mag_filtered, which the entry point calls beside its parents' checks: check_model_mag_filter, the f = NULL
    rule, filt_init"""
    abi = pkg._abi
    good = mg.filter_options(abi, mq.FILT)
    init = np.tile(np.r_[1.0, np.zeros(57)], (4, 1))
    out58, out12 = np.zeros((4, 58)), np.zeros((4, 12))
    assert emu_mq.check(good, None, 4) == (0, "") and emu_mq.check(good, init, 4, out58, out12) == (0, "")
    assert emu_mq.check(None, None, 4) == (0, "")

    def fo(**kw):
        o = abi.ModelMagFilterOptions.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad(idx, val):
        z = init.copy()
        z[idx] = val
        return z

    for label, args, word in (
            ("sigma_v NaN", (fo(sigma_v=math.nan), None, 4), "must be finite and >= 0"),
            ("sigma_w negative", (fo(sigma_w=-1e-6), None, 4), "must be finite and >= 0"),
            ("sigma_w inf", (fo(sigma_w=math.inf), None, 4), "must be finite and >= 0"),
            ("sigma_u inf", (fo(sigma_u=math.inf), None, 4), "must be finite and >= 0"),
            ("sigma_m negative", (fo(sigma_m=-1e-9), None, 4), "must be finite and >= 0"),
            ("sigma_g NaN", (fo(sigma_g=math.nan), None, 4), "must be finite and >= 0"),
            ("p0_att negative", (fo(p0_att=-1.0), None, 4), "must be finite and >= 0"),
            ("p0_bias NaN", (fo(p0_bias=math.nan), None, 4), "must be finite and >= 0"),
            ("sigma_m zero", (fo(sigma_m=0.0), None, 4), "sigma_m must be > 0"),
            ("sigma_g zero", (fo(sigma_g=0.0), None, 4), "sigma_g must be > 0"),
            ("reserved 1", (fo(reserved=1), None, 4), "reserved must be 0"),
            ("f NULL with filt_init", (None, init, 4), "must be NULL when f is NULL"),
            ("f NULL with filt_state", (None, None, 4, out58), "must be NULL when f is NULL"),
            ("f NULL with filt_final", (None, None, 4, None, out12), "must be NULL when f is NULL"),
            ("filt_init NaN", (good, bad((2, 17), math.nan), 4), "non-finite filt_init entry at t = 2"),
            ("filt_init inf", (good, bad((3, 57), math.inf), 4), "non-finite filt_init entry at t = 3"),
            ("q^ of zero norm", (good, bad((1, 0), 0.0), 4), "q^ of zero norm at t = 1")):
        rc, text = emu_mq.check(*args)
        assert rc == -1 and word in text, (label, text)
    # without a handle the entry point itself is a code, not a crash: with f, and with f NULL (the sensed call)
    lib = abi.load()
    tail = (None,) * 11 + (0.0, None, None, None)
    assert lib.tsat_mpc_run_held_model_mag_filtered(None, None, None, 1, 0, 1, 1, *tail, C.byref(good), None, None, None) == -1
    assert lib.tsat_mpc_run_held_model_mag_filtered(None, None, None, 1, 0, 1, 1, *tail, None, None, None, None) == -1


def test_host_layer_argument_handling(pkg):
    """mpc.receding_horizon_held_model_mag_filtered: what it refuses before anything reaches the library"""
    mpc = pkg.mpc
    assert mpc.MODEL_FILTER_STATE_W == mq.STATE_W == 58
    with pytest.raises(ValueError, match="filter must be None"):
        mpc.receding_horizon_held_model_mag_filtered(None, None, 1, 1, filter=3.0)
    with pytest.raises(ValueError, match="filter must be None"):           # the attitude-updated filter's options are not this filter's
        mpc.receding_horizon_held_model_mag_filtered(None, None, 1, 1, filter=mm.filter_options(pkg._abi, mm.FILT))
    with pytest.raises(ValueError, match="sigma_g and sigma_m must be positive"):
        mpc.receding_horizon_held_model_mag_filtered(None, None, 1, 1, filter=dict(sigma_w=1e-4, sigma_g=1e-3, sigma_m=0.0))
    with pytest.raises(ValueError, match="unknown tsat_sensor_options"):
        mpc.receding_horizon_held_model_mag_filtered(None, None, 1, 1, filter=dict(sigma_w=1e-4, sigma_g=1e-3, sigma_m=5e-7),
                                                     sensor_opts=dict(sigma_gyroscope=1.0))
