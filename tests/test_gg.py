"""CPU tier of the gravity-gradient entry points (tsat_tvlqr_ensemble_gg, tsat_mpc_run_held_gg): the references of
tests/gg_common.py pinned at gm = 0 to their parents, the kernel source of tortoisesat.jl_amd/csrc/tsat_gg.hpp under the lane
emulator against them (bars of dispersed_common.compare and mpc_dispersed_common.same), gm = 0 through the new code bit-equal to
the emulated parents, and what the entry points reject (the library's own validation function).

Measured on the references (T = 2, N = 20, 3U model inertia, all five dispersions, noise on, limits +-0.6): the term moves the final
state of the ensemble by 3.0e-6 and of the held loop by 1.7e-6 (the bar is 1e-7)."""
import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import sensed_common as sc

IDS = np.array([7, 2 ** 33 + 1], dtype=np.int64)


@pytest.fixture(scope="module")
def emu(pkg):
    return gc.EmuGg(pkg._abi)


def _pair(pkg):
    """T = 2, N = 20, horizons (20, 13), the 3U inertia, one field table and the orbit rows it was sampled on"""
    b = gc.use_3u(pkg, hc.mpc_batch(pkg))
    b.n_knots = np.array([20, 13], dtype=np.int32)
    return b, gc.orbit(pkg, b.n_tab, 0.2)[None]


@pytest.fixture(scope="module")
def ens_case(pkg, ol):
    """the pair solved by the oracle (1 x 3 budget), its gains from the model inertia, M = 3 realisations"""
    b, Rtab = _pair(pkg)
    r = ol.solve_batch(b, hc.solve_options(ol))
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 3, np.random.default_rng(5))
    o = ec.tv_options(ol)
    o.min_steps, o.w_tol, o.angle_tol = hc.MIN_STEPS, hc.W_TOL, hc.ANGLE_TOL
    return b, Rtab, r["X"], r["U"], Qd, Qfd, Rd, x0s, K, o, dc.all_five_plants(pkg, b, 3)


def test_references_at_gm0_are_their_parents(pkg, ol, ens_case):
    """the pin of both references: gm = 0 is the parent reference, max |d| = 0"""
    b, Rtab, X, U, Qd, Qfd, Rd, x0s, K, o, plant = ens_case
    pairs = np.concatenate([dc.all_pairs(b.T, 3), [(0, -1), (1, -1)]])
    old = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, plant=plant, sat=hc.SAT, noise_id0=IDS)
    new = gc.ensemble_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, Rtab, 0.0, plant=plant, sat=hc.SAT, noise_id0=IDS)
    d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
    print(f"ensemble reference at gm = 0 against dispersed_common: max|d| {d:.1e}")
    assert d == 0.0 and np.array_equal(old["stats"], new["stats"])
    assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
    po, p1 = hc.noise_options(ol, min_steps=1), hc.plants(pkg, b)
    for es in (0, 1):
        so = hc.solve_options(ol, error_state=es)
        old = hc.reference_loop(ol, b, so, 7, 3, 1, po, p1, hc.SAT, IDS, step0=2)
        new = gc.held_loop(ol, b, so, 7, 3, 1, po, Rtab, 0.0, p1, hc.SAT, IDS, step0=2)
        d = max(float(np.max(np.abs(old[k] - new[k]))) for k in ("X_hist", "U_hist", "X", "U"))
        print(f"held reference at gm = 0, error_state {es}: max|d| {d:.1e}")
        assert d == 0.0
        for k in ("stats", "tracking_stats", "n_sure", "n_maybe", "tally", "statuses"):
            assert np.array_equal(old[k], new[k]), k


def test_emulated_ensemble_matches_reference(pkg, ol, emu, ens_case):
    """T = 2 ragged (20, 13), M = 3, every pair, all five dispersions, noise on, limits +-0.6; stats_nominal with it"""
    b, Rtab, X, U, Qd, Qfd, Rd, x0s, K, o, plant = ens_case
    pairs = dc.all_pairs(b.T, 3)
    kw = dict(plant=plant, sat=hc.SAT, noise_id0=IDS)
    ref = gc.ensemble_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, Rtab, gc.GM, **kw)
    ref0 = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, **kw)
    last = lambda r: [r["X_sim"][i, n - 1] for i, n in enumerate(r["n_knots"])]
    gc.moved(last(ref), last(ref0), "ensemble")
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], o.min_steps, o.w_tol, o.angle_tol)
    print(f"margin on the reference {m:.2e}")
    assert m > dc.MARGIN
    got = emu.ensemble(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, Rtab, gc.GM, sat=hc.SAT, noise_id0=IDS)
    dc.compare(ref, got, pairs)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom_pairs = np.array([(t, -1) for t in range(b.T)])
    nom = gc.ensemble_pairs(ol, pkg._abi, b, X, U, K, x0s, o, nom_pairs, Rtab, gc.GM, sat=hc.SAT)
    nom0 = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, nom_pairs, sat=hc.SAT)
    gc.moved(last(nom), last(nom0), "noise-free model plant")     # the model's 3U inertia feels the torque too
    ec.same_stats(nom["stats"], got["nominal"])


def test_emulated_ensemble_at_gm0_is_bit_equal_to_the_dispersed_kernel(pkg, ol, emu, ens_case):
    b, Rtab, X, U, Qd, Qfd, Rd, x0s, K, o, plant = ens_case
    old = ec.EmuEnsemble(pkg._abi).run(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, sat=hc.SAT, noise_id0=IDS)
    new = emu.ensemble(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, Rtab, 0.0, sat=hc.SAT, noise_id0=IDS)
    for k in ("X_sim", "stats", "summary", "nominal", "n_clipped"):
        assert old[k].tobytes() == new[k].tobytes(), k
    on = emu.ensemble(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, Rtab, gc.GM, sat=hc.SAT, noise_id0=IDS)
    assert np.max(np.abs(on["X_sim"] - new["X_sim"])) >= gc.MOVED


@pytest.mark.parametrize("error_state", [0, 1])
def test_emulated_hold_matches_reference(pkg, ol, emu, error_state):
    """T = 2 ragged, R = 3 over 7 steps (blocks 3 + 3 + 1), both feedback values, to the project's MPC bars, last plan included"""
    b, Rtab = _pair(pkg)
    po, plant = hc.noise_options(ol, min_steps=1), hc.plants(pkg, b)
    so = hc.solve_options(ol, error_state=error_state)
    for fb in (1, 0):
        ref = gc.held_loop(ol, b, so, 7, 3, fb, po, Rtab, gc.GM, plant, hc.SAT, IDS)
        ref0 = hc.reference_loop(ol, b, so, 7, 3, fb, po, plant, hc.SAT, IDS)
        gc.moved(ref["X_hist"][:, -1], ref0["X_hist"][:, -1], f"hold, error_state {error_state} feedback {fb}")
        assert ref["n_solves"] == 3 and np.all(ref["statuses"] <= hc.TSAT_MAX_OUTER)
        got = emu.held(b, so, po, 7, 3, fb, Rtab, gc.GM, plant, hc.SAT, IDS)
        hc.same(ref, got, b, po, plan=True)


@pytest.mark.parametrize("error_state", [0, 1])
def test_emulated_hold_at_gm0_is_bit_equal_to_the_held_loop(pkg, ol, emu, error_state):
    b, Rtab = _pair(pkg)
    po, plant = hc.noise_options(ol, min_steps=1), hc.plants(pkg, b)
    so = hc.solve_options(ol, error_state=error_state)
    for fb in (0, 1):
        old = hc.EmuMpcHeld(pkg._abi).run(b, so, po, 7, 3, fb, plant, hc.SAT, IDS, step0=3)
        new = emu.held(b, so, po, 7, 3, fb, Rtab, 0.0, plant, hc.SAT, IDS, step0=3)
        for k in ("X_hist", "U_hist", "stats", "X", "U", "tracking_stats", "n_clipped"):
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)


def test_emulated_hold_at_r1_does_not_see_the_feedback_switch(pkg, ol, emu):
    """R = 1 is the every-step loop under gravity gradient: no gain product is evaluated, so both feedback values agree bit for
    bit — and the term is in it"""
    b, Rtab = _pair(pkg)
    po, plant = hc.noise_options(ol, min_steps=1), hc.plants(pkg, b)
    so = hc.solve_options(ol)
    a = emu.held(b, so, po, 5, 1, 0, Rtab, gc.GM, plant, hc.SAT, IDS)
    c = emu.held(b, so, po, 5, 1, 1, Rtab, gc.GM, plant, hc.SAT, IDS)
    for k in ("X_hist", "U_hist", "stats", "X", "U", "tracking_stats", "n_clipped"):
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    off = emu.held(b, so, po, 5, 1, 1, Rtab, 0.0, plant, hc.SAT, IDS)
    assert np.max(np.abs(off["X_hist"] - a["X_hist"])) >= gc.MOVED


def test_rejected_arguments(pkg, ol, emu):
    """check_gravity, which both entry points call after their parents' checks"""
    good = gc.orbit(pkg, 12, 0.2)
    assert emu.check(good, gc.GM) == (0, "") and emu.check(good, 0.0) == (0, "")

    def edit(i, j, v):
        r = good.copy()
        r[i, j] = v
        return r

    zero = good.copy(); zero[7] = 0.0
    for R, gm, word in ((None, gc.GM, "null Rtab"), (edit(3, 1, np.nan), gc.GM, "non-finite Rtab entry in row 3"),
                        (edit(11, 0, -np.inf), gc.GM, "non-finite Rtab entry in row 11"), (zero, gc.GM, "row 7 has |r| = 0"),
                        (good, -1.0, "gm must be finite and >= 0"), (good, np.nan, "gm must"), (good, np.inf, "gm must")):
        rc, text = emu.check(R, gm)
        assert rc == -1 and word in text, (word, text)
    # the emulated ensemble refuses a null plant, half a limit and — unlike the sensed calls — a null table whatever gm is
    call = sc.smallest_tv_call(pkg, ec.tv_options(ol))
    fn = emu.lib.emu_tvlqr_ensemble_gg
    assert fn(*call.parent_args(True)) == 0 and fn(*call.edit(sat_lo=None, sat_hi=None).parent_args(True)) == 0
    for label, bad in (("plant NULL", call.edit(plant=None)), ("sat_hi NULL", call.edit(sat_hi=None)), ("sat_lo NULL", call.edit(sat_lo=None)),
                       ("Rtab NULL", call.edit(Rtab=None)), ("Rtab NULL, gm 0", call.edit(Rtab=None, gm=0.0)), ("gm negative", call.edit(gm=-1.0))):
        assert fn(*bad.parent_args(True)) == -1, label
    # without a handle the entry points themselves are codes, not crashes
    lib = pkg._abi.load()
    assert lib.tsat_mpc_run_held_gg(None, None, None, 1, 0, 1, 1, None, None, None, None, None, None, None, None, None, None, None, 0.0) == -1
    assert lib.tsat_tvlqr_ensemble_gg(*([None, None, 1, 1, 1] + [None] * 25 + [0.0])) == -1


def test_host_layers_name_the_entry_points(pkg):
    import os
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    for name in ("tsat_tvlqr_ensemble_gg", "tsat_mpc_run_held_gg"):
        assert name in hdr and name in pkg._abi.PROTOTYPES and (":" + name) in jl
    assert callable(pkg.tracking.attitude_ensemble_gg) and callable(pkg.mpc.receding_horizon_held_gg)
    pos = np.arange(2 * 9 * 3, dtype=np.float64).reshape(2, 9, 3)
    rows = pkg.magnetic.orbit_rows(pos, 4)
    assert rows.shape == (2, 4, 3) and rows.flags["C_CONTIGUOUS"] and np.array_equal(rows, pos[:, :4])
    with pytest.raises(ValueError):
        pkg.magnetic.orbit_rows(pos, 10)
