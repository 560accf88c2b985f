"""Dispersed-plant ensemble tracking (tsat_tvlqr_ensemble_dispersed), CPU tier: the kernel source of
tortoisesat.jl_amd/csrc/tsat_dispersed.hpp under the lane emulator against the reference closed loop of tests/dispersed_common.py
(the unchanged oracle's primitives, knot by knot), which is first pinned to the oracle's own tracking run.

Bars: |dX_sim| < 1e-9, `same_stats` (identical slew index and failure flag where the reference is more than 1e-7 away from a
threshold), the clipped-knot counter inside the reference's bracket (the plan rides its box, so the clip decision on such knots
is a matter of the last bit), `summary` against NumPy to 1e-12."""
import os

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import sensed_common as sc


@pytest.fixture(scope="module")
def emu_disp(pkg):
    return ec.EmuEnsemble(pkg._abi)


@pytest.fixture(scope="module")
def emu_ens(pkg):
    return ec.EmuEnsemble(pkg._abi)


def _with_gains(ol, case):
    b, r, Qd, Qfd, Rd, x0s = case
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]          # model inertia, once per slew
    return b, r["X"], r["U"], Qd, Qfd, Rd, x0s, K


@pytest.fixture(scope="module")
def mc_case(pkg, ol):
    return _with_gains(ol, ec.case_monte_carlo(pkg, ol))


@pytest.fixture(scope="module")
def ragged_case(pkg, ol):
    return _with_gains(ol, ec.case_ragged(pkg, ol))


def _box(b):
    return b.ulo, b.uhi


def test_emulated_driver_rejects_a_null_plant_and_half_a_limit(pkg, ol, emu_disp):
    """what tsat_tvlqr_ensemble_dispersed rejects of its own three arguments, through the emulator driver: -1 and nothing run"""
    good = sc.smallest_tv_call(pkg, ec.tv_options(ol))
    fn = emu_disp.lib.emu_tvlqr_ensemble_dispersed
    assert fn(*good.parent_args(False)) == 0 and fn(*good.edit(sat_lo=None, sat_hi=None).parent_args(False)) == 0
    for label, call in (("plant NULL", good.edit(plant=None)), ("sat_hi NULL", good.edit(sat_hi=None)), ("sat_lo NULL", good.edit(sat_lo=None))):
        assert fn(*call.parent_args(False)) == -1, label


def test_reference_is_pinned_to_the_oracle(pkg, ol, mc_case):
    """the hand-built loop with the MODEL plant and no limits is the oracle's tvlqr_batch run (noise_mode 1): 1e-12 on X_sim
    (a different operation order costs ~5e-15 over 1000 knots), same statistic"""
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    pairs = np.array([(0, 0), (1, 63), (2, 64), (3, 99)])
    o = ec.tv_options(ol)
    orc = ec.oracle_ensemble(ol, b, X, U, Qd, Qfd, Rd, x0s, pairs=pairs)
    assert np.array_equal(orc["K"], K[pairs[:, 0]])
    ref = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs)
    d = float(np.max(np.abs(ref["X_sim"] - orc["X_sim"])))
    print(f"reference loop against ol.tvlqr_batch: max|dX_sim| {d:.2e}")
    assert d < 1e-12
    ec.same_stats(orc["stats"], ref["stats"])
    assert np.array_equal(orc["stats"]["slew_time"], ref["stats"]["slew_time"])
    assert np.all(ref["n_sure"] == 0) and np.all(ref["n_maybe"] == 0)


def test_emulated_dispersed_matches_reference_small(pkg, ol, emu_disp, ragged_case):
    """T = 3 ragged, M = 70 (two wavefronts per slew), every realisation: all five dispersions, the plan's box as limits"""
    b, X, U, Qd, Qfd, Rd, x0s, K = ragged_case
    M = x0s.shape[1]
    plant = dc.all_five_plants(pkg, b, M)
    o = ec.tv_options(ol)
    got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, sat=_box(b), noise_id0=ec.RAGGED_ID0)
    pairs = dc.all_pairs(b.T, M)
    ref = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, plant=plant, sat=_box(b), noise_id0=ec.RAGGED_ID0)
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"])
    print(f"margin on the reference {m:.2e}")
    assert m > dc.MARGIN
    dc.compare(ref, got, pairs)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    # stats_nominal: the noise-free MODEL plant from the plan's first state, limits applied
    nom = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, np.array([(t, -1) for t in range(b.T)]), sat=_box(b))
    ec.same_stats(nom["stats"], got["nominal"])


def test_emulated_dispersed_matches_reference_sampled(pkg, ol, emu_disp, mc_case):
    """case_monte_carlo (4 x 1000 knots, M = 100): 34 seeded (t, m) drawn, the first 32 that meet the margin compared — the
    reference alone has to stay within the cap of 2 replacements, so that a GPU run cannot hide behind it"""
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    M = x0s.shape[1]
    plant = dc.all_five_plants(pkg, b, M)
    o = ec.tv_options(ol)
    got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, sat=_box(b))
    pairs = dc.sampled_pairs(b.T, M)
    ref = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, plant=plant, sat=_box(b))
    keep = dc.kept(ref)
    dc.compare(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    nom = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, np.array([(t, -1) for t in range(b.T)]), sat=_box(b))
    ec.same_stats(nom["stats"], got["nominal"])


def test_nominal_plants_reproduce_the_ensemble(pkg, ol, emu_disp, emu_ens, mc_case, ragged_case):
    """disperse_plant(all zeros) and no limits against the emulated tsat_tvlqr_ensemble (bit equality is not required: an
    isotropic model takes another instantiation of the dynamics in the nominal kernel)"""
    for case, id0 in ((mc_case, None), (ragged_case, ec.RAGGED_ID0)):
        b, X, U, Qd, Qfd, Rd, x0s, K = case
        M = x0s.shape[1]
        plant = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(1))
        o = ec.tv_options(ol)
        ens = emu_ens.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, noise_id0=id0)
        got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, noise_id0=id0)
        d = float(np.max(np.abs(ens["X_sim"] - got["X_sim"])))
        print(f"dispersed kernel with the model's plants against the ensemble kernel: max|dX_sim| {d:.2e}")
        assert d < 1e-9
        ec.same_stats(ens["stats"], got["stats"])
        ec.same_stats(ens["nominal"], got["nominal"])
        assert np.all(got["n_clipped"] == 0)


def test_each_dispersion_moves_the_result(pkg, ol, emu_disp, emu_ens, mc_case):
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    M = 8
    x0 = np.ascontiguousarray(x0s[:, :M])
    id0 = np.arange(b.T, dtype=np.int64) * x0s.shape[1]
    o = ec.tv_options(ol)
    ens = emu_ens.run(b, X, U, Qd, Qfd, Rd, x0, K, o, noise_id0=id0)
    # (turning the principal axes of an isotropic model alone changes nothing; it acts once the moments differ)
    runs = {}
    for kw in (dict(inertia_rel=0.01), dict(inertia_rel=0.01, axes_deg=0.2), dict(gain_rel=0.01), dict(misalign_deg=0.5),
               dict(residual_dipole=2e-4)):
        plant = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **kw)
        got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0, K, o, plant, noise_id0=id0)
        d = float(np.max(np.abs(ens["X_sim"] - got["X_sim"])))
        print(f"{kw}: max|dX_sim| against the nominal ensemble {d:.2e}")
        assert d > 1e-6, kw
        runs[tuple(kw)] = got["X_sim"]
    assert np.max(np.abs(runs[("inertia_rel",)] - runs[("inertia_rel", "axes_deg")])) > 1e-6
    # the limits alone: the plan rides its box, so the feedback command is clipped on many knots
    plant = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7))
    got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0, K, o, plant, sat=_box(b), noise_id0=id0)
    print(f"limits alone: clipped knots per loop {got['n_clipped'].min()} .. {got['n_clipped'].max()}")
    # per slew, not per loop: a realisation whose feedback happens to pull every command inwards is legitimate (one of
    # these 32 clips nothing), a slew none of whose realisations touches the box it was planned on would not be
    assert np.all(got["n_clipped"].max(axis=1) > 0)
    assert np.all(np.isfinite(got["X_sim"]))
    assert np.max(np.abs(got["X_sim"] - ens["X_sim"])) > 0.0


def test_disperse_plant_properties(pkg):
    dp = pkg.tracking.disperse_plant
    J = np.array([np.diag([0.01, 0.02, 0.03]).T.reshape(9), (np.diag([0.05, 0.04, 0.045]) + 1e-3 * (np.ones((3, 3)) - np.eye(3))).T.reshape(9)])
    z = dp(J, 5, np.random.default_rng(3))
    assert z.shape == (2, 5, 21)
    assert np.all(z[:, :, :9] == J[:, None, :]) and np.all(z[:, :, 9:18] == np.eye(3).reshape(9)) and np.all(z[:, :, 18:] == 0)
    p = dp(J, 200, np.random.default_rng(3), inertia_rel=0.3, axes_deg=5.0, gain_rel=0.05, misalign_deg=1.0, residual_dipole=1e-3)
    Jp = p[:, :, :9].reshape(2, 200, 3, 3)
    assert np.array_equal(Jp, Jp.transpose(0, 1, 3, 2))                               # symmetric exactly
    assert np.all(np.linalg.eigvalsh(Jp) > 0)                                          # positive definite at 0.3
    lam = np.linalg.eigvalsh(Jp)
    lam0 = np.linalg.eigvalsh(J.reshape(2, 3, 3))
    assert np.all(lam.min(axis=-1) >= 0.1 * lam0.min(axis=-1)[:, None] * (1 - 1e-9))  # (1 - 0.3 * 3) of the smallest moment
    assert np.all(np.isfinite(p)) and np.std(p[:, :, 18:]) > 0
    G = p[:, :, 9:18].reshape(2, 200, 3, 3).transpose(0, 1, 3, 2)
    assert np.max(np.abs(np.linalg.norm(G, axis=2) - 1.0)) < 0.16                      # columns: unit axes times (1 +- 0.15)
    small = dp(J, 7, np.random.default_rng(3), inertia_rel=0.3, axes_deg=5.0, gain_rel=0.05, misalign_deg=1.0, residual_dipole=1e-3)
    assert np.array_equal(small, p[:, :7])                                             # a prefix of the larger ensemble
    assert np.array_equal(dp(J.reshape(2, 3, 3).transpose(0, 2, 1), 7, np.random.default_rng(3), inertia_rel=0.3), dp(J, 7, np.random.default_rng(3), inertia_rel=0.3))
    for bad in (0.34, 1.0 / 3.0, -0.1):
        with pytest.raises(ValueError):
            dp(J, 2, np.random.default_rng(3), inertia_rel=bad)


def test_dispersions_decide_arrival(pkg, ol, emu_disp, emu_ens, mc_case):
    """1 % inertia / 0.2 deg axes at the reference's noise level: the nominal ensemble never fails, the dispersed one does"""
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    M = x0s.shape[1]
    o = ec.tv_options(ol)
    plant = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), inertia_rel=0.01, axes_deg=0.2)
    got = emu_disp.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, plant, want_trajectories=False)
    ens = emu_ens.run(b, X, U, Qd, Qfd, Rd, x0s, K, o, want_trajectories=False)
    fails = got["stats"]["failed"].sum(axis=1)
    print(f"failures per slew of {M}: dispersed {fails}, nominal {ens['stats']['failed'].sum(axis=1)}")
    assert ens["stats"]["failed"].sum() == 0
    assert 0 < fails.sum() < b.T * M


def test_host_layers_name_the_entry_point(pkg):
    root = ec.ROOT
    hdr = open(os.path.join(root, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(root, "julia", "TortoiseHIP.jl")).read()
    name = "tsat_tvlqr_ensemble_dispersed"
    assert name in hdr and name in pkg._abi.PROTOTYPES and (":" + name) in jl and "TSAT_PLANT_W 21" in hdr
    assert callable(pkg.tracking.attitude_ensemble_dispersed) and pkg.tracking.PLANT_W == 21
