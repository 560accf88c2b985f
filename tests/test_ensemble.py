"""Ensemble tracking (tsat_tvlqr_ensemble), CPU tier: the kernel source of tortoisesat.jl_amd/csrc/tsat_ensemble.hpp under the
lane emulator against the unchanged oracle, realisation by realisation. Realisation (t, m) is the oracle's tvlqr_batch run of
slew t with x0_sim[t, m], noise_mode = 1 and generator id noise_id0[t] + m.

Index equality is only meaningful when no judged sample sits within the state error of a threshold: every parity test first
asserts on the ORACLE's trajectories that the nearest one is more than 1e-7 (relative) away — 100 x the 1e-9 bar on the states."""
import numpy as np
import pytest

import ensemble_common as ec

MARGIN = 1e-7


@pytest.fixture(scope="module")
def emu_ens(pkg):
    return ec.EmuEnsemble(pkg._abi)


@pytest.fixture(scope="module")
def mc_case(pkg, ol):
    return ec.case_monte_carlo(pkg, ol)


@pytest.fixture(scope="module")
def ragged_case(pkg, ol):
    return ec.case_ragged(pkg, ol)


def _check(ref, got, batch, M):
    m = ec.margin(ref["X_sim"].reshape((-1,) + ref["X_sim"].shape[2:]), ref["batch"].xf, ec.horizons(batch, M))
    print(f"margin on the oracle {m:.2e}")
    assert m > MARGIN
    dX = float(np.max(np.abs(ref["X_sim"] - got["X_sim"])))
    print(f"max|dX_sim| {dX:.2e}; oracle failures per slew {ref['stats']['failed'].sum(axis=1)}")
    assert dX < 1e-9
    ec.same_stats(ref["stats"], got["stats"])
    assert np.array_equal(ref["stats"]["slew_time"], got["stats"]["slew_time"])
    return m


@pytest.mark.parametrize("sigma_scale", [1.0, 60.0])
def test_emulated_ensemble_matches_oracle(pkg, ol, emu_ens, mc_case, sigma_scale):
    """T = 4, N = 1000, M = 100 (two wavefronts per slew, the second with 36 live lanes + the nominal one), at the reference's
    noise level and at 60 x, where both outcomes of the statistic occur"""
    b, r, Qd, Qfd, Rd, x0s = mc_case
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, sigma_scale=sigma_scale)
    got = emu_ens.run(b, r["X"], r["U"], Qd, Qfd, Rd, x0s, ref["K"], ec.tv_options(ol, sigma_scale=sigma_scale))
    _check(ref, got, b, x0s.shape[1])
    fails = ref["stats"]["failed"].sum(axis=1)
    if sigma_scale == 1.0:
        assert fails.sum() == 0
    else:
        assert np.all(fails > 0) and np.all(fails < x0s.shape[1])        # both outcomes of the statistic are covered
    # the nominal realisation: the noise-free plant from the plan's own first state
    o = ol.tvlqr_default_options()
    nom = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0], opts=o)
    ec.same_stats(nom["stats"], got["nominal"])


def test_emulated_ensemble_ragged(pkg, ol, emu_ens, ragged_case):
    """per-slew horizons (60, 37, 12), M = 70, ids from (5, 900, 2^33): slabs beyond a horizon are zero, and every realisation
    fails (the horizons are too short) — slew_time = dt n_knots[t]"""
    b, r, Qd, Qfd, Rd, x0s = ragged_case
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, noise_id0=ec.RAGGED_ID0)
    got = emu_ens.run(b, r["X"], r["U"], Qd, Qfd, Rd, x0s, ref["K"], ec.tv_options(ol), noise_id0=ec.RAGGED_ID0)
    _check(ref, got, b, x0s.shape[1])
    assert np.all(ref["stats"]["failed"] == 1)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
        assert np.all(got["stats"]["slew_time"][t] == b.dt[t] * n)


def test_one_realisation_equals_the_tracking_kernel(pkg, ol, emu, emu_ens, ragged_case):
    """M = 1 is the existing emulated tracking kernel's run of the same realisation (its own gains handed over)"""
    b, r, Qd, Qfd, Rd, x0s = ragged_case
    x1 = np.ascontiguousarray(x0s[:, :1])
    o = ec.tv_options(ol)
    one = emu.tvlqr(b, r["X"], r["U"], Qd, Qfd, Rd, x1[:, 0], opts=pkg._abi.TvlqrOptions.from_buffer_copy(o), noise_ids=ec.RAGGED_ID0)
    got = emu_ens.run(b, r["X"], r["U"], Qd, Qfd, Rd, x1, one["K"], o, noise_id0=ec.RAGGED_ID0)
    assert np.max(np.abs(got["X_sim"][:, 0] - one["X_sim"])) < 1e-12
    for f in ("slew_index", "failed", "slew_time", "final_w_norm", "final_angle"):
        assert np.array_equal(got["stats"][f][:, 0], one["stats"][f]), f


def test_summary_definitions(pkg, ol, emu_ens, mc_case, ragged_case):
    """the eight entries of `summary` against NumPy: mixed outcomes (noise x 60) and every realisation failed"""
    b, r, Qd, Qfd, Rd, x0s = mc_case
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, sigma_scale=60.0)
    got = emu_ens.run(b, r["X"], r["U"], Qd, Qfd, Rd, x0s, ref["K"], ec.tv_options(ol, sigma_scale=60.0), want_trajectories=False)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    assert np.all(got["summary"][:, 1] > 0) and np.all(got["summary"][:, 3] <= got["summary"][:, 2])
    b, r, Qd, Qfd, Rd, x0s = ragged_case
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, noise_id0=ec.RAGGED_ID0)
    got = emu_ens.run(b, r["X"], r["U"], Qd, Qfd, Rd, x0s, ref["K"], ec.tv_options(ol), noise_id0=ec.RAGGED_ID0, want_trajectories=False)
    s = got["summary"]
    np.testing.assert_allclose(s, ec.summary_numpy(got["stats"]), rtol=1e-12)
    assert np.all(s[:, 0] == x0s.shape[1]) and np.all(s[:, 1] == x0s.shape[1]) and np.all(s[:, 2:5] == 0)
    np.testing.assert_allclose(s[:, 5], b.dt * b.n_knots, rtol=1e-12)
    # the function alone on statistics made up here: one arrival among failures
    st = np.zeros((1, 3), dtype=pkg._abi.TVLQR_STATS_DTYPE)
    st["failed"][0] = (1, 0, 1); st["slew_time"][0] = (200.0, 31.4, 200.0); st["final_angle"][0] = (0.5, 0.01, 0.7)
    np.testing.assert_allclose(emu_ens.summary(st), [[3, 2, 31.4, 31.4, 31.4, 431.4 / 3, 0.7, 0.0]], rtol=1e-12)


def test_host_layers_name_the_entry_points(pkg):
    """header, ctypes prototypes and the Julia shim all carry the two entry points (their agreement in arity and widths is
    what tests/test_abi.py and tests/test_julia_shim.py check)"""
    import os
    root = ec.ROOT
    hdr = open(os.path.join(root, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(root, "julia", "TortoiseHIP.jl")).read()
    for name in ("tsat_tvlqr_ensemble", "tsat_ensemble_last_error"):
        assert name in hdr and name in pkg._abi.PROTOTYPES and (":" + name) in jl
    x = pkg.tracking.ensemble_initial_states(np.tile(np.r_[0.0, 0, 0, 1, 0, 0, 0], (2, 1)), 5, np.random.default_rng(1))
    assert x.shape == (2, 5, 7) and np.allclose(np.linalg.norm(x[..., 3:], axis=-1), 1.0) and np.all(x[..., :3] == 0)
    assert np.array_equal(pkg.tracking.ensemble_noise_ids(2, 3), [[0, 1, 2], [3, 4, 5]])
