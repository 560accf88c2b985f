"""CPU tier of the receding-horizon loop on a noisy, dispersed plant with limits (tsat_mpc_run_dispersed): the reference loop of
tests/mpc_dispersed_common.py pinned to the oracle's own loop, the device function under the lane emulator against that
reference, what the entry point rejects (the library's own validation function, no GPU needed), and the host-side layout
helper."""
import ctypes as C

import numpy as np
import pytest

import mpc_dispersed_common as mc


@pytest.fixture(scope="module")
def emu_md(pkg):
    return mc.EmuMpcDispersed(pkg._abi)


def test_reference_is_pinned_to_the_oracle_loop(pkg, ol):
    """the dispersed reference's own pin: model's plant, no noise, no limits = ol.mpc_batch over 6 steps — X_hist within 1e-12
    (measured: 0, bit-equal on this workload — the stage arithmetic is the oracle's own), identical iteration counts"""
    b = mc.mpc_batch(pkg)
    o = mc.solve_options(ol)
    ref = ol.mpc_batch(b, o, 6, plant_integrator=4)
    got = mc.reference_loop(ol, b, o, 6, mc.noise_options(ol, noise=False))
    dX = float(np.max(np.abs(ref["X_hist"] - got["X_hist"])))
    print(f"pin: max|dX_hist| against ol.mpc_batch {dX:.2e}")
    assert dX < 1e-12
    assert np.max(np.abs(ref["U_hist"] - got["U_hist"])) < 1e-12
    for k in ("inner_iters", "ls_trials", "status", "outer_iters", "n_backward"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
    assert np.max(np.abs(ref["X"] - got["X"])) < 1e-12 and np.max(np.abs(ref["U"] - got["U"])) < 1e-12
    # ragged horizons: the shift stays inside the trajectory's own horizon
    b.n_knots = np.array([20, 13], dtype=np.int32)
    ref = ol.mpc_batch(b, o, 6, plant_integrator=4)
    got = mc.reference_loop(ol, b, o, 6, mc.noise_options(ol, noise=False))
    assert np.max(np.abs(ref["X_hist"] - got["X_hist"])) < 1e-12
    assert np.array_equal(ref["stats"]["inner_iters"], got["stats"]["inner_iters"])


def test_emulated_loop_matches_reference(pkg, ol, emu_md):
    """T = 2, N = 20, 4 steps, ragged (20, 13): all five dispersions, noise on, limits +-0.6, generator ids given"""
    b = mc.mpc_batch(pkg)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    o = mc.solve_options(ol)
    po = mc.noise_options(ol, min_steps=1)
    plant = mc.plants(pkg, b)
    ids = np.array([7, 2 ** 33 + 1], dtype=np.int64)
    ref = mc.reference_loop(ol, b, o, 4, po, plant, mc.SAT, ids)
    got = emu_md.run(b, o, po, 4, plant, mc.SAT, ids)
    mc.same(ref, got, b, po, plan=True)
    assert ref["n_maybe"].sum() > 0, "the limits never bite: the clip is not exercised"
    # the dispersion and the noise are really in the loop: the nominal plant's history differs
    nom = emu_md.run(b, o, mc.noise_options(ol, noise=False), 4)
    assert np.max(np.abs(nom["X_hist"] - got["X_hist"])) > 1e-7


def test_emulated_nominal_limit_matches_the_advance_kernel(pkg, ol, emu, emu_md):
    """plant = NULL, no noise, no limits: the loop of the existing advance kernel (its rk4 plant), to the MPC bars"""
    b = mc.mpc_batch(pkg)
    o = mc.solve_options(ol)
    old = emu.mpc(b, o, 4, plant_integrator=4)
    new = emu_md.run(b, o, mc.noise_options(ol, noise=False), 4)
    print(f"max|dX_hist| new loop against the advance kernel {np.max(np.abs(old['X_hist'] - new['X_hist'])):.2e}")
    assert np.max(np.abs(old["X_hist"] - new["X_hist"])) < 1e-9 and np.max(np.abs(old["U_hist"] - new["U_hist"])) < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(old["stats"][k], new["stats"][k]), k
    assert np.array_equal(new["n_clipped"], np.zeros(2, dtype=np.int32))


def test_emulated_continuation_and_statistic(pkg, ol, emu_md):
    """the statistic on a history long enough to judge: thresholds wide open except the rate, so that the first judged sample
    arrives; and step0 shifts the noise draws"""
    b = mc.mpc_batch(pkg)
    o = mc.solve_options(ol)
    po = mc.noise_options(ol, min_steps=2, w_tol=1e3, angle_tol=10.0)
    ref = mc.reference_loop(ol, b, o, 4, po, None, None, None, step0=5)
    got = emu_md.run(b, o, po, 4, step0=5)
    ok = mc.same(ref, got, b, po, clipped=False)
    assert ok.all() and np.array_equal(got["tracking_stats"]["slew_index"], [3, 3])
    assert np.array_equal(got["tracking_stats"]["slew_time"], b.dt * 3)
    other = emu_md.run(b, o, po, 4, step0=0)
    assert np.max(np.abs(other["X_hist"][:, 1] - got["X_hist"][:, 1])) > 0
    po.angle_tol = 1e-9                                   # nobody arrives: failed, slew_time = dt (n_steps + 1)
    got = emu_md.run(b, o, po, 4, step0=5)
    assert np.all(got["tracking_stats"]["failed"] == 1) and np.array_equal(got["tracking_stats"]["slew_time"], b.dt * 5)


def _check(emu_md, po, n_steps=4, step0=0, plant=None, lo=None, hi=None, T=2):
    text = C.create_string_buffer(256)
    d = emu_md.abi.as_dp
    rc = emu_md.lib.emu_mpc_dispersed_check(C.byref(po), C.c_int32(n_steps), C.c_int64(step0), d(plant), d(lo), d(hi), C.c_int64(T),
                                            text, C.c_int32(256))
    return rc, text.value.decode()


def test_rejected_arguments(pkg, ol, emu_md):
    """the library's own validation function (check_mpc_dispersed), which the entry point calls after tsat_mpc_run's checks"""
    b = mc.mpc_batch(pkg)
    plant = mc.plants(pkg, b)
    lo, hi = np.full((2, 3), -0.6), np.full((2, 3), 0.6)
    po = mc.noise_options(ol)
    assert _check(emu_md, po, plant=plant, lo=lo, hi=hi) == (0, "")
    assert _check(emu_md, po) == (0, "")
    for kw, word in ((dict(n_steps=0), "n_steps"), (dict(step0=-1), "step0"), (dict(step0=2 ** 31 - 2), "step0"),
                     (dict(lo=lo), "exactly one"), (dict(hi=hi), "exactly one"), (dict(lo=hi, hi=lo), "sat_lo > sat_hi")):
        rc, text = _check(emu_md, po, **kw)
        assert rc == -1 and word in text, (kw, text)
    bad = mc.noise_options(ol)
    bad.rate_as_written = 1
    assert "rate_as_written" in _check(emu_md, bad)[1]
    bad = mc.noise_options(ol)
    bad.noise_mode = 2
    assert "noise_mode" in _check(emu_md, bad)[1]
    # the plants: the dispersed ensemble's own checks and thresholds, with the offending trajectory
    p = plant.copy(); p[1, 20] = np.nan
    assert _check(emu_md, po, plant=p) == (-1, "non-finite plant entry at t = 1")
    p = plant.copy(); p[0, 1] += 1e-11 * np.abs(p[0, :9]).max()
    assert _check(emu_md, po, plant=p) == (-1, "Jp is not symmetric at t = 0")
    p = plant.copy(); p[0, 1] += 1e-13 * np.abs(p[0, :9]).max()
    assert _check(emu_md, po, plant=p)[0] == 0
    p = plant.copy(); p[1, 0:9] = -p[1, 0:9]
    assert _check(emu_md, po, plant=p) == (-1, "Jp is not positive definite at t = 1")
    # without a handle the entry point itself is a code, not a crash
    lib = pkg._abi.load()
    assert lib.tsat_mpc_run_dispersed(None, None, None, 1, 0, None, None, None, None, None, None, None, None, None, None) == -1


def test_tile_realisations_layout(pkg):
    """M realisations per slew as a T M batch: per-slew arrays repeated, tables shared, plants and ids of the ensemble's (t, m)"""
    b = mc.mpc_batch(pkg)
    b.n_knots = np.array([20, 13], dtype=np.int32)
    M = 3
    plant = mc.plants(pkg, b, M)
    tiled, kw = pkg.mpc.tile_realisations(b, M, plant=plant, noise_id0=np.array([10, 2 ** 33]), sat=mc.SAT)
    assert tiled.T == 6 and tiled.Btab is b.Btab and np.array_equal(tiled.btab_idx, np.repeat(b.btab_idx, M))
    assert np.array_equal(tiled.x0, np.repeat(b.x0, M, axis=0)) and np.array_equal(tiled.n_knots, [20, 20, 20, 13, 13, 13])
    assert np.array_equal(kw["plant"][4], plant[1, 1]) and kw["plant"].shape == (6, 21)
    assert np.array_equal(kw["noise_id"], [10, 11, 12, 2 ** 33, 2 ** 33 + 1, 2 ** 33 + 2])
    assert kw["sat"][0].shape == (6, 3) and np.all(kw["sat"][1] == 0.6)
    assert np.array_equal(pkg.mpc.tile_realisations(b, M)[1]["noise_id"], np.arange(6))
    with pytest.raises(ValueError):
        pkg.mpc.tile_realisations(b, M, plant=plant[:, :2])
