"""CPU tier of the projection PD baseline (tsat_pd_ensemble): the reference of tests/pd_common.py pinned to
``gg_common.ensemble_loop`` at zero gains, the kernel source of tortoisesat.jl_amd/csrc/tsat_pd.hpp under the lane emulator against it
(bars of dispersed_common.compare), the four bit-equalities of the entry point, the zero field row, what the entry point rejects
(the library's own validation function, check_pd) and ``tracking.pd_gains``.

The case: slews 0 and 1 of the GPU tier's case (horizons 20 and 13, table 0 and table 1, 16 rows under a clock that clamps onto row
15), M = 3, every pair, all five dispersions, noise on, limits +-0.6, gains pd_common.KD / KP. The plan comes from ``ol.solve_batch``
(1 x 3 budget). Regulating from its start, slew 0 has e0 < 0 and clips at every knot and slew 1 has e0 < 0 and never clips."""
import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc

IDS = np.array([7, 2 ** 33 + 1], dtype=np.int64)
M = 3
KINDS = ("track", "track_ff", "regulate")


@pytest.fixture(scope="module")
def emu(pkg):
    return pc.EmuPd(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the pair, its plan from the oracle, M = 3 realisations; computed once and left unchanged"""
    b8, Rtab = pc.case(pkg)
    b = b8.slice(0, 2)
    r = ol.solve_batch(b, hc.solve_options(ol))
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, M),
                x0n=np.ascontiguousarray(b.x0))


def _kw(cs, kind, mode, **over):
    """the keyword arguments that both the reference and the emulator take"""
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"], gm=gc.GM,
              plant=cs["plant"], sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], noise_id0=IDS)
    kw.update(over)
    return kw


def _ref(pkg, ol, cs, pairs, kw, kd=pc.KD, kp=pc.KP, **extra):
    return pc.reference_pairs(ol, pkg._abi, cs["b"], cs["x0s"], kd, kp, cs["o"], pairs, **kw, **extra)


def test_reference_with_zero_gains_is_the_gg_reference(pkg, ol, cs):
    """the pin: kd = kp = 0, feed-forward on, limit_mode 0 is gg_common.ensemble_loop with an all-zero K, max |d| = 0"""
    b = cs["b"]
    pairs = np.concatenate([dc.all_pairs(b.T, M), [(0, -1), (1, -1)]])
    K0 = np.zeros((b.T, b.N - 1, 6, 3))
    old = gc.ensemble_pairs(ol, pkg._abi, b, cs["X"], cs["U"], K0, cs["x0s"], cs["o"], pairs, cs["Rtab"], gc.GM, plant=cs["plant"],
                            sat=hc.SAT, noise_id0=IDS)
    kw = _kw(cs, "track_ff", 0, x0_nom=None)
    new = _ref(pkg, ol, cs, pairs, kw, kd=np.zeros(3), kp=np.zeros(3))
    d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
    print(f"reference at zero gains against gg_common.ensemble_loop with K = 0: max|d| {d:.1e}")
    assert d == 0.0 and np.array_equal(old["stats"], new["stats"])
    assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
    assert old["n_sure"].max() > 0, "the pin must cover clipped knots"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_kernel_matches_reference(pkg, ol, emu, cs, kind, mode):
    """every pair of T = 2 x M = 3 and stats_nominal, for {tracking, tracking + feed-forward, regulation} x {clip, direction-preserving}"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw = _kw(cs, kind, mode)
    ref = _ref(pkg, ol, cs, pairs, kw)
    # the conditions, on references alone
    pc.differs(ref, _ref(pkg, ol, cs, pairs, kw, kd=np.zeros(3), kp=np.zeros(3)), "law on against law off")
    pc.differs(ref, _ref(pkg, ol, cs, pairs, dict(kw, gm=0.0)), "gm on against gm = 0")
    pc.differs(ref, _ref(pkg, ol, cs, pairs, dict(kw, Rtab=cs["Rtab"][::-1])), "orbit tables swapped")
    if kind == "regulate":
        pc.differs(ref, _ref(pkg, ol, cs, pairs, kw, sign_rule=False), "sign rule on against s = +1")
    if kind == "track_ff":
        pc.differs(ref, _ref(pkg, ol, cs, pairs, dict(kw, U=None)), "feed-forward on against off")
    pc.limit_condition(ref, lambda: _ref(pkg, ol, cs, pairs, dict(kw, limit_mode=0)), kind, mode)
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], cs["o"].min_steps, cs["o"].w_tol, cs["o"].angle_tol)
    print(f"margin on the reference {m:.2e}; clipped knots sure {ref['n_sure'].tolist()} maybe {ref['n_maybe'].tolist()}")
    assert m > dc.MARGIN
    got = emu.run(b, cs["o"], cs["x0s"], pc.KD, pc.KP, **kw)
    dc.compare(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom = _ref(pkg, ol, cs, np.array([(t, -1) for t in range(b.T)]), kw)
    ec.same_stats(nom["stats"], got["nominal"])


def _same_bytes(a, c):
    for k in ("X_sim", "stats", "summary", "nominal", "n_clipped"):
        assert a[k].tobytes() == c[k].tobytes(), k


def test_emulated_bit_equalities(pkg, ol, emu, cs):
    b, o, x0s = cs["b"], cs["o"], cs["x0s"]
    run = lambda kw: emu.run(b, o, x0s, pc.KD, pc.KP, **kw)
    # Rtab given with gm = 0 against Rtab = NULL: the kernel with the gravity rows against the one without
    kw = _kw(cs, "track_ff", 0, gm=0.0)
    _same_bytes(run(kw), run(dict(kw, Rtab=None)))
    on = run(dict(kw, gm=gc.GM))
    assert np.max(np.abs(on["X_sim"] - run(kw)["X_sim"])) >= gc.MOVED
    # plant = NULL against plants filled with (Jmat, I, 0)
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    assert np.array_equal(model[0, 0, 9:18], np.eye(3).ravel()) and not model[..., 18:].any()
    for kind in KINDS:
        kw = _kw(cs, kind, 1)
        _same_bytes(run(dict(kw, plant=None)), run(dict(kw, plant=model)))
    assert np.max(np.abs(run(dict(kw, plant=None))["X_sim"] - run(kw)["X_sim"])) >= gc.MOVED
    # X = xf tiled against X = NULL, the same explicit x0_nom
    tiled = np.ascontiguousarray(np.broadcast_to(b.xf[:, None, :], (b.T, b.N, 7)))
    for mode in (0, 1):
        kw = _kw(cs, "regulate", mode)
        _same_bytes(run(kw), run(dict(kw, X=tiled)))
    # mode 1 against mode 0 under limits nothing reaches
    for kind in KINDS:
        kw = _kw(cs, kind, 0, sat=pc.WIDE)
        a = run(kw)
        assert not a["n_clipped"].any()
        _same_bytes(a, run(dict(kw, limit_mode=1)))


def test_zero_field_row(pkg, ol, emu, cs):
    """Btab[:, 15, :] = 0, the last row of a magnetic_simulation table: the clock of the case clamps the last knots of the 20-knot
    horizon onto it. There the law gives no dipole (the command is the feed-forward alone), nothing is non-finite, and the kernel
    still matches the reference"""
    import dataclasses
    B = cs["b"].Btab.copy()
    B[:, 15, :] = 0.0
    b = dataclasses.replace(cs["b"], Btab=np.ascontiguousarray(B))
    pairs = dc.all_pairs(b.T, M)
    for kind, mode in (("track_ff", 0), ("regulate", 1)):
        kw = _kw(cs, kind, mode)
        ref = pc.reference_pairs(ol, pkg._abi, b, cs["x0s"], pc.KD, pc.KP, cs["o"], pairs, **kw)
        on_zero = [k for k in range(b.N - 1) if dc._row(b, 0, k, 0.0) is not None and not dc._row(b, 0, k, 0.0).any()]
        assert len(on_zero) >= 2, "the last two knots of the 20-knot horizon must sit on the zero row"
        for i, p in enumerate(pairs):
            if p[0] == 0:
                want = cs["U"][0, on_zero] if kind == "track_ff" else np.zeros((len(on_zero), 3))
                assert np.array_equal(ref["U_cmd"][i, on_zero], want)
        got = emu.run(b, cs["o"], cs["x0s"], pc.KD, pc.KP, **kw)
        assert np.all(np.isfinite(got["X_sim"])) and np.all(np.isfinite(got["summary"]))
        for f in ("slew_time", "final_w_norm", "final_angle"):
            assert np.all(np.isfinite(got["stats"][f])) and np.all(np.isfinite(got["nominal"][f]))
        dc.compare(ref, got, pairs)


def test_rejected_arguments(pkg, emu, cs):
    """check_pd, the one validation function of the entry point, through the emulator driver"""
    b = cs["b"]
    good = pc.Call(pkg._abi, b, cs["o"], cs["x0s"], pc.KD, pc.KP, **_kw(cs, "track_ff", 0))
    assert emu.check(good) == (0, "")
    # what the parent rejects and this entry point allows
    for ok in (good.edit(plant=None), good.edit(Rtab=None, gm=0.0), good.edit(X=None, U=None, feedforward=0),
               good.edit(U=None, feedforward=0), good.edit(limit_mode=1), good.edit(X=None, U=None, feedforward=0, x0_nom=None, stats_nominal=None)):
        assert emu.check(ok) == (0, "")
    for label, call, words in pc.rejections(good, b, cs["Rtab"]):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
    # the driver itself refuses what the function refuses, and the entry point without a handle is a code, not a crash
    assert emu.lib.emu_pd_ensemble(*good.edit(limit_mode=3).c_args()) == -1
    lib = pkg._abi.load()
    assert lib.tsat_pd_ensemble(None, *good.c_args()) == -1
    assert b"null handle" in lib.tsat_ensemble_last_error()


def test_pd_gains_and_host_layers(pkg):
    J = np.stack([pkg.slew_setup.jmat_cm(pkg.slew_setup.INERTIA["3U"])] * 2).reshape(2, 9)
    wn, zeta = np.array([0.01, 0.03]), 0.7
    kd, kp = pkg.tracking.pd_gains(J, wn, zeta)
    Jd = J[:, [0, 4, 8]]
    assert kd.shape == kp.shape == (2, 3)
    np.testing.assert_allclose(kp, 2.0 * Jd * wn[:, None] ** 2, rtol=1e-15)
    np.testing.assert_allclose(kd, 2.0 * zeta * wn[:, None] * Jd, rtol=1e-15)
    np.testing.assert_array_equal(pkg.tracking.pd_gains(J.reshape(2, 3, 3), wn, zeta)[0], kd)
    import os
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    assert "tsat_pd_ensemble" in hdr and "tsat_pd_ensemble" in pkg._abi.PROTOTYPES and ":tsat_pd_ensemble" in jl
    assert callable(pkg.tracking.attitude_ensemble_pd)
    assert pkg._abi.load().tsat_version() == 300
