"""CPU tier of the ensemble controllers fed measurements (tsat_tvlqr_ensemble_sensed, tsat_pd_ensemble_sensed): the references of
tests/sensed_common.py pinned to their parents at the ideal sensor, the draw layout of the two sensor stages, the kernel source of
tortoisesat.jl_amd/csrc/tsat_sensed.hpp under the lane emulator against the references (bars of dispersed_common.compare), the
bit-equalities of the entry points, what they reject (the library's own validation function, check_sensor) and
``tracking.disperse_sensor``.

The case: slews 0 and 1 of the GPU tier's case (horizons 20 and 13, table 0 and table 1), M = 3, every pair, all five plant
dispersions, plant noise on, gravity gradient on, TVLQR weights r = 0.5e-6, PD gains 10 x pd_common's, sensor levels
sensed_common.SIGMAS / BIAS. The plan comes from ``ol.solve_batch`` (1 x 3 budget)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

IDS = np.array([7, 2 ** 33 + 1], dtype=np.int64)
M = 3
KINDS = ("track", "track_ff", "regulate")


@pytest.fixture(scope="module")
def emu(pkg):
    return sc.EmuSensed(pkg._abi)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """the pair, its plan and gains from the oracle, M = 3 realisations; computed once and left unchanged"""
    b8, Rtab = pc.case(pkg)
    b = b8.slice(0, 2)
    r = ol.solve_batch(b, hc.solve_options(ol))
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]
    print(f"max|K| {np.abs(K).max():.2e}")
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=(Qd, Qfd, Rd), K=K, x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, M),
                x0n=np.ascontiguousarray(b.x0), sensor=sc.biases(pkg, b.T, M))


def _tv_kw(cs, sat=hc.SAT, **over):
    kw = dict(Rtab=cs["Rtab"], gm=gc.GM, plant=cs["plant"], sat=sat, noise_id0=IDS, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"])
    kw.update(over)
    return kw


def _pd_kw(cs, kind, mode, **over):
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"], gm=gc.GM,
              plant=cs["plant"], sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], noise_id0=IDS, sens=sc.SIGMAS, latency=0, sensor=cs["sensor"])
    kw.update(over)
    return kw


def _tv_ref(pkg, ol, cs, pairs, kw):
    return sc.pairs_of(ol, pkg._abi, "tv", cs["b"], cs["x0s"], cs["K"], cs["o"], pairs, X=cs["X"], U=cs["U"], **kw)


def _pd_ref(pkg, ol, cs, pairs, kw):
    return sc.pairs_of(ol, pkg._abi, "pd", cs["b"], cs["x0s"], (sc.KD, sc.KP), cs["o"], pairs, **kw)


def _tv_emu(emu, cs, kw):
    return emu.tv(cs["b"], cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], cs["K"], **kw)


def _pd_emu(emu, cs, kw):
    return emu.pd(cs["b"], cs["o"], cs["x0s"], sc.KD, sc.KP, **kw)


def test_references_with_the_ideal_sensor_are_their_parents(pkg, ol, cs):
    """the pin: no biases, zero sigmas, latency 0 — through ``measure`` — is gg_common.ensemble_loop / pd_common.reference_loop,
    max |d| = 0"""
    b = cs["b"]
    pairs = np.concatenate([dc.all_pairs(b.T, M), [(0, -1), (1, -1)]])
    old = gc.ensemble_pairs(ol, pkg._abi, b, cs["X"], cs["U"], cs["K"], cs["x0s"], cs["o"], pairs, cs["Rtab"], gc.GM, plant=cs["plant"],
                            sat=hc.SAT, noise_id0=IDS)
    new = _tv_ref(pkg, ol, cs, pairs, _tv_kw(cs, sens=sc.IDEAL, sensor=None))
    d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
    print(f"TVLQR reference with the ideal sensor against gg_common.ensemble_loop: max|d| {d:.1e}")
    assert d == 0.0 and np.array_equal(old["stats"], new["stats"])
    assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])
    assert old["n_sure"].max() > 0, "the pin must cover clipped knots"
    for kind in KINDS:
        for mode in (0, 1):
            kw = _pd_kw(cs, kind, mode, sens=sc.IDEAL, sensor=None)
            pkw = {k: v for k, v in kw.items() if k not in ("sens", "latency", "sensor")}
            old = pc.reference_pairs(ol, pkg._abi, b, cs["x0s"], sc.KD, sc.KP, cs["o"], pairs, **pkw)
            new = _pd_ref(pkg, ol, cs, pairs, kw)
            d = float(np.max(np.abs(old["X_sim"] - new["X_sim"])))
            print(f"PD reference ({kind}, mode {mode}) with the ideal sensor against pd_common.reference_loop: max|d| {d:.1e}")
            assert d == 0.0 and np.array_equal(old["stats"], new["stats"]) and np.array_equal(old["U_cmd"], new["U_cmd"])
            assert np.array_equal(old["n_sure"], new["n_sure"]) and np.array_equal(old["n_maybe"], new["n_maybe"])


def test_draw_layout_of_the_sensor_stages(pkg, ol):
    """stage 4 and 5 of ``ol.plant_noise`` are Philox counters (gid lo, gid hi, k, 16 / 17 / 20) under the key of the seed, through
    Box-Muller: the layout include/tortoise_hip.h documents, restated in numpy around ``tracking.philox4x32_10``"""
    seed = 0x1234_5678_9ABC_DEF1
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)

    def words(gid, k, c):
        return pkg.tracking.philox4x32_10(key, np.array([gid & 0xFFFFFFFF, gid >> 32, k, c], dtype=np.uint64)).astype(np.float64)

    def bm(a, c):
        ua, uc = (a + 0.5) / 4294967296.0, (c + 0.5) / 4294967296.0
        r, th = math.sqrt(-2.0 * math.log(ua)), 2.0 * math.pi * uc
        return r * math.cos(th), r * math.sin(th)

    sg, sa, sm = 3e-4, 5e-3, 5e-7
    for gid, k in ((7, 3), (2 ** 33 + 12345, 19999)):
        w0, w1, w5 = words(gid, k, 16), words(gid, k, 17), words(gid, k, 20)
        z = [*bm(w0[0], w0[1]), *bm(w0[2], w0[3]), *bm(w1[0], w1[1])]
        want = np.r_[sg * np.array(z[0:3]), sa * np.array(z[3:6])]
        got = ol.plant_noise(seed, gid, k, 4, sg, sa, 0.0)
        np.testing.assert_allclose(got[0:6], want, rtol=1e-13, atol=0)
        z5 = [*bm(w5[0], w5[1]), *bm(w5[2], w5[3])]
        got5 = ol.plant_noise(seed, gid, k, 5, sm, 0.0, 0.0)
        np.testing.assert_allclose(got5[0:3], sm * np.array(z5[0:3]), rtol=1e-13, atol=0)
        assert not got5[3:9].any() and not got[6:9].any()
        assert np.abs(got[0:6]).min() > 0 and not np.array_equal(got[0:3], ol.plant_noise(seed, gid, k, 3, sg, sa, 0.0)[0:3])


def _check_against(pkg, ol, cs, ref, got, pairs, nom_ref):
    b = cs["b"]
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], cs["o"].min_steps, cs["o"].w_tol, cs["o"].angle_tol)
    print(f"margin on the reference {m:.2e}; clipped knots sure {ref['n_sure'].tolist()} maybe {ref['n_maybe'].tolist()}")
    assert m > dc.MARGIN
    dc.compare(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    ec.same_stats(nom_ref["stats"], got["nominal"])


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("limits", ["0.6", "25"])
def test_emulated_tvlqr_matches_reference(pkg, ol, emu, cs, limits, latency):
    """every pair of T = 2 x M = 3 and stats_nominal, limits +-0.6 and +-25, latency 0 and 1"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    kw = _tv_kw(cs, sat=hc.SAT if limits == "0.6" else pc.WIDE, latency=latency)
    ref = sc.conditions(lambda **o: _tv_ref(pkg, ol, cs, pairs, dict(kw, **o)), "tv", cs["sensor"])
    off = sc.pairs_of(ol, pkg._abi, "tv", b, cs["x0s"], np.zeros_like(cs["K"]), cs["o"], pairs, X=cs["X"], U=cs["U"], **kw)
    pc.differs(ref, off, "gains on against off")
    got = _tv_emu(emu, cs, kw)
    nom = _tv_ref(pkg, ol, cs, np.array([(t, -1) for t in range(b.T)]), kw)
    _check_against(pkg, ol, cs, ref, got, pairs, nom)
    if limits == "0.6":
        assert ref["n_sure"].max() > 0, "no knot of the case clips"
    else:
        assert not got["n_clipped"].any()


@pytest.mark.parametrize("latency", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_pd_matches_reference(pkg, ol, emu, cs, kind, mode, latency):
    """{tracking, tracking + feed-forward, regulation} x {clip, direction-preserving} x latency {0, 1}. Regulation from the case's
    starts commands far beyond +-0.6: under the component clip every component sits on its limit at every knot and no sensor error
    reaches the plant (measured: 0.0), so regulation is compared under +-0.6 AND under +-25, and asserts its conditions there"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    nomp = np.array([(t, -1) for t in range(b.T)])
    kw = _pd_kw(cs, kind, mode, latency=latency)
    if kind == "regulate":
        ref = _pd_ref(pkg, ol, cs, pairs, kw)
        assert ref["n_sure"].max() > 0, "no knot of the case clips"
        _check_against(pkg, ol, cs, ref, _pd_emu(emu, cs, kw), pairs, _pd_ref(pkg, ol, cs, nomp, kw))
        kw = dict(kw, sat=pc.WIDE)
    ref = sc.conditions(lambda **o: _pd_ref(pkg, ol, cs, pairs, dict(kw, **o)), "pd", cs["sensor"])
    _check_against(pkg, ol, cs, ref, _pd_emu(emu, cs, kw), pairs, _pd_ref(pkg, ol, cs, nomp, kw))


def test_tiny_horizons_at_latency_1(pkg, ol, emu, cs):
    """n_knots = 2 (one command) and 3 (two commands, both from y_0) at latency 1"""
    import dataclasses
    b = dataclasses.replace(cs["b"], n_knots=np.array([2, 3], dtype=np.int32))
    c2 = dict(cs, b=b)
    pairs = dc.all_pairs(b.T, M)
    nomp = np.array([(t, -1) for t in range(b.T)])
    for law, kw in (("tv", _tv_kw(cs, latency=1)), ("pd", _pd_kw(cs, "track_ff", 0, latency=1)), ("pd", _pd_kw(cs, "regulate", 1, latency=1))):
        ref_of = _tv_ref if law == "tv" else _pd_ref
        ref = ref_of(pkg, ol, c2, pairs, kw)
        got = (_tv_emu if law == "tv" else _pd_emu)(emu, c2, kw)
        dc.compare(ref, got, pairs)
        ec.same_stats(ref_of(pkg, ol, c2, nomp, kw)["stats"], got["nominal"])
        for t, n in enumerate(b.n_knots):
            assert np.all(got["X_sim"][t, :, n:] == 0)
        # the command of knot 0 is y_0's whatever the latency; that of knot 1 of the 3-knot slew is y_0's only at latency 1
        r0 = ref_of(pkg, ol, c2, pairs, dict(kw, latency=0))
        assert np.array_equal(ref["U_cmd"][:, 0], r0["U_cmd"][:, 0])
        three = pairs[:, 0] == 1
        assert np.all(np.any(ref["U_cmd"][three, 1] != r0["U_cmd"][three, 1], axis=1))
        assert np.array_equal(ref["X_sim"][~three], r0["X_sim"][~three])


def _same(a, c, keys=("X_sim", "stats", "summary", "nominal", "n_clipped")):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_ideal_sensor_is_bit_equal_to_the_emulated_parents(pkg, ol, emu, cs):
    """zero (or NULL) sensor, zero sigmas, latency 0: x + 0 + 0 z, x (x) (1, 0, 0, 0) and b + 0 + 0 z are exact, so the sensed
    kernels repeat tsat_tvlqr_ensemble_gg, tsat_tvlqr_ensemble_dispersed (Rtab = NULL) and tsat_pd_ensemble (both ways) byte for
    byte; Rtab with gm = 0 is Rtab = NULL"""
    b, o, x0s, K = cs["b"], cs["o"], cs["x0s"], cs["K"]
    zero = np.zeros_like(cs["sensor"])
    ideal = dict(sens=sc.IDEAL, latency=0, sensor=zero)
    gg = gc.EmuGg(pkg._abi).ensemble(b, cs["X"], cs["U"], *cs["W"], x0s, K, o, cs["plant"], cs["Rtab"], gc.GM, sat=hc.SAT, noise_id0=IDS)
    new = _tv_emu(emu, cs, _tv_kw(cs, **ideal))
    _same(gg, new)
    _same(new, _tv_emu(emu, cs, _tv_kw(cs, **dict(ideal, sensor=None))))
    disp = ec.EmuEnsemble(pkg._abi).run(b, cs["X"], cs["U"], *cs["W"], x0s, K, o, cs["plant"], sat=hc.SAT, noise_id0=IDS)
    new0 = _tv_emu(emu, cs, _tv_kw(cs, Rtab=None, gm=0.0, **ideal))
    _same(disp, new0)
    _same(new0, _tv_emu(emu, cs, _tv_kw(cs, gm=0.0, **ideal)))                    # Rtab with gm = 0 against Rtab = NULL
    assert np.max(np.abs(new["X_sim"] - new0["X_sim"])) >= gc.MOVED
    # with the sensor on, too: Rtab / gm = 0 against NULL, sensor NULL against zeros
    on = _tv_kw(cs, gm=0.0, latency=1)
    _same(_tv_emu(emu, cs, on), _tv_emu(emu, cs, dict(on, Rtab=None)))
    _same(_tv_emu(emu, cs, dict(on, sensor=None)), _tv_emu(emu, cs, dict(on, sensor=zero)))
    assert np.max(np.abs(_tv_emu(emu, cs, on)["X_sim"] - new0["X_sim"])) >= gc.MOVED
    # plant = NULL flies the model's plant
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    _same(_tv_emu(emu, cs, dict(on, plant=None)), _tv_emu(emu, cs, dict(on, plant=model)))
    epd = pc.EmuPd(pkg._abi)
    for kind in KINDS:
        for mode in (0, 1):
            for rt in (cs["Rtab"], None):
                kw = _pd_kw(cs, kind, mode, Rtab=rt, gm=gc.GM if rt is not None else 0.0, **ideal)
                pkw = {k: v for k, v in kw.items() if k not in ("sens", "latency", "sensor")}
                old = epd.run(b, o, x0s, sc.KD, sc.KP, **pkw)
                _same(old, _pd_emu(emu, cs, kw))
                _same(old, _pd_emu(emu, cs, dict(kw, sensor=None)))
        on = _pd_kw(cs, kind, 0, gm=0.0, latency=1)
        _same(_pd_emu(emu, cs, on), _pd_emu(emu, cs, dict(on, Rtab=None)))
        _same(_pd_emu(emu, cs, dict(on, sensor=None)), _pd_emu(emu, cs, dict(on, sensor=zero)))


def test_rejected_arguments(pkg, emu, cs):
    """check_sensor, the validation function both entry points add to their parents', through the emulator driver; the drivers and
    the entry points refuse what it refuses"""
    b = cs["b"]
    good = sc.PdCall(pkg._abi, b, cs["o"], cs["x0s"], sc.KD, sc.KP, **_pd_kw(cs, "track_ff", 0))
    assert emu.check(good) == (0, "")
    assert emu.check(good.edit(sensor=None)) == (0, "")
    for label, call, words in sc.sensor_rejections(good):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
        assert emu.lib.emu_pd_ensemble_sensed(*call.c_args()) == -1, label
    # what the parent rejects is still rejected, and the sensed TVLQR call allows the NULL plant and the NULL Rtab with gm = 0
    assert emu.lib.emu_pd_ensemble_sensed(*good.edit(limit_mode=3).c_args()) == -1
    tv = sc.TvCall(pkg._abi, b, cs["o"], cs["X"], cs["U"], *cs["W"], cs["x0s"], K=cs["K"], **_tv_kw(cs))
    assert emu.lib.emu_tvlqr_ensemble_sensed(*tv.edit(Rtab=None).c_args(emu=True)) == -1          # gm != 0 needs the table
    assert emu.lib.emu_tvlqr_ensemble_sensed(*tv.edit(Rtab=None, gm=0.0, plant=None).c_args(emu=True)) == 0
    for label, call, words in sc.sensor_rejections(tv):
        assert emu.lib.emu_tvlqr_ensemble_sensed(*call.c_args(emu=True)) == -1, label
    # the entry points without a handle: a code, not a crash
    lib = pkg._abi.load()
    assert lib.tsat_pd_ensemble_sensed(None, *good.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()
    assert lib.tsat_tvlqr_ensemble_sensed(None, *tv.c_args()) == -1 and b"null handle" in lib.tsat_ensemble_last_error()


def test_disperse_sensor_and_host_layers(pkg):
    tr, abi = pkg.tracking, pkg._abi
    a = tr.disperse_sensor(3, 5, np.random.default_rng(4), gyro_bias=1e-3, att_bias_deg=0.5, mag_bias=2e-6)
    assert a.shape == (3, 5, 9) and a.dtype == np.float64 and np.all(np.isfinite(a)) and np.all(a != 0)
    assert np.array_equal(a, tr.disperse_sensor(3, 5, np.random.default_rng(4), gyro_bias=1e-3, att_bias_deg=0.5, mag_bias=2e-6))
    assert not np.array_equal(a, tr.disperse_sensor(3, 5, np.random.default_rng(5), gyro_bias=1e-3, att_bias_deg=0.5, mag_bias=2e-6))
    assert not tr.disperse_sensor(3, 5, np.random.default_rng(4)).any()
    big = tr.disperse_sensor(3, 8, np.random.default_rng(4), gyro_bias=1e-3, att_bias_deg=0.5, mag_bias=2e-6)
    assert np.array_equal(big[:, :5], a)                              # the first M' realisations of a larger ensemble
    z = np.random.default_rng(4).standard_normal((3, 9))
    np.testing.assert_allclose(a[:, 0], z * np.repeat([1e-3, np.deg2rad(0.5), 2e-6], 3), rtol=1e-15)
    with pytest.raises(ValueError):
        tr.disperse_sensor(1, 1, np.random.default_rng(0), gyro_bias=-1.0)
    # the struct, its defaults and the three symbols through every layer
    assert C.sizeof(abi.SensorOptions) == 32
    assert [(n, C.sizeof(t)) for n, t in abi.SensorOptions._fields_] == [("sigma_gyro", 8), ("sigma_att", 8), ("sigma_mag", 8),
                                                                          ("latency", 4), ("reserved", 4)]
    lib = abi.load()
    so = abi.SensorOptions(1.0, 2.0, 3.0, 1, 7)
    lib.tsat_sensor_default_options(C.byref(so))
    assert (so.sigma_gyro, so.sigma_att, so.sigma_mag, so.latency, so.reserved) == (0.0, 0.0, 0.0, 0, 0)
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    import re
    body = re.search(r"struct tsat_sensor_options \{(.*?)\};", hdr, flags=re.S).group(1)
    assert re.findall(r"(double|int32_t)\s+(\w+);", body) == [("double", "sigma_gyro"), ("double", "sigma_att"), ("double", "sigma_mag"),
                                                              ("int32_t", "latency"), ("int32_t", "reserved")]
    for name in ("tsat_sensor_default_options", "tsat_tvlqr_ensemble_sensed", "tsat_pd_ensemble_sensed"):
        assert name in hdr and name in abi.PROTOTYPES and ":" + name in jl and re.fullmatch(r"tsat_[a-z_]+", name)
    assert callable(tr.attitude_ensemble_sensed) and callable(tr.attitude_ensemble_pd_sensed)
    assert tr.SENSOR_SIGMA_GYRO == 0.38 * np.pi / 180.0 and tr.SENSOR_SIGMA_ATT == np.pi / 180.0
    assert lib.tsat_version() == 300
