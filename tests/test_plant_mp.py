"""The closed-loop plant (dyn_sim_h, plant_noise and the loops of tvlqr_trajectory) against a 50-digit reference, CPU tier: the
oracle and the emulated kernel on every run of tests/golden/plant_mp.npz (cases, bars and the table the tests print:
tests/plant_mp_common.py), the file itself regenerated on its short cases, and zero noise levels — which gave NaN before
the `th == 0` rule of the attitude-noise rotation — at tsat_tvlqr_batch and at every emulated ensemble and loop."""
import numpy as np
import pytest

import plant_mp_common as pm

SHORT = 34       # the runs regenerated in-process: every slew of at most this many knots


def _short_runs():
    _, B, R = pm.fixture()
    return [n for n in pm.RUN_NAMES if int(np.max(B[str(R[n]["batch"])]["n_knots"])) <= SHORT]


@pytest.mark.parametrize("name", _short_runs())
def test_file_is_the_50_digit_reference(pkg, name):
    """tests/refmath_mp.py::tracking_reference on the file's inputs, rounded to float64: the file's outputs, bit for bit"""
    Btab, B, R = pm.fixture()
    _, b, r = pm.case(pkg, name)
    out, margin, gap = pm.script().compute_run(pkg.tracking, Btab, b, r)
    assert margin > pm.script().MARGIN and gap > pm.script().ROW_GAP
    for k, v in out.items():
        assert v.dtype == R[name][k].dtype and v.tobytes() == R[name][k].tobytes(), (name, k)


def test_cases_reach_what_they_are_there_for(pkg):
    """the horizons of the issue, in uniform and in ragged calls; the three modes, both linearisation steps; the generator's
    extreme words; arrivals, failures and the two readings of the rate"""
    _, B, R = pm.fixture()
    s = pm.script()
    want = {n + 1 for n in (1, 2, 15, 16, 17, 31, 32, 33, 51, 52, 53, 64, 65, 104, 105)}
    uniform, ragged, modes = set(), set(), set()
    for n in pm.RUN_NAMES:
        nk, o = B[str(R[n]["batch"])]["n_knots"], R[n]["opts"]
        (uniform if len(set(nk.tolist())) == 1 else ragged).update(nk.tolist())
        modes.add(("gen" if o[s.O_MODE] == 1 else "array" if ("noise" in R[n] or "noise_seed" in R[n]) else "free", int(o[s.O_LIN])))
        assert len(nk) <= 4
    assert ragged == want and {k for k in want if k <= SHORT} <= uniform
    assert modes == {(m, l) for m in ("free", "array", "gen") for l in (0, 1)}
    for n in ("u15_gen_lin1", "u16_gen_lin1", "u16_gen_lin0", "u17_gen_lin0"):       # the 16-knot boundary in generator mode
        assert n in pm.RUN_NAMES
    ids, w = s.extreme_ids(pkg.tracking)
    assert np.array_equal(ids, R["gx_extreme_words"]["ids"])
    print(f"extreme words of 2^16 ids: smallest first word {w[ids[0], 0]}, largest {w[ids[1], 0]}, second word {w[ids[2], 1]} "
          f"(multiple of 2^30 within {min(w[ids[2], 1] % 2 ** 30, 2 ** 30 - w[ids[2], 1] % 2 ** 30)})")
    assert w[ids[0], 0] < 2 ** 17 and w[ids[1], 0] > 2 ** 32 - 2 ** 17
    nz = R["s1_zero_att"]["noise"]
    assert np.all(nz[0] == 0) and np.all(nz[1][..., 3:6] == 0) and np.any(nz[1][..., :3] != 0)
    assert np.all(nz[2][..., 3:6] ** 2 == 0) and np.all(nz[2][..., 3:6] != 0)                      # squares underflow
    s.expectations(R)


@pytest.mark.parametrize("name", pm.RUN_NAMES)
def test_oracle_and_emulated_kernel_against_50_digits(pkg, ol, emu, name):
    ora = pm.run_oracle(ol, pkg, name)
    got = pm.run_emu(emu, pkg, name)
    bad = [who for who, r in (("oracle", ora), ("emulator", got)) if not pm.all_finite(r)]
    assert not bad, (name, "non-finite output", bad)
    pm.check_oracle(name, ora)
    pm.check_impl(name, got, [ora], "emulator")


@pytest.mark.parametrize("who", ["oracle", "emulator"])
def test_zero_noise_levels_tracking(pkg, ol, emu, who):
    """noise_mode = 1 with sigma_gyro = sigma_att = field_amp = 0 is the noise-free run; sigma_att = 0 alone ("gyro noise only")
    is array mode fed the same draws — on the oracle and on the emulated kernel"""
    if who == "oracle":
        pm.tvlqr_zero_sigma_checks(pkg, ol.tvlqr_default_options, lambda n, o, nz: pm.run_oracle(ol, pkg, n, o, nz), who)
    else:
        pm.tvlqr_zero_sigma_checks(pkg, pkg._abi.TvlqrOptions, lambda n, o, nz: pm.run_emu(emu, pkg, n, o, nz), who)


def test_zero_noise_levels_emulated_ensembles(pkg, ol):
    """the ensemble roll-outs (nominal and dispersed kernels) with every level zero: each realisation is the noise-free run of
    tsat_tvlqr_batch from its own initial state"""
    import ensemble_common as ec

    sb, b, r = pm.case(pkg, pm.ZERO_RUN)
    s = pm.script()
    M = 3
    x0 = np.ascontiguousarray(np.stack([b["x0_sim"], b["X"][:, 0], 0.5 * (b["x0_sim"] + b["X"][:, 0])], axis=1))      # (T, M, 7)
    v = np.array(r["opts"]); v[[s.O_SG, s.O_SA, s.O_FA]] = 0.0
    o = pm.fill_options(ol.tvlqr_default_options(), v)
    K = pm.fixture()[2][pm.ZERO_RUN]["K"]
    v0 = v.copy(); v0[s.O_MODE] = 0
    free = [ol.tvlqr_batch(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], x0[:, m], opts=pm.fill_options(ol.tvlqr_default_options(), v0)) for m in range(M)]
    free = dict(X_sim=np.stack([f["X_sim"] for f in free], axis=1), stats=np.stack([f["stats"] for f in free], axis=1))
    e = ec.EmuEnsemble(pkg._abi)
    pm.check_zero_sigmas(free, e.run(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], x0, K, o), b["n_knots"], "emulated ensemble")
    plant = pkg.tracking.disperse_plant(sb.Jmat, M, np.random.default_rng(7))           # all levels zero: the model's plant
    pm.check_zero_sigmas(free, e.run(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], x0, K, o, plant=plant), b["n_knots"], "emulated dispersed ensemble")


@pytest.mark.parametrize("entry", ["gg", "pd", "sensed", "filtered", "model_filtered"])
def test_zero_noise_levels_other_emulated_ensembles(pkg, entry):
    """the other emulated ensemble kernels on dispersed plants under gravity gradient, the sensors' own noise on: every plant level
    zero is finite and is the limit of a vanishing attitude level (plant_mp_common.TINY_ATT), which never met th == 0"""
    import filtered_common as fc
    import gg_common as gc
    import model_filtered_common as mf
    import pd_common as pc
    import sensed_common as sc

    c = pm.ensemble_case(pkg)
    sb, b, abi = c["sb"], c["b"], pkg._abi
    plan = (b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], c["x0"], c["K"])
    kw = dict(plant=c["plant"], Rtab=c["Rtab"], gm=gc.GM)
    out = []
    for sa in (0.0, pm.TINY_ATT):
        o = pm.level_options(abi.TvlqrOptions, c["r"], sa)
        if entry == "gg":
            out.append(gc.EmuGg(abi).ensemble(sb, *plan, o, c["plant"], c["Rtab"], gc.GM))
        elif entry == "pd":
            out.append(pc.EmuPd(abi).run(sb, o, c["x0"], 10 * pc.KD, 10 * pc.KP, X=b["X"], U=b["U"], **kw))
        else:
            emu = {"sensed": sc.EmuSensed, "filtered": fc.EmuFiltered, "model_filtered": mf.EmuModelFiltered}[entry](abi)
            out.append(emu.tv(sb, o, *plan, sens=sc.SIGMAS, **kw))
    pm.check_same_limit(out[0], out[1], b["n_knots"], f"emulated {entry}")


@pytest.mark.parametrize("loop", ["dispersed", "held", "held_sensed", "held_filtered"])
def test_zero_noise_levels_emulated_loops(pkg, ol, loop):
    """the emulated receding-horizon loops, two control steps of 17-knot solves: generated noise with every plant level zero is the
    noise-free loop; with the sensors' own noise on, the limit of a vanishing attitude level"""
    import mpc_dispersed_common as mc
    import mpc_filtered_common as mfc
    import mpc_held_common as hc
    import mpc_sensed_common as msc
    import sensed_common as sc

    b = mc.mpc_batch(pkg, T=2, N=17)
    opts = mc.solve_options(ol)
    level = lambda sa: mc.noise_options(ol, True, sigma_gyro=0.0, sigma_att=sa, field_amp=0.0)
    if loop == "dispersed":
        run = lambda po: mc.EmuMpcDispersed(pkg._abi).run(b, opts, po, 2)
    elif loop == "held":
        run = lambda po: hc.EmuMpcHeld(pkg._abi).run(b, opts, po, 2, 2, 1)
    elif loop == "held_sensed":
        run = lambda po: msc.EmuMpcSensed(pkg._abi).run(b, opts, po, 2, 2, 1, sens=sc.SIGMAS)
    else:
        run = lambda po: mfc.EmuMpcFiltered(pkg._abi).run(b, opts, po, 2, 2, 1, sens=sc.SIGMAS)
    z = run(level(0.0))
    base = run(level(pm.TINY_ATT)) if loop in ("held_sensed", "held_filtered") else run(mc.noise_options(ol, False))
    assert np.all(np.isfinite(z["X_hist"])) and np.all(np.isfinite(z["U_hist"])), (loop, "zero noise levels give a non-finite history")
    d, bar = float(np.max(np.abs(base["X_hist"] - z["X_hist"]))), pm.FLOOR_ULPS * pm.ULP * float(np.max(np.abs(z["X_hist"]))) * 2
    print(f"zero sigmas emulated {loop}: |dX_hist| {d:.2e}, bar {bar:.2e}")
    assert d <= bar, (loop, d, bar)
