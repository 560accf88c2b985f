"""CPU tier of the asymptotic periodic LQR (tsat_aplqr_gains, tsat_aplqr_ensemble): the source of tortoisesat.jl_amd/csrc/tsat_aplqr.hpp
under the lane emulator.

  care6 alone      four weight / inertia sets (aplqr_common.named_cases), the reference's own A with the 3U inertia and twenty random
                   stabilisable triples against the 50-digit P, by the CARE bar of tests/aplqr_common.py (4 e_ref), with A - G P
                   stable and P symmetric positive definite
  the synthesis    T = 6 slews on two 130-row tables, windows of 2, 63, 64, 65, 129 rows and the whole table with its zero last row;
                   a one-row window (rank-two Gamma) fails as the numpy restatement does and comes back zero-filled; two nearly
                   parallel rows that the restatement solves come back with status 0
  the checks       every rejection of both entry points, by its text
  the roll-out     the fixture of tests/test_gpu_pd.py (8 slews, N = 20, ragged, all five dispersions, noise, limits +-0.6) against
                   the numpy closed loop, every realisation, M = 3 and M = 70; gm = 0 through the gravity kernel is the plain kernel
                   bit for bit; a random Kg flies as given
  the wrapper      ``tracking.aplqr_gains`` raises on a failed status and hands the zeros back under allow_failed

profiles/aplqr/care_e_ref.txt holds the e_ref of every case and the residual behind ``tracking.APLQR_RES_TOL``."""
import types

import numpy as np
import pytest

import aplqr_common as ac
import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc

KINDS = ("track", "track_ff", "regulate")
CARE_CASES = ac.named_cases() + ac.random_cases()


@pytest.fixture(scope="module")
def emu(pkg):
    return ac.Emu(pkg._abi)


@pytest.fixture(scope="module")
def bars():
    """the 50-digit P and e_ref of every care6 case; computed once and left unchanged"""
    return {name: ac.care_bar(A, G, Q) for name, A, G, Q in CARE_CASES}


@pytest.mark.parametrize("case", CARE_CASES, ids=[c[0] for c in CARE_CASES])
def test_care6_matches_50_digit_reference(pkg, emu, bars, case):
    name, A, G, Q = case
    Pref, e_ref, res_np, (e_sc, e_np) = bars[name]
    assert pkg.tracking.APLQR_RES_TOL == ac.RES_TOL
    print(f"{name}: scipy {e_sc:.2e}, numpy restatement {e_np:.2e} (residual {res_np:.2e})")
    P, info = emu.care6(A, G, Q)
    assert info["status"] == 0 and 1 <= info["iterations"] <= 32 and info["pivot_min"] > 0
    ac.check_p(P, Pref, e_ref, A, G, name)
    assert abs(info["residual"] - ac.residual(A, G, Q, P)) <= 1e-3 * info["residual"] + ac.RES_NOISE
    assert info["residual"] <= ac.RES_TOL


def test_care6_reports_what_it_cannot_solve(emu):
    """no stabilising solution (an unstable mode G does not reach): not converged or a singular elimination, P zero-filled; a
    res_tol below the residual: status 3, zero-filled; non-finite input: zero-filled, finite"""
    A = np.diag([0.5, -1.0, -1.0, -1.0, -1.0, 0.0])
    G = np.zeros((6, 6))
    G[1, 1] = 1.0
    P, info = emu.care6(A, G, np.eye(6))
    assert ac.care_numpy(A, G, np.eye(6))[1] != 0
    assert info["status"] in (1, 2) and not P.any()
    name, A, G, Q = CARE_CASES[4]
    P, info = emu.care6(A, G, Q, res_tol=1e-30)
    assert info["status"] == 3 and info["residual"] > 1e-30 and not P.any()
    Qn = Q.copy()
    Qn[2, 2] = np.nan
    P, info = emu.care6(A, G, Qn)
    assert info["status"] != 0 and not P.any()


@pytest.fixture(scope="module")
def gcase(pkg, ol):
    c = ac.gains_case(pkg)
    return c, ac.gains_reference(ol, c)


def test_emulated_gains_match_reference(pkg, emu, gcase):
    c, ref = gcase
    assert [int(h - l) for l, h in zip(c["lo"], c["hi"])] == [2, 63, 64, 65, 129, 130] and not c["Btab"][:, -1].any()
    call = ac.GainsCall(pkg._abi, c)
    Kg, info = emu.gains(call)
    ac.check_gains(ref, Kg, info, "emulator")
    # the whole table through NULL windows is the last slew's explicit [0, n_tab)
    c6 = {k: (v[5:6] if k not in ("Btab",) else v) for k, v in c.items()}
    whole = ac.GainsCall(pkg._abi, c6).edit(avg_lo=None, avg_hi=None)
    Kw, iw = emu.gains(whole)
    assert Kw[0].tobytes() == Kg[5].tobytes() and iw["P"][0].tobytes() == info["P"][5].tobytes()
    # P_ss and Gamma are optional
    assert emu.gains(call.edit(P_ss=None, Gamma=None))[0].tobytes() == Kg.tobytes()


def test_emulated_gains_rank_deficient_windows(pkg, ol, emu, gcase):
    """one row: Gamma has rank two, the restatement fails, and so does the kernel — zero-filled, finite. Two rows 1e-2 rad apart: the
    restatement still solves, and the kernel has to (``aplqr_common.rank_case`` asserts the restatement's side)"""
    two = ac.rank_case(ol, gcase[0])
    Kg, info = emu.gains(ac.GainsCall(pkg._abi, two))
    ac.check_rank_case(Kg, info, "emulator")


def test_rejected_gains_arguments(pkg, emu, gcase):
    c, _ = gcase
    good = ac.GainsCall(pkg._abi, c)
    assert emu.gains_check(good) == (0, "")
    assert emu.gains_check(good.edit(avg_lo=None, avg_hi=None)) == (0, "")
    for label, call, words in ac.gains_rejections(good):
        rc, text = emu.gains_check(call)
        assert rc == -1 and words in text, (label, rc, text)
    assert emu.lib.emu_aplqr_gains(*good.edit(res_tol=-1.0).c_args()) == -1
    lib = pkg._abi.load()
    assert lib.tsat_aplqr_gains(None, *good.c_args()) == -1
    assert b"null handle" in lib.tsat_ensemble_last_error()


# ---- the roll-out ---------------------------------------------------------------------------------------------------------------

IDS = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33


@pytest.fixture(scope="module")
def cs(pkg, ol, emu):
    """the fixture of tests/test_gpu_pd.py with its plan from the oracle (1 x 3 budget), 70 realisations, the gains of the numpy
    synthesis; computed once and left unchanged. Every condition asked of it (``aplqr_common.fixture_conditions``) is asserted here,
    on the reference alone, before any roll-out test compares a kernel with it"""
    b, Rtab = pc.case(pkg)
    r = ol.solve_batch(b, hc.solve_options(ol))
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 70, np.random.default_rng(5))
    d = dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 70),
             x0n=np.ascontiguousarray(b.x0), Kg=ac.fixture_gains(ol, b))
    ac.fixture_conditions(lambda pairs, kw, Kg=None, **extra: _ref(pkg, ol, d, 3, pairs, kw, Kg, **extra), lambda kind, mode: _kw(d, kind, mode, 3),
                          d["Kg"], b)
    return d


def _kw(cs, kind, mode, M, gg=True, **over):
    kw = dict(X=None if kind == "regulate" else cs["X"], U=cs["U"] if kind == "track_ff" else None, Rtab=cs["Rtab"] if gg else None,
              gm=gc.GM if gg else 0.0, plant=np.ascontiguousarray(cs["plant"][:, :M]), sat=hc.SAT, limit_mode=mode, x0_nom=cs["x0n"], noise_id0=IDS)
    kw.update(over)
    return kw


def _ref(pkg, ol, cs, M, pairs, kw, Kg=None, **extra):
    return ac.reference_pairs(ol, pkg._abi, cs["b"], cs["x0s"][:, :M], cs["Kg"] if Kg is None else Kg, ac.RD, cs["o"], pairs, **kw, **extra)


def _check(pkg, ol, emu, cs, M, kw, Kg=None):
    """every realisation of the call against the numpy loop: none within the statistic's threshold band, none left out"""
    b = cs["b"]
    pairs = dc.all_pairs(b.T, M)
    ref = _ref(pkg, ol, cs, M, pairs, kw, Kg)
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], cs["o"].min_steps, cs["o"].w_tol, cs["o"].angle_tol)
    print(f"margin on the reference {m:.2e}; clipped knots sure {ref['n_sure'].min()} .. {ref['n_sure'].max()}, "
          f"undecided up to {int((ref['n_maybe'] - ref['n_sure']).max())}")
    assert m > dc.MARGIN, "a realisation sits within the threshold band of the statistic"
    got = emu.run(b, cs["o"], np.ascontiguousarray(cs["x0s"][:, :M]), cs["Kg"] if Kg is None else Kg, ac.RD, **kw)
    dc.compare(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom = _ref(pkg, ol, cs, M, np.array([(t, -1) for t in range(b.T)]), kw, Kg)
    ec.same_stats(nom["stats"], got["nominal"])
    return ref, got


@pytest.mark.parametrize("gg", [True, False], ids=["gg", "plain"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_rollout_matches_reference(pkg, ol, emu, cs, kind, mode, gg):
    """M = 3: every pair of 8 slews, {track, track + feed-forward, regulate} x {clip, direction-preserving} x both plant kernels"""
    _check(pkg, ol, emu, cs, 3, _kw(cs, kind, mode, 3, gg))


@pytest.mark.parametrize("kind,mode,gg", [("regulate", 1, True), ("track_ff", 0, False)])
def test_emulated_rollout_two_wavefronts(pkg, ol, emu, cs, kind, mode, gg):
    """M = 70: the model slot and six realisations in a second wavefront; every realisation compared, and realisation m >= 64 is not
    realisation m - 64. TWO of the twelve kind x limit x kernel combinations, chosen so that both plant kernels, both limit modes,
    regulation and feed-forward pass through the second wavefront: the numpy loop of 8 x 70 realisations takes six seconds a
    combination, all twelve would add a minute to every run of the suite, and what M = 70 adds to M = 3 — the lane-to-realisation
    mapping past lane 63 and the model slot's place — is the same code for every combination"""
    ref, got = _check(pkg, ol, emu, cs, 70, _kw(cs, kind, mode, 70, gg))
    full = np.flatnonzero(ec.horizons(cs["b"]) == cs["b"].N)
    d = min(float(np.max(np.abs(got["X_sim"][t, m, -1] - got["X_sim"][t, m - 64, -1]))) for t in full for m in range(64, 70))
    assert d >= gc.MOVED, d


def test_emulated_bit_equalities(pkg, emu, cs):
    b, o, M = cs["b"], cs["o"], 3
    run = lambda kw: emu.run(b, o, np.ascontiguousarray(cs["x0s"][:, :M]), cs["Kg"], ac.RD, **kw)
    same = lambda a, c: [(_ for _ in ()).throw(AssertionError(k)) for k in ("X_sim", "stats", "summary", "nominal", "n_clipped")
                         if a[k].tobytes() != c[k].tobytes()]
    # gm = 0 through the gravity kernel is the plain kernel, bit for bit
    for kind, mode in (("track_ff", 0), ("regulate", 1)):
        kw = _kw(cs, kind, mode, M, gg=True, gm=0.0)
        same(run(kw), run(dict(kw, Rtab=None)))
        assert np.max(np.abs(run(dict(kw, gm=gc.GM))["X_sim"] - run(kw)["X_sim"])) >= gc.MOVED
    # X = xf tiled against X = NULL
    tiled = np.ascontiguousarray(np.broadcast_to(b.xf[:, None, :], (b.T, b.N, 7)))
    kw = _kw(cs, "regulate", 1, M)
    same(run(kw), run(dict(kw, X=tiled)))
    # plant = NULL is the model's plant
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    same(run(dict(kw, plant=None)), run(dict(kw, plant=model)))
    # mode 1 against mode 0 under limits nothing reaches: the 1 % slews never come near +-25, the others do
    wide = run(_kw(cs, "regulate", 0, M, sat=pc.WIDE))
    quiet = [t for t in range(b.T) if ac.ALPHA[t] < 1.0]
    assert not wide["n_clipped"][quiet].any()
    w1 = run(_kw(cs, "regulate", 1, M, sat=pc.WIDE))
    assert wide["X_sim"][quiet].tobytes() == w1["X_sim"][quiet].tobytes()


def test_caller_gain_flies_as_given(pkg, ol, emu, cs):
    """a random Kg, not from the synthesis (no symmetry, no sign pattern), of a size that leaves some knots unclipped"""
    rng = np.random.default_rng(77)
    Kg = rng.standard_normal(cs["Kg"].shape) * np.array([1e7] * 3 + [1e9] * 3)[None, :, None]
    ref, got = _check(pkg, ol, emu, cs, 3, _kw(cs, "track_ff", 0, 3), Kg=Kg)
    zero = _ref(pkg, ol, cs, 3, dc.all_pairs(cs["b"].T, 3), _kw(cs, "track_ff", 0, 3), Kg=np.zeros_like(Kg))
    assert ac.moved_by(ref, zero) >= 1e-6
    assert (ref["n_sure"] < (ref["n_knots"] - 1)).any()


def test_rejected_rollout_arguments(pkg, emu, cs):
    b, M = cs["b"], 3
    good = ac.Call(pkg._abi, b, cs["o"], np.ascontiguousarray(cs["x0s"][:, :M]), cs["Kg"], ac.RD, **_kw(cs, "track_ff", 0, M))
    assert emu.check(good) == (0, "")
    for ok in (good.edit(plant=None), good.edit(Rtab=None, gm=0.0), good.edit(X=None, U=None, feedforward=0), good.edit(limit_mode=1),
               good.edit(Kg=-cs["Kg"]), good.edit(Kg=np.zeros_like(cs["Kg"]))):
        assert emu.check(ok) == (0, "")
    for label, call, words in ac.rejections(good, b, cs["Rtab"]):
        rc, text = emu.check(call)
        assert rc == -1 and words in text, (label, rc, text)
    assert emu.lib.emu_aplqr_ensemble(*good.edit(limit_mode=3).c_args()) == -1
    lib = pkg._abi.load()
    assert lib.tsat_aplqr_ensemble(None, *good.c_args()) == -1
    assert b"null handle" in lib.tsat_ensemble_last_error()


def test_wrapper_and_host_layers(pkg, emu, gcase, monkeypatch):
    """``tracking.aplqr_gains`` over the emulated synthesis in the library's place: the same arguments after the handle"""
    import os
    hdr = open(os.path.join(ec.ROOT, "include", "tortoise_hip.h")).read()
    jl = open(os.path.join(ec.ROOT, "julia", "TortoiseHIP.jl")).read()
    for name in ("tsat_aplqr_gains", "tsat_aplqr_ensemble"):
        assert name in hdr and name in pkg._abi.PROTOTYPES and f":{name}" in jl
    assert callable(pkg.tracking.attitude_ensemble_aplqr) and pkg._abi.APLQR_INFO_DTYPE == ac.INFO_DTYPE
    assert pkg._abi.load().tsat_version() == 300
    c, ref = gcase
    emu.lib.emu_aplqr_gains.argtypes = pkg._abi.PROTOTYPES["tsat_aplqr_gains"][1][1:]          # the library's prototype without the handle
    fake = types.SimpleNamespace(tsat_aplqr_gains=lambda h, *a: emu.lib.emu_aplqr_gains(*a), tsat_ensemble_last_error=lambda: b"")
    monkeypatch.setattr(pkg._abi, "load", lambda: fake)
    batch = types.SimpleNamespace(T=len(c["lo"]), Btab=c["Btab"], n_tab=c["Btab"].shape[1], xf=c["xf"], btab_idx=c["bidx"], Jmat=c["Jmat"])
    solver = types.SimpleNamespace(_h=None)
    Kg, info = pkg.tracking.aplqr_gains(solver, batch, c["qd"], c["rd"], c["alpha"], rows=(c["lo"], c["hi"]))
    ac.check_gains(ref, Kg, info, "wrapper")
    one = (np.full(batch.T, 7, dtype=np.int32), np.r_[np.full(batch.T - 1, 8), 100].astype(np.int32))     # one-row windows but the last
    with pytest.raises(RuntimeError, match="slew 0 has status"):
        pkg.tracking.aplqr_gains(solver, batch, c["qd"], c["rd"], c["alpha"], rows=one)
    Kg, info = pkg.tracking.aplqr_gains(solver, batch, c["qd"], c["rd"], c["alpha"], rows=one, allow_failed=True)
    assert np.all(info["status"][:-1] != 0) and info["status"][-1] == 0
    assert not Kg[:-1].any() and not info["P"][:-1].any() and Kg[-1].any() and np.all(np.isfinite(Kg))
