"""GPU tier of the asymptotic periodic LQR (tsat_aplqr_gains through ``tracking.aplqr_gains``, tsat_aplqr_ensemble through
``tracking.attitude_ensemble_aplqr``) on the shapes of tests/test_aplqr.py against the same references: the 50-digit P with the
CARE bar (4 e_ref) and the numpy Gramian for the synthesis, the numpy closed loop of tests/aplqr_common.py with the bars of
dispersed_common.compare for the roll-out. No emulator library is used here.

The synthesis: T = 6 slews on two 130-row tables, windows of 2, 63, 64, 65, 129 rows and the whole table with its zero last row; a
one-row window comes back with a status and zeros, two rows 1e-2 rad apart with status 0. The roll-out: the fixture of tests/test_gpu_pd.py with the gains of the numpy
synthesis, M = 3 for every {kind} x {limit mode} x {plant kernel} and M = 70 (two wavefronts) for two of them, every realisation
compared; a random gain of the caller's; what the entry points reject, with the handle's workspace unchanged; two identical calls
byte for byte; a regulation call grows nothing with N."""
import numpy as np
import pytest

import aplqr_common as ac
import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc

pytestmark = pytest.mark.gpu

STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
KINDS = ("track", "track_ff", "regulate")
OUT = ("stats", "summary", "nominal", "X_sim", "n_clipped")
IDS = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


def _ws(pkg, solver):
    return int(pkg._abi.load().tsat_workspace_bytes(solver._h))


def _trim(pkg, solver):
    assert pkg._abi.load().tsat_workspace_trim(solver._h, 1) == 0
    assert _ws(pkg, solver) == 0


@pytest.fixture(scope="module")
def gcase(pkg, ol):
    c = ac.gains_case(pkg)
    return c, ac.gains_reference(ol, c)


def _batch(pkg, c):
    """the slews of ``aplqr_common.gains_case`` as the wrapper takes them"""
    import types
    return types.SimpleNamespace(T=len(c["lo"]), Btab=c["Btab"], n_tab=c["Btab"].shape[1], xf=c["xf"], btab_idx=c["bidx"], Jmat=c["Jmat"])


def test_gpu_gains_match_reference(pkg, solver, gcase):
    c, ref = gcase
    assert pkg.tracking.APLQR_RES_TOL == ac.RES_TOL
    b = _batch(pkg, c)
    Kg, info = pkg.tracking.aplqr_gains(solver, b, c["qd"], c["rd"], c["alpha"], rows=(c["lo"], c["hi"]))
    ac.check_gains(ref, Kg, info, "GPU")
    assert np.all(info["residual"] <= ac.RES_TOL) and np.all(info["pivot_min"] > 0)
    # a second identical call is bit-identical
    K2, i2 = pkg.tracking.aplqr_gains(solver, b, c["qd"], c["rd"], c["alpha"], rows=(c["lo"], c["hi"]))
    assert K2.tobytes() == Kg.tobytes() and all(i2[k].tobytes() == info[k].tobytes() for k in info)
    # the whole table through NULL windows is the last slew's explicit [0, n_tab)
    c6 = {k: (v[5:6] if k != "Btab" else v) for k, v in c.items()}
    Kw, iw = pkg.tracking.aplqr_gains(solver, _batch(pkg, c6), c6["qd"], c6["rd"], c6["alpha"])
    assert Kw[0].tobytes() == Kg[5].tobytes() and iw["P"][0].tobytes() == info["P"][5].tobytes()


def test_gpu_gains_rank_deficient_windows(pkg, ol, solver, gcase):
    """the two slews of ``aplqr_common.rank_case``: the one-row window (rank-two Gamma) comes back with a status and zeros, the two
    rows 1e-2 rad apart, which the restatement solves, with status 0, a gain and a stable A - G P — the device's reciprocal, log and
    exp are not the emulator's, and this is the case next to the edge. Then the wrapper: it raises on a status unless told"""
    c, ref = gcase
    two = ac.rank_case(ol, c)
    Kg, info = pkg.tracking.aplqr_gains(solver, _batch(pkg, two), two["qd"], two["rd"], two["alpha"], rows=(two["lo"], two["hi"]), allow_failed=True)
    ac.check_rank_case(Kg, info, "GPU")
    b = _batch(pkg, c)
    one = (np.full(b.T, 7, dtype=np.int32), np.r_[np.full(b.T - 1, 8), 100].astype(np.int32))
    with pytest.raises(RuntimeError, match="slew 0 has status"):
        pkg.tracking.aplqr_gains(solver, b, c["qd"], c["rd"], c["alpha"], rows=one)
    Kg, info = pkg.tracking.aplqr_gains(solver, b, c["qd"], c["rd"], c["alpha"], rows=one, allow_failed=True)
    assert np.all(info["status"][:-1] != 0) and info["status"][-1] == 0
    assert not Kg[:-1].any() and not info["P"][:-1].any() and Kg[-1].any()
    assert np.all(np.isfinite(Kg)) and np.all(np.isfinite(info["P"])) and np.all(np.isfinite(info["Gamma"]))


def test_gpu_gains_rejections_and_workspace(pkg, solver, gcase):
    c, _ = gcase
    lib = pkg._abi.load()
    good = ac.GainsCall(pkg._abi, c)
    _trim(pkg, solver)
    for label, call, words in ac.gains_rejections(good):
        rc = lib.tsat_aplqr_gains(solver._h, *call.c_args())
        msg = lib.tsat_ensemble_last_error().decode()
        assert rc == -1 and words in msg, (label, rc, msg)
        assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    assert lib.tsat_aplqr_gains(solver._h, *good.c_args()) == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) == 0                                # the synthesis keeps nothing on the handle


# ---- the roll-out ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ens(pkg, ol, solver):
    """the plan (solved here, 1 x 3 budget), 70 realisations, their plants and the gains of the numpy synthesis; computed once"""
    to = pkg.trajopt
    b, Rtab = pc.case(pkg)
    solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
    r = to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, 70, np.random.default_rng(5))
    d = dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, 70),
             x0n=np.ascontiguousarray(b.x0), Kg=ac.fixture_gains(ol, b))
    # the plan of this tier is the library's, not the oracle's: the fixture's conditions are asserted on it too, on the reference alone
    ac.fixture_conditions(lambda pairs, kw, Kg=None, **extra: _ref(pkg, ol, d, 3, pairs, kw, Kg, **extra), lambda kind, mode: _kw(d, kind, mode, 3),
                          d["Kg"], b)
    return d


def _kw(e, kind, mode, M, gg=True, **over):
    kw = dict(X=None if kind == "regulate" else e["X"], U=e["U"] if kind == "track_ff" else None, Rtab=e["Rtab"] if gg else None,
              gm=gc.GM if gg else 0.0, plant=np.ascontiguousarray(e["plant"][:, :M]), sat=hc.SAT, limit_mode=mode, x0_nom=e["x0n"], noise_id0=IDS)
    kw.update(over)
    return kw


def _run(pkg, solver, e, M, kw, Kg=None, batch=None, traj=True):
    return pkg.tracking.attitude_ensemble_aplqr(solver, batch or e["b"], np.ascontiguousarray(e["x0s"][:, :M]), e["Kg"] if Kg is None else Kg,
                                                ac.RD, ec.SEED, want_trajectories=traj, **STAT, **kw)


def _ref(pkg, ol, e, M, pairs, kw, Kg=None, **extra):
    return ac.reference_pairs(ol, pkg._abi, e["b"], e["x0s"][:, :M], e["Kg"] if Kg is None else Kg, ac.RD, e["o"], pairs, **kw, **extra)


def _check(pkg, ol, solver, e, M, kw, Kg=None):
    """every realisation of the call against the numpy loop: none within the statistic's threshold band, none left out"""
    b = e["b"]
    pairs = dc.all_pairs(b.T, M)
    ref = _ref(pkg, ol, e, M, pairs, kw, Kg)
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"], e["o"].min_steps, e["o"].w_tol, e["o"].angle_tol)
    print(f"margin on the reference {m:.2e}; clipped knots sure {ref['n_sure'].min()} .. {ref['n_sure'].max()}")
    assert m > dc.MARGIN, "a realisation sits within the threshold band of the statistic"
    got = _run(pkg, solver, e, M, kw, Kg)
    dc.compare(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0)
    nom = _ref(pkg, ol, e, M, np.array([(t, -1) for t in range(b.T)]), kw, Kg)
    ec.same_stats(nom["stats"], got["nominal"])
    return ref, got


@pytest.mark.parametrize("gg", [True, False], ids=["gg", "plain"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_rollout_matches_reference(pkg, ol, solver, ens, kind, mode, gg):
    _check(pkg, ol, solver, ens, 3, _kw(ens, kind, mode, 3, gg))


@pytest.mark.parametrize("kind,mode,gg", [("regulate", 1, True), ("track_ff", 0, False)])
def test_gpu_rollout_two_wavefronts(pkg, ol, solver, ens, kind, mode, gg):
    """M = 70: the model slot and six realisations in a second wavefront; every realisation compared. Two of the twelve combinations,
    as in tests/test_aplqr.py and for its reason: six seconds of numpy reference each, and both plant kernels, both limit modes,
    regulation and feed-forward are among the two"""
    ref, got = _check(pkg, ol, solver, ens, 70, _kw(ens, kind, mode, 70, gg))
    full = np.flatnonzero(ec.horizons(ens["b"]) == ens["b"].N)
    d = min(float(np.max(np.abs(got["X_sim"][t, m, -1] - got["X_sim"][t, m - 64, -1]))) for t in full for m in range(64, 70))
    assert d >= gc.MOVED, d


def _same_bytes(a, c, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_gpu_bit_equalities(pkg, solver, ens):
    e, b, M = ens, ens["b"], 70
    run = lambda kw: _run(pkg, solver, e, M, kw)
    # a second identical call is bit-identical
    kw = _kw(e, "track_ff", 1, M)
    _same_bytes(run(kw), run(kw))
    # gm = 0 through the gravity kernel is the plain kernel, bit for bit
    kw = _kw(e, "track_ff", 0, M, gm=0.0)
    off = run(kw)
    _same_bytes(off, run(dict(kw, Rtab=None)))
    assert np.max(np.abs(run(dict(kw, gm=gc.GM))["X_sim"] - off["X_sim"])) >= gc.MOVED
    # X = xf tiled against X = NULL, the same explicit x0_nom; plant = NULL is the model's plant
    tiled = np.ascontiguousarray(np.broadcast_to(b.xf[:, None, :], (b.T, b.N, 7)))
    kw = _kw(e, "regulate", 1, M)
    _same_bytes(run(kw), run(dict(kw, X=tiled)))
    model = pkg.tracking.disperse_plant(b.Jmat, M, np.random.default_rng(0))
    _same_bytes(run(dict(kw, plant=None)), run(dict(kw, plant=model)))


def test_gpu_caller_gain_flies_as_given(pkg, ol, solver, ens):
    rng = np.random.default_rng(77)
    Kg = rng.standard_normal(ens["Kg"].shape) * np.array([1e7] * 3 + [1e9] * 3)[None, :, None]
    ref, got = _check(pkg, ol, solver, ens, 3, _kw(ens, "track_ff", 0, 3), Kg=Kg)
    zero = _ref(pkg, ol, ens, 3, dc.all_pairs(ens["b"].T, 3), _kw(ens, "track_ff", 0, 3), Kg=np.zeros_like(Kg))
    assert ac.moved_by(ref, zero) >= 1e-6


def test_gpu_synthesised_gain_flies(pkg, ol, solver, ens):
    """the two calls in a row, as a user makes them: the gains of tsat_aplqr_gains over each slew's whole table, handed to
    tsat_aplqr_ensemble; the roll-out with them matches the reference flown with THEM"""
    b = ens["b"]
    Kg, info = pkg.tracking.aplqr_gains(solver, b, ac.QD, ac.RD, ac.ALPHA)
    assert not info["status"].any()
    rel = float(np.max(np.abs(Kg - ens["Kg"])) / np.max(np.abs(ens["Kg"])))
    print(f"device gains against the numpy synthesis: {rel:.2e} of the largest entry (a figure: Gamma is nearly of rank two here, and the "
          "CARE bar is pinned on the cases of test_gpu_gains_match_reference)")
    _check(pkg, ol, solver, ens, 3, _kw(ens, "regulate", 1, 3), Kg=Kg)


def test_gpu_rejections_and_workspace(pkg, solver, ens):
    """every listed error returns -1 with its text and leaves the handle's workspaces empty; a regulating call without an orbit table
    grows them by nothing that scales with N (N = 20 against N = 2000)"""
    e, b = ens, ens["b"]
    lib, M = pkg._abi.load(), 5
    good = ac.Call(pkg._abi, b, e["o"], np.ascontiguousarray(e["x0s"][:, :M]), e["Kg"], ac.RD, **_kw(e, "track_ff", 0, M))
    _trim(pkg, solver)
    for label, call, words in ac.rejections(good, b, e["Rtab"]):
        rc = lib.tsat_aplqr_ensemble(solver._h, *call.c_args())
        msg = lib.tsat_ensemble_last_error().decode()
        assert rc == -1 and words in msg, (label, rc, msg)
        assert _ws(pkg, solver) == 0, "a rejected call reached the device"
    sizes = []
    for N in (20, 2000):
        bn = hc.mpc_batch(pkg, T=2, N=N)
        x0s = pkg.tracking.ensemble_initial_states(bn.x0, M, np.random.default_rng(5))
        r = pkg.tracking.attitude_ensemble_aplqr(solver, bn, x0s, e["Kg"][:2], ac.RD, ec.SEED, sat=hc.SAT, limit_mode=1, **STAT)
        assert r["nominal"] is None and r["X_sim"] is None and np.all(np.isfinite(r["summary"]))
        sizes.append(_ws(pkg, solver))
    assert sizes[0] == sizes[1], sizes
    rc = lib.tsat_aplqr_ensemble(solver._h, *good.c_args())
    assert rc == 0 and lib.tsat_ensemble_last_error() == b""
    assert _ws(pkg, solver) - sizes[1] == 32 * e["Rtab"].shape[0] * e["Rtab"].shape[1]      # the packed gravity rows, the handle's
    _trim(pkg, solver)
