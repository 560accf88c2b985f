"""Dispersed-plant ensemble tracking (tsat_tvlqr_ensemble_dispersed), GPU tier: through the C ABI on the MI355X against the
reference closed loop of tests/dispersed_common.py (bars as in tests/test_dispersed.py), against the CPU lane emulator of the
same kernel source, against tsat_tvlqr_ensemble where the two must agree, and at size."""
import ctypes as C

import numpy as np
import pytest

import dispersed_common as dc
import ensemble_common as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    to = pkg.trajopt
    opts = to.AugmentedLagrangianSolverOptions()
    opts.opts_uncon.dJ_counter_limit = 1
    s = to.AugmentedLagrangianSolver(None, opts)

    def solve(b, budget):
        opts.iterations, opts.opts_uncon.iterations = budget
        return to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)

    yield s, solve
    s.close()


def _with_gains(ol, case):
    b, r, Qd, Qfd, Rd, x0s = case
    K = ol.tvlqr_batch(b, r["X"], r["U"], Qd, Qfd, Rd, r["X"][:, 0])["K"]          # the reference's gains: model inertia
    return b, r["X"], r["U"], Qd, Qfd, Rd, x0s, K


@pytest.fixture(scope="module")
def mc_case(pkg, ol, gpu):
    return _with_gains(ol, ec.case_monte_carlo(pkg, ol, solve=gpu[1]))


@pytest.fixture(scope="module")
def ragged_case(pkg, ol, gpu):
    return _with_gains(ol, ec.case_ragged(pkg, ol, solve=gpu[1]))


def _box(b):
    return b.ulo, b.uhi


def _run(pkg, s, case, plant, **kw):
    b, X, U, Qd, Qfd, Rd, x0s, K = case
    return pkg.tracking.attitude_ensemble_dispersed(s, b, X, U, x0s, Qd, Qfd, Rd, ec.SEED, plant, **kw)


def _nominal_pairs(T):
    return np.array([(t, -1) for t in range(T)])


def test_gpu_dispersed_matches_reference_small(pkg, ol, gpu, ragged_case):
    """every realisation of the ragged case (M = 70, all five dispersions, the plan's box), and the emulator of the same source"""
    b, X, U, Qd, Qfd, Rd, x0s, K = ragged_case
    M = x0s.shape[1]
    plant = dc.all_five_plants(pkg, b, M)
    o = ec.tv_options(ol)
    got = _run(pkg, gpu[0], ragged_case, plant, sat=_box(b), noise_id0=ec.RAGGED_ID0, want_K=True, want_trajectories=True)
    ec.same_gains(K, got["K"])
    pairs = dc.all_pairs(b.T, M)
    ref = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, plant=plant, sat=_box(b), noise_id0=ec.RAGGED_ID0)
    m = ec.margin(ref["X_sim"], ref["xf"], ref["n_knots"])
    print(f"[dispersed small] margin on the reference {m:.2e}")
    assert m > dc.MARGIN
    dc.compare(ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    nom = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, _nominal_pairs(b.T), sat=_box(b))
    ec.same_stats(nom["stats"], got["nominal"])
    # ragged horizons: zero beyond n_knots
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["K"][t, n - 1:] == 0)
    emu = ec.EmuEnsemble(pkg._abi).run(b, X, U, Qd, Qfd, Rd, x0s, got["K"], o, plant, sat=_box(b), noise_id0=ec.RAGGED_ID0)
    d = float(np.max(np.abs(emu["X_sim"] - got["X_sim"])))
    print(f"[dispersed small] GPU against the emulator: max|dX_sim| {d:.2e}")
    assert d < 1e-9
    ec.same_stats(emu["stats"], got["stats"])


def test_gpu_dispersed_matches_reference_sampled(pkg, ol, gpu, mc_case):
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    M = x0s.shape[1]
    plant = dc.all_five_plants(pkg, b, M)
    o = ec.tv_options(ol)
    got = _run(pkg, gpu[0], mc_case, plant, sat=_box(b), want_K=True, want_trajectories=True)
    ec.same_gains(K, got["K"])
    pairs = dc.sampled_pairs(b.T, M)
    ref = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, pairs, plant=plant, sat=_box(b))
    keep = dc.kept(ref)
    dc.compare(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    nom = dc.reference_pairs(ol, pkg._abi, b, X, U, K, x0s, o, _nominal_pairs(b.T), sat=_box(b))
    ec.same_stats(nom["stats"], got["nominal"])
    print(f"[dispersed sampled] failures per slew of {M}: {got['summary'][:, 1]}; clipped knots {int(got['n_clipped'].sum())}")


def test_gpu_nominal_plants_reproduce_the_ensemble(pkg, ol, gpu, mc_case, ragged_case):
    """disperse_plant(all zeros), no limits: the ensemble entry point's states to 1e-9 and its statistic; the gains bit for bit
    (the same gains kernel on the same inputs)"""
    for case, id0 in ((mc_case, None), (ragged_case, ec.RAGGED_ID0)):
        b, X, U, Qd, Qfd, Rd, x0s, K = case
        plant = pkg.tracking.disperse_plant(b.Jmat, x0s.shape[1], np.random.default_rng(1))
        ens = pkg.tracking.attitude_ensemble(gpu[0], b, X, U, x0s, Qd, Qfd, Rd, ec.SEED, noise_id0=id0, want_K=True, want_trajectories=True)
        got = _run(pkg, gpu[0], case, plant, noise_id0=id0, want_K=True, want_trajectories=True)
        d = float(np.max(np.abs(ens["X_sim"] - got["X_sim"])))
        print(f"[dispersed, model plants] against tsat_tvlqr_ensemble: max|dX_sim| {d:.2e}")
        assert d < 1e-9
        ec.same_stats(ens["stats"], got["stats"])
        ec.same_stats(ens["nominal"], got["nominal"])
        assert np.array_equal(ens["K"], got["K"])
        assert np.all(got["n_clipped"] == 0)


def test_gpu_dispersed_is_repeatable_and_prefix_stable(pkg, gpu, mc_case):
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    M = x0s.shape[1]
    plant = dc.all_five_plants(pkg, b, M)
    a = _run(pkg, gpu[0], mc_case, plant, sat=_box(b), want_K=True)
    a2 = _run(pkg, gpu[0], mc_case, plant, sat=_box(b), want_K=True)
    for f in ("stats", "summary", "nominal", "K", "n_clipped"):
        assert a[f].tobytes() == a2[f].tobytes(), f
    ens = pkg.tracking.attitude_ensemble(gpu[0], b, X, U, x0s, Qd, Qfd, Rd, ec.SEED, want_K=True)
    assert np.array_equal(ens["K"], a["K"])                       # the gains do not see the plants
    id0 = np.arange(b.T, dtype=np.int64) * M
    for Mp in (1, 64, 65):
        part = pkg.tracking.attitude_ensemble_dispersed(gpu[0], b, X, U, np.ascontiguousarray(x0s[:, :Mp]), Qd, Qfd, Rd, ec.SEED,
                                                        np.ascontiguousarray(plant[:, :Mp]), sat=_box(b), noise_id0=id0)
        assert part["stats"].shape == (b.T, Mp) and part["stats"].tobytes() == np.ascontiguousarray(a["stats"][:, :Mp]).tobytes()
        assert np.array_equal(part["n_clipped"], a["n_clipped"][:, :Mp])
        assert np.all(part["summary"][:, 0] == Mp)
        assert part["nominal"].tobytes() == a["nominal"].tobytes()


def test_gpu_dispersed_rejections(pkg, gpu, ragged_case):
    """every listed error returns -1 with its word (and the offending (t, m)) in tsat_ensemble_last_error(); a good call
    afterwards returns 0 with an empty text"""
    s = gpu[0]
    b, X, U, Qd, Qfd, Rd, x0s, K = ragged_case
    lib, abi = pkg._abi.load(), pkg._abi
    T, N, M = b.T, b.N, x0s.shape[1]
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    X, U, Qd, Qfd, Rd, x0s = c(X), c(U), c(Qd), c(Qfd), c(Rd), c(x0s)
    good = dc.all_five_plants(pkg, b, M)
    lo0, hi0 = c(b.ulo), c(b.uhi)

    def call(M=M, nk=b.n_knots, x0=x0s, plant=good, lo=lo0, hi=hi0, **opt):
        o = abi.TvlqrOptions()
        lib.tsat_tvlqr_default_options(C.byref(o))
        o.n_knots, o.n_tab, o.noise_mode, o.noise_seed = N, b.n_tab, 1, ec.SEED
        for k, v in opt.items():
            setattr(o, k, v)
        st = np.zeros((T, max(M, 1)), dtype=abi.TVLQR_STATS_DTYPE)
        summary = np.zeros((T, 8))
        d = abi.as_dp
        nk = np.ascontiguousarray(nk, dtype=np.int32)
        rc = lib.tsat_tvlqr_ensemble_dispersed(s._h, C.byref(o), T, b.Btab.shape[0], M, d(X), d(U), d(b.xf), d(b.Btab),
                                               abi.as_ip(b.btab_idx), d(b.tau0), d(b.dtau), d(b.dt), d(b.Jmat), d(Qd), d(Qfd), d(Rd),
                                               d(x0), None, abi.as_ip(nk), None if plant is None else d(c(plant)), d(lo), d(hi),
                                               st.ctypes.data_as(C.c_void_p), d(summary), None, None, None, None)
        return rc, lib.tsat_ensemble_last_error()

    def edit(i, v, t=1, m=66):
        p = good.copy()
        p[t, m, i] = v
        return p

    skew = good.copy(); skew[2, 5, 3] += 1e-9 * np.abs(good[2, 5, :9]).max()          # Jp(0,1) != Jp(1,0)
    indef = good.copy(); indef[0, 69, 0:9] = np.diag([0.01, -0.02, 0.03]).reshape(9)
    minor = good.copy(); minor[0, 0, 0:9] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]).reshape(9)   # 2nd leading minor < 0
    hi_bad = hi0.copy(); hi_bad[1, 2] = lo0[1, 2] - 1.0
    rc, msg = call()
    assert rc == 0 and msg == b""
    for kw, words in ((dict(plant=None), (b"plant",)), (dict(plant=edit(20, np.nan)), (b"non-finite", b"(1, 66)")),
                      (dict(plant=edit(10, np.inf)), (b"non-finite", b"(1, 66)")), (dict(plant=skew), (b"not symmetric", b"(2, 5)")),
                      (dict(plant=indef), (b"not positive definite", b"(0, 69)")), (dict(plant=minor), (b"not positive definite", b"(0, 0)")),
                      (dict(lo=None), (b"exactly one",)), (dict(hi=None), (b"exactly one",)), (dict(hi=hi_bad), (b"sat_lo > sat_hi", b"t = 1")),
                      # and what tsat_tvlqr_ensemble rejects
                      (dict(noise_mode=0), (b"noise_mode",)), (dict(rate_as_written=1), (b"rate_as_written",)), (dict(M=0), (b"M must",)),
                      (dict(x0=None), (b"null",)), (dict(nk=(60, 1, 12)), (b"n_knots",))):
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (list(kw), rc, msg)
    rc, msg = call(lo=None, hi=None)
    assert rc == 0 and msg == b""            # no limits at all is a good call; the text is the LAST call's


def test_gpu_dispersed_at_size(pkg, ol, gpu):
    """the configs[1] workload (1024 slews x 1000 knots, solved here) x 64 plants with all five dispersions and the plan's box:
    65 536 closed loops in one call; 34 seeded (t, m) drawn, the first 32 that meet the margin against the reference"""
    s, solve = gpu
    b = pkg.slew_setup.workload_monte_carlo(T=1024, N=1000)
    r = solve(b, (5, 10))
    M = 64
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    plant = dc.all_five_plants(pkg, b, M)
    got = pkg.tracking.attitude_ensemble_dispersed(s, b, r["X"], r["U"], x0s, Qd, Qfd, Rd, ec.SEED, plant, sat=_box(b))
    st = got["stats"]
    assert st.shape == (1024, M) and got["n_clipped"].shape == (1024, M)
    for f in ("slew_time", "final_w_norm", "final_angle"):
        assert np.all(np.isfinite(st[f])), f
    assert np.all(np.isfinite(got["summary"])) and np.all(got["summary"][:, 0] == M) and np.all(got["summary"][:, 1] <= M)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(st), rtol=1e-12)
    assert np.all(got["n_clipped"] >= 0) and np.all(got["n_clipped"] <= b.N - 1)
    print(f"[dispersed at size] failures over 65 536 loops: {int(got['summary'][:, 1].sum())}; clipped knots {int(got['n_clipped'].sum())}")
    pairs = dc.sampled_pairs(b.T, M)
    ts = np.unique(pairs[:, 0])
    K = np.zeros((b.T, b.N - 1, 6, 3))
    K[ts] = ol.tvlqr_batch(_rows(b, ts), r["X"][ts], r["U"][ts], Qd[ts], Qfd[ts], Rd[ts], r["X"][ts, 0])["K"]
    ref = dc.reference_pairs(ol, pkg._abi, b, r["X"], r["U"], K, x0s, ec.tv_options(ol), pairs, plant=plant, sat=_box(b))
    keep = dc.kept(ref)
    dc.compare(ref, got, pairs, keep)


def _rows(batch, idx):
    """the slews `idx` of a batch (per-slew arrays of tests/ensemble_common.py)"""
    import dataclasses
    kw = {k: np.ascontiguousarray(getattr(batch, k)[idx]) for k in ec.PER_SLEW}
    if batch.n_knots is not None:
        kw["n_knots"] = np.ascontiguousarray(batch.n_knots[idx])
    return dataclasses.replace(batch, **kw)


def test_gpu_nominal_entry_point_is_untouched(pkg, ol, gpu, mc_case):
    """a dispersed call on the same handle leaves tsat_tvlqr_ensemble as it was: the same bytes before and after it, and
    realisations m in {0, 63, 64, 99} still are the tracking kernel's runs (states, gains, slew indices — the bars of
    test_gpu_ensemble.py::test_gpu_realisations_equal_the_tracking_kernel)"""
    s = gpu[0]
    b, X, U, Qd, Qfd, Rd, x0s, K = mc_case
    tr = pkg.tracking
    id0 = np.array([11, 2 ** 34, 500, 7000], dtype=np.int64)
    ens = lambda: tr.attitude_ensemble(s, b, X, U, x0s, Qd, Qfd, Rd, ec.SEED, noise_id0=id0, want_K=True, want_trajectories=True)
    before = ens()
    _run(pkg, s, mc_case, dc.all_five_plants(pkg, b, x0s.shape[1]), sat=_box(b))
    got = ens()
    for f in ("stats", "summary", "nominal", "K", "X_sim"):
        assert before[f].tobytes() == got[f].tobytes(), f
    worst = 0.0
    for m in (0, 63, 64, 99):
        one = tr.attitude_simulation(s, b, X, U, x0s[:, m], Qd, Qfd, Rd, noise_seed=ec.SEED, noise_ids=id0 + m)
        assert np.array_equal(one["stats"]["slew_index"], got["stats"]["slew_index"][:, m])
        worst = max(worst, float(np.max(np.abs(one["X_sim"] - got["X_sim"][:, m]))))
        assert np.array_equal(one["K"], got["K"])
    print(f"[ensemble after a dispersed call vs tracking kernel] max|dX_sim| over m in (0, 63, 64, 99): {worst:.2e}")
    assert worst < 1e-9
