"""Ensemble tracking (tsat_tvlqr_ensemble), GPU tier: through the C ABI on the MI355X, against the unchanged oracle realisation
by realisation (bars of tests/test_tracking.py::_same_tracking), against the existing tracking kernel, and at size."""
import ctypes as C

import numpy as np
import pytest

import ensemble_common as ec

pytestmark = pytest.mark.gpu
MARGIN = 1e-7


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


@pytest.fixture(scope="module")
def mc_case(pkg, ol, gpu):
    return ec.case_monte_carlo(pkg, ol, solve=gpu[1])


@pytest.fixture(scope="module")
def ragged_case(pkg, ol, gpu):
    return ec.case_ragged(pkg, ol, solve=gpu[1])


def _against_oracle(pkg, ol, s, case, sigma_scale=1.0, noise_id0=None):
    b, r, Qd, Qfd, Rd, x0s = case
    M = x0s.shape[1]
    got = pkg.tracking.attitude_ensemble(s, b, r["X"], r["U"], x0s, Qd, Qfd, Rd, ec.SEED, noise_id0=noise_id0, sigma_scale=sigma_scale,
                                         want_K=True, want_trajectories=True)
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, noise_id0=noise_id0, sigma_scale=sigma_scale)
    m = ec.margin(ref["X_sim"].reshape((-1,) + ref["X_sim"].shape[2:]), ref["batch"].xf, ec.horizons(b, M))
    dX = float(np.max(np.abs(ref["X_sim"] - got["X_sim"])))
    print(f"[ensemble vs oracle, sigma x {sigma_scale:g}] margin on the oracle {m:.2e}, max|dX_sim| {dX:.2e}, "
          f"failures per slew {ref['stats']['failed'].sum(axis=1)}")
    assert m > MARGIN
    assert dX < 1e-9
    ec.same_stats(ref["stats"], got["stats"])
    ec.same_gains(ref["K"], got["K"])
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    # the gains are those of the tracking entry point, bit for bit
    one = pkg.tracking.attitude_simulation(s, b, r["X"], r["U"], x0s[:, 0], Qd, Qfd, Rd, want_trajectories=False)
    assert np.array_equal(one["K"], got["K"])
    return ref, got


@pytest.mark.parametrize("sigma_scale", [1.0, 60.0])
def test_gpu_ensemble_matches_oracle(pkg, ol, gpu, mc_case, sigma_scale):
    ref, got = _against_oracle(pkg, ol, gpu[0], mc_case, sigma_scale=sigma_scale)
    fails = got["summary"][:, 1]
    assert (fails.sum() == 0) if sigma_scale == 1.0 else (np.all(fails > 0) and np.all(fails < mc_case[5].shape[1]))


def test_gpu_ensemble_ragged_matches_oracle(pkg, ol, gpu, ragged_case):
    ref, got = _against_oracle(pkg, ol, gpu[0], ragged_case, noise_id0=ec.RAGGED_ID0)
    b = ragged_case[0]
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["K"][t, n - 1:] == 0)
    assert np.all(got["summary"][:, 1] == ragged_case[5].shape[1]) and np.all(got["summary"][:, 2:5] == 0)
    np.testing.assert_allclose(got["summary"][:, 5], b.dt * b.n_knots, rtol=1e-12)


def test_gpu_realisations_equal_the_tracking_kernel(pkg, ol, gpu, mc_case):
    """realisation (t, m) against the EXISTING kernel's run of it; the nominal statistic against its noise-free run"""
    s = gpu[0]
    b, r, Qd, Qfd, Rd, x0s = mc_case
    tr = pkg.tracking
    id0 = np.array([11, 2 ** 34, 500, 7000], dtype=np.int64)
    got = tr.attitude_ensemble(s, b, r["X"], r["U"], x0s, Qd, Qfd, Rd, ec.SEED, noise_id0=id0, want_K=True, want_trajectories=True)
    worst = 0.0
    for m in (0, 63, 64, 99):
        one = tr.attitude_simulation(s, b, r["X"], r["U"], x0s[:, m], Qd, Qfd, Rd, noise_seed=ec.SEED, noise_ids=id0 + m)
        assert np.array_equal(one["stats"]["slew_index"], got["stats"]["slew_index"][:, m])
        worst = max(worst, float(np.max(np.abs(one["X_sim"] - got["X_sim"][:, m]))))
        assert np.array_equal(one["K"], got["K"])
    print(f"[ensemble vs tracking kernel] max|dX_sim| over m in (0, 63, 64, 99): {worst:.2e}")
    assert worst < 1e-9
    nom = tr.attitude_simulation(s, b, r["X"], r["U"], r["X"][:, 0], Qd, Qfd, Rd, want_K=False, want_trajectories=False)
    ec.same_stats(nom["stats"], got["nominal"])
    assert np.array_equal(nom["stats"]["slew_time"], got["nominal"]["slew_time"])


def test_gpu_ensemble_is_repeatable_and_seeded(pkg, gpu, mc_case):
    s = gpu[0]
    b, r, Qd, Qfd, Rd, x0s = mc_case
    run = lambda seed, x=x0s: pkg.tracking.attitude_ensemble(s, b, r["X"], r["U"], x, Qd, Qfd, Rd, seed)
    a, a2, other = run(ec.SEED), run(ec.SEED), run(ec.SEED + 1)
    assert a["stats"].tobytes() == a2["stats"].tobytes() and a["summary"].tobytes() == a2["summary"].tobytes()
    assert a["stats"].tobytes() != other["stats"].tobytes()
    # M = 1, 64, 65: the first realisations of the larger ensemble (ids t M + m differ with M, so give them)
    id0 = np.arange(b.T, dtype=np.int64) * x0s.shape[1]
    for M in (1, 64, 65):
        part = pkg.tracking.attitude_ensemble(s, b, r["X"], r["U"], np.ascontiguousarray(x0s[:, :M]), Qd, Qfd, Rd, ec.SEED, noise_id0=id0)
        assert part["stats"].shape == (b.T, M) and part["stats"].tobytes() == np.ascontiguousarray(a["stats"][:, :M]).tobytes()
        assert np.all(part["summary"][:, 0] == M)
        assert part["nominal"].tobytes() == a["nominal"].tobytes()


def test_gpu_ensemble_rejections(pkg, gpu, ragged_case):
    """bad arguments return -1 with a text in tsat_ensemble_last_error()"""
    s = gpu[0]
    b, r, Qd, Qfd, Rd, x0s = ragged_case
    lib, abi = pkg._abi.load(), pkg._abi
    T, N, M = b.T, b.N, x0s.shape[1]
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    X, U, Qd, Qfd, Rd, x0s = c(r["X"]), c(r["U"]), c(Qd), c(Qfd), c(Rd), c(x0s)

    def call(M=M, nk=b.n_knots, x0=x0s, **opt):
        o = abi.TvlqrOptions()
        lib.tsat_tvlqr_default_options(C.byref(o))
        o.n_knots, o.n_tab, o.noise_mode, o.noise_seed = N, b.n_tab, 1, ec.SEED
        for k, v in opt.items():
            setattr(o, k, v)
        st = np.zeros((T, max(M, 1)), dtype=abi.TVLQR_STATS_DTYPE)
        summary = np.zeros((T, 8))
        d = abi.as_dp
        nk = np.ascontiguousarray(nk, dtype=np.int32)
        rc = lib.tsat_tvlqr_ensemble(s._h, C.byref(o), T, b.Btab.shape[0], M, d(X), d(U), d(b.xf), d(b.Btab), abi.as_ip(b.btab_idx),
                                     d(b.tau0), d(b.dtau), d(b.dt), d(b.Jmat), d(Qd), d(Qfd), d(Rd), d(x0), None, abi.as_ip(nk),
                                     st.ctypes.data_as(C.c_void_p), d(summary), None, None, None)
        return rc, lib.tsat_ensemble_last_error()

    rc, msg = call()
    assert rc == 0 and msg == b""
    for kw, word in ((dict(noise_mode=0), b"noise_mode"), (dict(rate_as_written=1), b"rate_as_written"), (dict(M=0), b"M must"),
                     (dict(M=65536), b"M must"), (dict(x0=None), b"null"), (dict(nk=(60, 1, 12)), b"n_knots")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call()
    assert rc == 0 and msg == b""            # the text is the LAST call's


def test_gpu_ensemble_at_size(pkg, ol, gpu):
    """the configs[1] workload (1024 slews x 1000 knots, solved here) x 64 realisations = 65 536 closed loops in one call; 32
    seeded (t, m) pairs against the oracle (a pair whose oracle run fails the margin condition is replaced by the next one)"""
    s, solve = gpu
    b = pkg.slew_setup.workload_monte_carlo(T=1024, N=1000)
    r = solve(b, (5, 10))
    M = 64
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    got = pkg.tracking.attitude_ensemble(s, b, r["X"], r["U"], x0s, Qd, Qfd, Rd, ec.SEED)
    st = got["stats"]
    assert st.shape == (1024, M)
    for f in ("slew_time", "final_w_norm", "final_angle"):
        assert np.all(np.isfinite(st[f])), f
    assert np.all(np.isfinite(got["summary"])) and np.all(got["summary"][:, 0] == M) and np.all(got["summary"][:, 1] <= M)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(st), rtol=1e-12)
    rng = np.random.default_rng(32)
    pairs = np.stack([rng.integers(0, b.T, 34), rng.integers(0, M, 34)], axis=1)
    ref = ec.oracle_ensemble(ol, b, r["X"], r["U"], Qd, Qfd, Rd, x0s, pairs=pairs)
    ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["batch"].xf[i:i + 1], [b.N]) > MARGIN for i in range(len(pairs))])
    keep = np.flatnonzero(ok)[:32]
    print(f"[ensemble at size] failures over 65 536 loops: {int(got['summary'][:, 1].sum())}; pairs replaced {int(np.count_nonzero(~ok[:keep[-1] + 1]))}")
    assert keep.size == 32
    ec.same_stats(ref["stats"][keep], st[pairs[keep, 0], pairs[keep, 1]])
