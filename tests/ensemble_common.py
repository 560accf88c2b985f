"""Shared pieces of tests/test_ensemble.py (CPU tier) and tests/test_gpu_ensemble.py (GPU tier): the cases, the oracle side of
every comparison (the unchanged ``oracle_lib.tvlqr_batch`` on the batch replicated M times), the margin condition that keeps
index equality meaningful, the bars of ``tests/test_tracking.py::_same_tracking`` per realisation, and the ctypes binding of the
emulated ensemble kernels, nominal and dispersed (tests/emu/tsat_emu_ensemble.cpp)."""
import ctypes as C
import dataclasses

import numpy as np

import helpers
from conftest import ROOT, oracle_options  # noqa: F401  (the tests reach ROOT through this module)

SEED = 2019
PER_SLEW = ("x0", "xf", "btab_idx", "tau0", "dtau", "dt", "Jmat", "Qd", "Qfd", "Rd", "ulo", "uhi", "U0")


def replicate(batch, M):
    """the batch with every slew repeated M times, slew-major (t * M + m)"""
    idx = np.repeat(np.arange(batch.T), M)
    kw = {k: np.ascontiguousarray(getattr(batch, k)[idx]) for k in PER_SLEW}
    if batch.n_knots is not None:
        kw["n_knots"] = np.ascontiguousarray(batch.n_knots[idx])
    return dataclasses.replace(batch, **kw), idx


def tv_options(ol, seed=SEED, sigma_scale=1.0):
    o = ol.tvlqr_default_options()
    o.noise_mode, o.noise_seed = 1, seed
    o.sigma_gyro, o.sigma_att = o.sigma_gyro * sigma_scale, o.sigma_att * sigma_scale
    return o


def oracle_ensemble(ol, batch, X, U, Qd, Qfd, Rd, x0_sim, seed=SEED, noise_id0=None, sigma_scale=1.0, nthreads=8, pairs=None):
    """realisation (t, m) = the oracle's tvlqr_batch run of slew t with x0_sim[t, m], noise_mode = 1, id noise_id0[t] + m.
    ``pairs`` (n, 2): only those (t, m); the results then have a leading axis n instead of (T, M)."""
    T, M = x0_sim.shape[:2]
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    if pairs is None:
        rb, idx = replicate(batch, M)
        ids = (id0[:, None] + np.arange(M, dtype=np.int64)[None, :]).ravel()
        x0s = x0_sim.reshape(T * M, 7)
    else:
        pairs = np.asarray(pairs)
        idx = pairs[:, 0]
        kw = {k: np.ascontiguousarray(getattr(batch, k)[idx]) for k in PER_SLEW}
        if batch.n_knots is not None:
            kw["n_knots"] = np.ascontiguousarray(batch.n_knots[idx])
        rb = dataclasses.replace(batch, **kw)
        ids = id0[idx] + pairs[:, 1]
        x0s = np.ascontiguousarray(x0_sim[pairs[:, 0], pairs[:, 1]])
    r = ol.tvlqr_batch(rb, X[idx], U[idx], Qd[idx], Qfd[idx], Rd[idx], x0s, opts=tv_options(ol, seed, sigma_scale),
                       nthreads=min(nthreads, ol.num_procs()), noise_ids=ids)
    if pairs is not None:
        return dict(X_sim=r["X_sim"], stats=r["stats"], K=r["K"], batch=rb)
    N = batch.N
    return dict(X_sim=r["X_sim"].reshape(T, M, N, 7), stats=r["stats"].reshape(T, M), K=np.ascontiguousarray(r["K"][::M]), batch=rb)


def margin(X_sim, xf, n_knots, min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """over all samples j > min_steps of trajectories X_sim (n, N, 7) with goals xf (n, 7) and horizons n_knots (n,):
    min(| |w| - w_tol | / w_tol, | angle - angle_tol | / angle_tol) — how far the nearest sample is from a threshold"""
    n, N = X_sim.shape[:2]
    w = np.linalg.norm(X_sim[:, :, :3], axis=2)
    qf, q = xf[:, None, 3:7], X_sim[:, :, 3:7]
    e0 = qf[..., 0] * q[..., 0] + qf[..., 1] * q[..., 1] + qf[..., 2] * q[..., 2] + qf[..., 3] * q[..., 3]
    ang = 2.0 * np.arccos(np.minimum(e0, 1.0))
    d = np.minimum(np.abs(w - w_tol) / w_tol, np.abs(ang - angle_tol) / angle_tol)
    j = np.arange(1, N + 1)[None, :]
    live = (j > min_steps) & (j <= np.asarray(n_knots)[:, None])
    return float(d[live].min())


def same_stats(ref, got):
    """the bars of tests/test_tracking.py::_same_tracking on the statistic, every realisation"""
    assert np.array_equal(ref["slew_index"], got["slew_index"])
    assert np.array_equal(ref["failed"], got["failed"])
    np.testing.assert_allclose(got["final_angle"], ref["final_angle"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got["final_w_norm"], ref["final_w_norm"], rtol=1e-6, atol=1e-12)


def same_gains(K_ref, K_got):
    assert np.max(np.abs(K_ref - K_got) / np.maximum(1.0, np.abs(K_ref))) < 1e-8


def summary_numpy(stats):
    """the eight definitions of `summary` (include/tortoise_hip.h) from stats (T, M)"""
    out = np.zeros((stats.shape[0], 8))
    for t, s in enumerate(stats):
        ok = s["failed"] == 0
        out[t, 0], out[t, 1] = s.size, np.count_nonzero(~ok)
        if ok.any():
            out[t, 2], out[t, 3], out[t, 4] = s["slew_time"][ok].mean(), s["slew_time"][ok].min(), s["slew_time"][ok].max()
        out[t, 5], out[t, 6], out[t, 7] = s["slew_time"].mean(), s["final_angle"].max(), s["final_w_norm"].max()
    return out


def case_monte_carlo(pkg, ol, solve=None, M=100):
    """workload_monte_carlo(T=4, N=1000, seed=61), 5 x 10 budget, weights r = 0.5e3, x0_sim from default_rng(5)"""
    b = pkg.slew_setup.workload_monte_carlo(T=4, N=1000, seed=61)
    r = solve(b, (5, 10)) if solve else ol.solve_batch(b, oracle_options(ol, max_outer=5, max_inner=10, dj_counter_limit=1), nthreads=4)
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return b, r, Qd, Qfd, Rd, x0s


RAGGED_ID0 = np.array([5, 900, 2 ** 33], dtype=np.int64)


def case_ragged(pkg, ol, solve=None, M=70):
    """workload_monte_carlo(T=3, N=60, seed=77), n_knots = (60, 37, 12), 3 x 6 budget"""
    b = pkg.slew_setup.workload_monte_carlo(T=3, N=60, seed=77)
    b.n_knots = np.array((60, 37, 12), dtype=np.int32)
    r = solve(b, (3, 6)) if solve else ol.solve_batch(b, oracle_options(ol, max_outer=3, max_inner=6, dj_counter_limit=1))
    Qd, Qfd, Rd = pkg.tracking.tvlqr_weights(b.T, r=0.5e3)
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return b, r, Qd, Qfd, Rd, x0s


def horizons(batch, n=None):
    nk = np.full(batch.T, batch.N) if batch.n_knots is None else np.asarray(batch.n_knots)
    return nk if n is None else np.repeat(nk, n)


class EmuEnsemble:
    """ctypes binding of tests/emu/libtsat_emu_ensemble.so (both emulated ensemble kernels), built here by the emulator Makefile"""

    def __init__(self, abi):
        self.lib = helpers.emu_library("libtsat_emu_ensemble.so")
        self.abi = abi

    def run(self, batch, X, U, Qd, Qfd, Rd, x0_sim, K, opts, plant=None, sat=None, noise_id0=None, want_trajectories=True):
        """emu_tvlqr_ensemble, or — with ``plant`` (T, M, 21) and optionally ``sat`` = (lo, hi) — emu_tvlqr_ensemble_dispersed,
        whose result has ``n_clipped`` too"""
        T, N, M = batch.T, batch.N, x0_sim.shape[1]
        o = self.abi.TvlqrOptions.from_buffer_copy(opts)
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        X, U, Qd, Qfd, Rd, x0_sim, K = c(X), c(U), c(Qd), c(Qfd), c(Rd), c(x0_sim), c(K)
        st = np.zeros((T, M), dtype=self.abi.TVLQR_STATS_DTYPE)
        nom = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        summary = np.zeros((T, 8))
        Xs = np.full((T, M, N, 7), np.nan) if want_trajectories else None
        d = self.abi.as_dp
        id0 = None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64)
        nk = None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32)
        head = [C.byref(o), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), C.c_int32(M), d(X), d(U), d(batch.xf), d(batch.Btab),
                self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(Qd), d(Qfd), d(Rd), d(x0_sim),
                None if id0 is None else id0.ctypes.data_as(C.POINTER(C.c_int64)), self.abi.as_ip(nk)]
        tail = [d(K), st.ctypes.data_as(C.c_void_p), d(summary), nom.ctypes.data_as(C.c_void_p), d(Xs)]
        out = dict(stats=st, summary=summary, nominal=nom, X_sim=Xs)
        if plant is None:
            assert sat is None
            name, rc = "emu_tvlqr_ensemble", self.lib.emu_tvlqr_ensemble(*head, *tail)
        else:
            plant = c(plant)
            assert plant.shape == (T, M, 21)
            lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
            out["n_clipped"] = np.full((T, M), -1, dtype=np.int32)
            name, rc = "emu_tvlqr_ensemble_dispersed", self.lib.emu_tvlqr_ensemble_dispersed(*head, d(plant), d(lo), d(hi), *tail,
                                                                                               self.abi.as_ip(out["n_clipped"]))
        if rc != 0:
            raise RuntimeError(f"{name} rc={rc}")
        return out

    def summary(self, stats):
        T, M = stats.shape
        stats = np.ascontiguousarray(stats)
        out = np.zeros((T, 8))
        self.lib.emu_ensemble_summary(C.c_int64(T), C.c_int32(M), stats.ctypes.data_as(C.c_void_p), self.abi.as_dp(out))
        return out
