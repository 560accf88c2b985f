"""Shared pieces of tests/test_mpc_dispersed.py (CPU tier) and tests/test_gpu_mpc_dispersed.py (GPU tier).

THE REFERENCE of the receding-horizon loop on a dispersed plant (tsat_mpc_run_dispersed) is a Python loop built here, control
step by control step, from the unchanged oracle's primitives only, in the manner of tests/dispersed_common.py: ``ol.solve_batch``
with the advanced x0, tau0 and warm start; the clip of U[0]; ``ol.plant_noise``, the noise injection and the row lookup of
``dispersed_common``; ``ol.dyn7(..., Jp)`` per RK4 stage with dipole G u_sat + m_res / u_scale; the plan shifted by one knot
inside the trajectory's own horizon; ``dispersed_common.stats_of`` on the history. With the model's plant, no noise and no limits
it has to reproduce ``ol.mpc_batch`` (test_mpc_dispersed.py::test_reference_is_pinned_to_the_oracle_loop).

Also: the workload of tests/test_mpc.py, the bars (the project's MPC bars, the bracket on the clipped-step counter, the statistic
where the reference is off a threshold), and the ctypes binding of the emulated loop (tests/emu/tsat_emu_mpc_dispersed.cpp,
built on demand by its own make fragment)."""
import ctypes as C
import os
import subprocess

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
from conftest import ROOT, oracle_options

MARGIN, CLIP_BAND, LEVELS = dc.MARGIN, dc.CLIP_BAND, dc.LEVELS
SEED = ec.SEED
SAT = (np.full(3, -0.6), np.full(3, 0.6))       # far inside the workload's +-19 box: the early steps all clip, decided far from the band


def mpc_batch(pkg, T=2, N=20, seed=41, rows=200):
    """the workload of tests/test_mpc.py: Monte-Carlo slews on one dipole table, one row per knot"""
    ss = pkg.slew_setup
    b = ss.workload_monte_carlo(T=T, N=N, seed=seed)
    B = ss.dipole_btable(rows, 0.2, 6771.0, 96.6)
    b.Btab, b.n_tab = np.ascontiguousarray(B[None]), rows
    b.dtau[:] = 1.0
    return b


def solve_options(ol, **kw):
    """budget 1 x 3, dj_counter_limit = 1, as tests/test_mpc.py"""
    return oracle_options(ol, max_outer=1, max_inner=3, dj_counter_limit=1, **kw)


def noise_options(ol, noise=True, seed=SEED, **kw):
    o = ol.tvlqr_default_options()
    o.noise_mode, o.noise_seed = (1, seed) if noise else (0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def plants(pkg, batch, M=None, rng_seed=7):
    """all five dispersions at LEVELS: (T, 21), or (T, M, 21) with M"""
    p = pkg.tracking.disperse_plant(batch.Jmat, M or 1, np.random.default_rng(rng_seed), **LEVELS)
    return p if M else np.ascontiguousarray(p[:, 0])


def reference_loop(ol, batch, opts, n_steps, po, plant=None, sat=None, noise_id=None, step0=0, nthreads=4, noise_fn=None):
    """the loop for the whole batch. plant (T, 21) or None (the model's), sat = (lo, hi) broadcastable to (T, 3) or None,
    noise_id (T,) or None (= t); noise_fn(t, knot, stage) -> nine values replaces ``ol.plant_noise`` as the source of the draws.
    Returns dict(X_hist, U_hist, stats, X, U of the last solve, tracking_stats, n_sure, n_maybe)."""
    T = batch.T
    nk = ec.horizons(batch)
    us = float(opts.u_scale)
    noisy = int(po.noise_mode) == 1
    ids = np.arange(T, dtype=np.int64) if noise_id is None else np.asarray(noise_id, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    x, U0, tau = batch.x0.copy(), batch.U0.copy(), batch.tau0.copy()
    Xh, Uh = np.zeros((T, n_steps + 1, 7)), np.zeros((T, n_steps, 3))
    n_sure, n_maybe = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    ol.load()
    for s in range(n_steps):
        b2 = batch.slice(0, T)
        b2.x0, b2.U0, b2.tau0 = np.ascontiguousarray(x), np.ascontiguousarray(U0), np.ascontiguousarray(tau)
        r = ol.solve_batch(b2, opts, nthreads=min(nthreads, ol.num_procs()), want_K=False)
        Xh[:, s] = x
        for t in range(T):
            if plant is None:
                Jp, G, mres = np.asarray(batch.Jmat[t]).reshape(3, 3).T, np.eye(3), np.zeros(3)
            else:
                Jp, G, mres = plant[t, 0:9].reshape(3, 3).T, plant[t, 9:18].reshape(3, 3).T, plant[t, 18:21]
            u = r["U"][t, 0].copy()
            if lo is not None:
                bl, bh = CLIP_BAND * np.abs(lo[t]), CLIP_BAND * np.abs(hi[t])
                n_sure[t] += bool(np.any((lo[t] - u > bl) | (u - hi[t] > bh)))
                n_maybe[t] += bool(np.any((lo[t] - u > -bl) | (u - hi[t] > -bh)))
                u = np.minimum(np.maximum(u, lo[t]), hi[t])
            Uh[t, s] = u
            ua = G @ u + mres / us
            draw = noise_fn or (lambda t_, k_, st_: ol.plant_noise(int(po.noise_seed), int(ids[t_]), k_, st_, po.sigma_gyro,
                                                                    po.sigma_att, po.field_amp))
            nz = [draw(t, int(step0) + s, st) if noisy else None for st in range(4)]
            b0, b1, b2r = dc._row(b2, t, 0, 0.0), dc._row(b2, t, 0, 0.5), dc._row(b2, t, 0, 1.0)
            h = float(batch.dt[t])

            def f(xx, bb, n):
                xn, bn = dc._noisy(ol, xx, bb, n)
                return h * ol.dyn7(xn, ua, bn, Jp, us)

            k1 = f(x[t], b0, nz[0])
            k2 = f(x[t] + k1 / 2, b1, nz[1])
            k3 = f(x[t] + k2 / 2, b1, nz[2])
            k4 = f(x[t] + k3, b2r, nz[3])
            x[t] = x[t] + (k1 + 2 * k2 + 2 * k3 + k4) / 6
            n = int(nk[t])                                   # the shift inside the trajectory's own horizon, last control repeated
            U0[t, :n - 1] = np.concatenate([r["U"][t, 1:n - 1], r["U"][t, n - 2:n - 1]], axis=0)
        tau = tau + batch.dtau
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    return dict(X_hist=Xh, U_hist=Uh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe)


def margins(ref, batch, po):
    """per trajectory: how far the nearest judged sample of the reference history is from a threshold of the statistic"""
    X = ref["X_hist"]
    n = np.full(1, X.shape[1])
    return np.array([ec.margin(X[t:t + 1], batch.xf[t:t + 1], n, po.min_steps, po.w_tol, po.angle_tol) for t in range(X.shape[0])])


def same(ref, got, batch, po, clipped=True, plan=False):
    """the project's MPC bars (tests/test_mpc.py::_same) + the bracket on the clipped-step counter + the statistic wherever the
    reference is more than MARGIN from a threshold. Prints every figure before it asserts; returns the margin mask."""
    dX = float(np.max(np.abs(ref["X_hist"] - got["X_hist"])))
    dU = float(np.max(np.abs(ref["U_hist"] - got["U_hist"])))
    print(f"max|dX_hist| {dX:.2e}  max|dU_hist| {dU:.2e}")
    assert dX < 1e-9
    assert dU < 1e-8
    for k in ("inner_iters", "ls_trials", "status"):
        assert np.array_equal(ref["stats"][k], got["stats"][k]), k
    if plan:
        assert np.max(np.abs(ref["X"] - got["X"])) < 1e-9 and np.max(np.abs(ref["U"] - got["U"])) < 1e-8
    if clipped:
        n = got["n_clipped"]
        print(f"clipped steps: sure {ref['n_sure']}, got {n}, maybe {ref['n_maybe']}")
        assert np.all(ref["n_sure"] <= n) and np.all(n <= ref["n_maybe"])
    ok = margins(ref, batch, po) > MARGIN
    rs, gs = ref["tracking_stats"], got["tracking_stats"]
    print(f"statistic: {int(np.count_nonzero(ok))} of {ok.size} off the thresholds, arrivals {int(np.count_nonzero(rs['failed'] == 0))}, "
          f"slew_index ref {rs['slew_index']} got {gs['slew_index']}")
    for k in ("slew_index", "failed", "slew_time"):
        assert np.array_equal(rs[k][ok], gs[k][ok]), k
    np.testing.assert_allclose(gs["final_angle"], rs["final_angle"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(gs["final_w_norm"], rs["final_w_norm"], rtol=1e-6, atol=1e-12)
    return ok


class EmuMpcDispersed:
    """ctypes binding of tests/emu/libtsat_emu_mpc_dispersed.so, built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_dispersed.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_dispersed.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, plant=None, sat=None, noise_id=None, step0=0):
        T, N = batch.T, batch.N
        o = opts.copy()
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        plant = c(plant)
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
        Xh = np.zeros((T, n_steps + 1, 7)); Uh = np.zeros((T, n_steps, 3))
        X = np.zeros((T, N, 7)); U = np.zeros((T, N - 1, 3))
        st = np.zeros(T, dtype=self.abi.STATS_DTYPE)
        ts = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        ncl = np.full(T, -1, dtype=np.int32)
        d = self.abi.as_dp
        rc = self.lib.emu_mpc_dispersed_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), d(plant), d(lo), d(hi),
            None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh), st.ctypes.data_as(C.c_void_p),
            ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_dispersed_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl)
