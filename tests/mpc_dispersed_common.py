"""Shared pieces of tests/test_mpc_dispersed.py (CPU tier) and tests/test_gpu_mpc_dispersed.py (GPU tier).

THE REFERENCE of the receding-horizon loop on a dispersed plant (tsat_mpc_run_dispersed) is a Python loop built control step by
control step (``reference_rollout.held_loop`` re-planning at every step) from the unchanged oracle's primitives only, in the manner
of tests/dispersed_common.py: ``ol.solve_batch`` with the advanced x0, tau0 and warm start; the clip of U[0]; ``ol.plant_noise``, the
noise injection and the row lookup of ``dispersed_common``; ``ol.dyn7`` on Jp per RK4 stage with dipole G u_sat + m_res / u_scale; the plan shifted by one knot
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
    """the loop for the whole batch: ``reference_rollout.held_loop`` re-planning at every step (no gains are asked of the solver).
    plant (T, 21) or None (the model's), sat = (lo, hi) broadcastable to (T, 3) or None, noise_id (T,) or None (= t);
    noise_fn(t, knot, stage) -> nine values replaces ``ol.plant_noise`` as the source of the draws.
    Returns dict(X_hist, U_hist, stats, X, U of the last solve, tracking_stats, n_sure, n_maybe)."""
    import reference_rollout as rr          # here: that module is built on this one's parents
    r = rr.held_loop(ol, batch, opts, n_steps, 1, 0, po, plant=plant, sat=sat, noise_id=noise_id, step0=step0, nthreads=nthreads,
                     want_K=False, noise_fn=noise_fn)
    return {k: r[k] for k in ("X_hist", "U_hist", "stats", "X", "U", "tracking_stats", "n_sure", "n_maybe")}


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
