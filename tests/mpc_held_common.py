"""Shared pieces of tests/test_mpc_held.py (CPU tier) and tests/test_gpu_mpc_held.py (GPU tier).

THE REFERENCE of the loop that re-plans every R control steps (tsat_mpc_run_held) is a Python loop over blocks built here from the
unchanged oracle's primitives only. It extends ``mpc_dispersed_common.reference_loop`` by: ``ol.solve_batch(..., want_K=True)`` once
per block; the command rule of include/tortoise_hip.h (U_0 at j = 0; U_j + K_j dx at j > 0 with ``feedback``, the sum started from
U_j with the columns ascending, dx = x - X_j or ``ol.quaternion_error(x, X_j)``; U_j without); ``tau += dtau`` once per step, the
rows of a step looked up at knot 0 of that clock; the plan shifted by the block's r knots inside the trajectory's own horizon. At
R = 1 it has to reproduce ``mpc_dispersed_common.reference_loop`` (test_mpc_held.py::test_reference_at_r1_is_the_every_step_reference).

The bars (``same``), the workload, the plants, the limits, the noise options and the margins are those of mpc_dispersed_common."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
from conftest import ROOT
from mpc_dispersed_common import CLIP_BAND, MARGIN, SAT, margins, mpc_batch, noise_options, plants, same, solve_options  # noqa: F401

# the statistic and the generator ids of the three cases of test_gpu_mpc_held.py (those of tests/test_gpu_mpc_dispersed.py)
W_TOL, ANGLE_TOL, MIN_STEPS = 1.25e-4, 3.0, 3
IDS = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
WIDE = (np.full(3, -25.0), np.full(3, 25.0))     # limits no command of the workload reaches (max |U_hist| 20.4)
RAGGED = np.array([20, 13, 6, 7, 20, 19, 6, 20], dtype=np.int32)
TSAT_MAX_OUTER = 1          # tsat_status: 0 converged, 1 outer budget exhausted; 2 REG_FAIL and 3 DIVERGED leave K undefined


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, plant=None, sat=None, noise_id=None, step0=0, nthreads=4):
    """the loop for the whole batch; arguments and result as ``mpc_dispersed_common.reference_loop`` plus ``n_solves``,
    ``statuses`` (n_solves, T), the status of every block solve, and ``tally`` (T, 4), the sums of tsat_mpc_tally over the solves (column 1,
    n_forward, counts the ORACLE's roll-outs: a backend's own count, not comparable across backends)"""
    T, R = batch.T, int(replan_every)
    nk = ec.horizons(batch)
    us = float(opts.u_scale)
    es = int(opts.error_state)
    nh = 6 if es else 7
    noisy = int(po.noise_mode) == 1
    ids = np.arange(T, dtype=np.int64) if noise_id is None else np.asarray(noise_id, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    x, U0, tau = batch.x0.copy(), batch.U0.copy(), batch.tau0.copy()
    Xh, Uh = np.zeros((T, n_steps + 1, 7)), np.zeros((T, n_steps, 3))
    n_sure, n_maybe = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    statuses, tally = [], np.zeros((T, 4), dtype=np.int64)    # tally: the sums tsat_mpc_tally holds after the call
    ol.load()
    for sb in range(0, n_steps, R):
        r_len = min(R, n_steps - sb)
        b2 = batch.slice(0, T)
        b2.x0, b2.U0, b2.tau0 = np.ascontiguousarray(x), np.ascontiguousarray(U0), np.ascontiguousarray(tau)
        r = ol.solve_batch(b2, opts, nthreads=min(nthreads, ol.num_procs()), want_K=True)
        statuses.append(r["stats"]["status"].copy())
        rs = r["stats"]
        tally += np.stack([rs["n_backward"], rs["n_forward"], np.maximum(rs["outer_iters"] - 1, 0), rs["inner_iters"]], axis=1)
        for j in range(r_len):
            s = sb + j
            Xh[:, s] = x
            clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
            for t in range(T):
                if plant is None:
                    Jp, G, mres = np.asarray(batch.Jmat[t]).reshape(3, 3).T, np.eye(3), np.zeros(3)
                else:
                    Jp, G, mres = plant[t, 0:9].reshape(3, 3).T, plant[t, 9:18].reshape(3, 3).T, plant[t, 18:21]
                u = r["U"][t, j].copy()
                if j > 0 and feedback:
                    dx = ol.quaternion_error(x[t], r["X"][t, j]) if es else x[t] - r["X"][t, j]
                    for a in range(3):
                        v = float(u[a])
                        for i in range(nh):
                            v += float(r["K"][t, j, i, a]) * float(dx[i])
                        u[a] = v
                if lo is not None:
                    bl, bh = CLIP_BAND * np.abs(lo[t]), CLIP_BAND * np.abs(hi[t])
                    n_sure[t] += bool(np.any((lo[t] - u > bl) | (u - hi[t] > bh)))
                    n_maybe[t] += bool(np.any((lo[t] - u > -bl) | (u - hi[t] > -bh)))
                    u = np.minimum(np.maximum(u, lo[t]), hi[t])
                Uh[t, s] = u
                ua = G @ u + mres / us
                nz = [ol.plant_noise(int(po.noise_seed), int(ids[t]), int(step0) + s, st, po.sigma_gyro, po.sigma_att, po.field_amp)
                      if noisy else None for st in range(4)]
                b0, b1, b2r = dc._row(clock, t, 0, 0.0), dc._row(clock, t, 0, 0.5), dc._row(clock, t, 0, 1.0)
                h = float(batch.dt[t])

                def f(xx, bb, n):
                    xn, bn = dc._noisy(ol, xx, bb, n)
                    return h * ol.dyn7(xn, ua, bn, Jp, us)

                k1 = f(x[t], b0, nz[0])
                k2 = f(x[t] + k1 / 2, b1, nz[1])
                k3 = f(x[t] + k2 / 2, b1, nz[2])
                k4 = f(x[t] + k3, b2r, nz[3])
                x[t] = x[t] + (k1 + 2 * k2 + 2 * k3 + k4) / 6
            tau = tau + batch.dtau                           # one rounded addition per step
        for t in range(T):                                   # the shift by the block's steps inside the trajectory's own horizon
            n = int(nk[t])
            U0[t, :n - 1] = r["U"][t, np.minimum(np.arange(n - 1) + r_len, n - 2)]
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    return dict(X_hist=Xh, U_hist=Uh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
                n_solves=len(statuses), statuses=np.array(statuses), tally=tally)


def condition(ref, batch, po, label):
    """what a case has to show on the reference alone before a kernel result is looked at: every trajectory off the statistic's
    thresholds, arrivals and failures both present, no block solve ended in a failure status"""
    m = margins(ref, batch, po)
    failed = ref["tracking_stats"]["failed"]
    print(f"{label} reference: smallest margin {m.min():.2e}, failed {failed}, statuses up to {int(ref['statuses'].max())}")
    assert np.all(m > MARGIN), "a trajectory of the case sits on a threshold"
    assert 0 < np.count_nonzero(failed) < failed.size, "the reference must have both arrivals and failures"
    assert np.all(ref["statuses"] <= TSAT_MAX_OUTER), "a block solve ended REG_FAIL or DIVERGED: its gains are undefined"


class EmuMpcHeld:
    """ctypes binding of tests/emu/libtsat_emu_mpc_held.so, built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_held.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_held.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, plant=None, sat=None, noise_id=None, step0=0):
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
        rc = self.lib.emu_mpc_held_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every),
            C.c_int32(feedback), d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl)

    def check(self, replan_every, feedback, min_nk):
        text = C.create_string_buffer(256)
        rc = self.lib.emu_mpc_held_check(C.c_int32(replan_every), C.c_int32(feedback), C.c_int32(min_nk), text, C.c_int32(256))
        return rc, text.value.decode()
