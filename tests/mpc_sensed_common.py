"""Shared pieces of tests/test_mpc_sensed.py (CPU tier) and tests/test_gpu_mpc_sensed.py (GPU tier): the held re-planning loop FED
MEASUREMENTS (tsat_mpc_run_held_sensed).

THE REFERENCE is ``mpc_held_common.reference_loop`` with three things inserted, built from the oracle's primitives only:
``sensed_common.measure`` (its w_m and q_m; the field measurement it also returns is dropped: the loop has no law that reads it),
the latency rule (y_s = m_s, or m_max(s-1, 0) with s counted FROM THE CALL), and the separation of the true state — which the
plant advances, the statistic judges and X_hist records — from the state the solver is given: each block's solve starts from
y_{s_b} and the held steps' gain product is evaluated on y_s. With an orbit table every stage also gets ``gg_common.gg_increment``,
as ``gg_common.held_loop`` adds it. With the ideal sensor it has to equal its parents with max |d| = 0
(test_mpc_sensed.py::test_reference_with_the_ideal_sensor_is_the_held_reference).

Workloads, plants, limits, ids and bars are the held tests' own (mpc_held_common). The sensor levels start from
``sensed_common.SIGMAS`` / ``BIAS``. The sigmas were kept. The biases were DOUBLED, on the reference alone: under the limits +-0.6
every command of the workload clips, so the flown commands are bang-bang and a small change of the measurement moves the final
state either by a flipped component or by exactly nothing — at the ensembles' bias levels the attitude or the gyro bias left three of
the six GPU cases unmoved (0.0); at twice the level every case meets every condition (``conditions`` below; the measured figures
are in the docstrings of the two test modules).

Also: the ctypes binding of the emulated loop (tests/emu/tsat_emu_mpc_sensed.cpp, built on demand by its own make fragment)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import mpc_held_common as hc
import sensed_common as sc
from conftest import ROOT

SIGMAS, IDEAL = sc.SIGMAS, sc.IDEAL
BIAS = {k: 2.0 * v for k, v in sc.BIAS.items()}      # gyro 3e-3 rad/s, attitude 1.5 deg (magnetometer 3e-6: nothing reads it)


def biases(pkg, T, M=None):
    """(T, 9), or (T, M, 9) with M: ``tracking.disperse_sensor`` at BIAS"""
    b = pkg.tracking.disperse_sensor(T, M or 1, np.random.default_rng(11), **BIAS)
    return b if M else np.ascontiguousarray(b[:, 0])


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4):
    """arguments and result as ``mpc_held_common.reference_loop`` plus: ``sens`` the three sigmas (None = IDEAL), ``bias`` (T, 9) or
    None, ``latency``, the orbit table and gm of ``gg_common.held_loop`` (None: no term); and ``Y_hist`` (T, n_steps, 7)"""
    T, R = batch.T, int(replan_every)
    sens = IDEAL if sens is None else sens
    nk = ec.horizons(batch)
    us = float(opts.u_scale)
    es = int(opts.error_state)
    nh = 6 if es else 7
    noisy = int(po.noise_mode) == 1
    ids = np.arange(T, dtype=np.int64) if noise_id is None else np.asarray(noise_id, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    x, U0, tau = batch.x0.copy(), batch.U0.copy(), batch.tau0.copy()          # x: the TRUE state
    y, held = np.zeros((T, 7)), [None] * T                                    # y: what the solver and the gains are given
    Xh, Uh, Yh = np.zeros((T, n_steps + 1, 7)), np.zeros((T, n_steps, 3)), np.zeros((T, n_steps, 7))
    n_sure, n_maybe = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    statuses, tally = [], np.zeros((T, 4), dtype=np.int64)
    ol.load()
    for sb in range(0, n_steps, R):
        r_len = min(R, n_steps - sb)
        for j in range(r_len):
            s = sb + j
            clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
            for t in range(T):                               # y_s = m_s, or m_max(s-1, 0): s counts from the call
                w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, x[t], po, ids[t], sens, None if bias is None else bias[t], noisy)
                m = np.r_[w_m, q_m]
                y[t] = held[t] if (latency and s > 0) else m
                held[t] = m
            if j == 0:                                       # the block's solve starts from the measurement
                b2 = batch.slice(0, T)
                b2.x0, b2.U0, b2.tau0 = np.ascontiguousarray(y), np.ascontiguousarray(U0), np.ascontiguousarray(tau)
                r = ol.solve_batch(b2, opts, nthreads=min(nthreads, ol.num_procs()), want_K=True)
                statuses.append(r["stats"]["status"].copy())
                rs = r["stats"]
                tally += np.stack([rs["n_backward"], rs["n_forward"], np.maximum(rs["outer_iters"] - 1, 0), rs["inner_iters"]], axis=1)
            Xh[:, s] = x
            Yh[:, s] = y
            for t in range(T):
                if plant is None:
                    Jp, G, mres = np.asarray(batch.Jmat[t]).reshape(3, 3).T, np.eye(3), np.zeros(3)
                else:
                    Jp, G, mres = plant[t, 0:9].reshape(3, 3).T, plant[t, 9:18].reshape(3, 3).T, plant[t, 18:21]
                u = r["U"][t, j].copy()
                if j > 0 and feedback:
                    dx = ol.quaternion_error(y[t], r["X"][t, j]) if es else y[t] - r["X"][t, j]
                    for a in range(3):
                        v = float(u[a])
                        for i in range(nh):
                            v += float(r["K"][t, j, i, a]) * float(dx[i])
                        u[a] = v
                if lo is not None:
                    bl, bh = hc.CLIP_BAND * np.abs(lo[t]), hc.CLIP_BAND * np.abs(hi[t])
                    n_sure[t] += bool(np.any((lo[t] - u > bl) | (u - hi[t] > bh)))
                    n_maybe[t] += bool(np.any((lo[t] - u > -bl) | (u - hi[t] > -bh)))
                    u = np.minimum(np.maximum(u, lo[t]), hi[t])
                Uh[t, s] = u
                ua = G @ u + mres / us
                nz = [ol.plant_noise(int(po.noise_seed), int(ids[t]), int(step0) + s, st, po.sigma_gyro, po.sigma_att, po.field_amp)
                      if noisy else None for st in range(4)]
                b0, b1, b2r = dc._row(clock, t, 0, 0.0), dc._row(clock, t, 0, 0.5), dc._row(clock, t, 0, 1.0)
                rr = [None] * 3 if Rtab is None else [gc._grow(clock, Rtab, t, 0, c) for c in (0.0, 0.5, 1.0)]
                h = float(batch.dt[t])

                def f(xx, bb, n, rk):
                    xn, bn = dc._noisy(ol, xx, bb, n)
                    kk = h * ol.dyn7(xn, ua, bn, Jp, us)
                    if rk is not None:
                        kk[0:3] = kk[0:3] + gc.gg_increment(ol, xx, rk, gm, Jp, h)
                    return kk

                k1 = f(x[t], b0, nz[0], rr[0])
                k2 = f(x[t] + k1 / 2, b1, nz[1], rr[1])
                k3 = f(x[t] + k2 / 2, b1, nz[2], rr[1])
                k4 = f(x[t] + k3, b2r, nz[3], rr[2])
                x[t] = x[t] + (k1 + 2 * k2 + 2 * k3 + k4) / 6
            tau = tau + batch.dtau                           # one rounded addition per step
        for t in range(T):                                   # the shift by the block's steps inside the trajectory's own horizon
            n = int(nk[t])
            U0[t, :n - 1] = r["U"][t, np.minimum(np.arange(n - 1) + r_len, n - 2)]
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    return dict(X_hist=Xh, U_hist=Uh, Y_hist=Yh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
                n_solves=len(statuses), statuses=np.array(statuses), tally=tally)


def measured(ol, batch, po, X_hist, sens, bias, latency, noise_id, step0=0):
    """``measure`` applied to the true states X_hist (T, n + 1, 7) with the latency shift: what Y_hist (T, n, 7) has to be"""
    T, n = X_hist.shape[0], X_hist.shape[1] - 1
    noisy = int(po.noise_mode) == 1
    clock = types.SimpleNamespace(dtau=batch.dtau, tau0=batch.tau0, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
    M = np.zeros((T, n, 7))
    for t in range(T):
        for s in range(n):
            w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, X_hist[t, s], po, noise_id[t], sens, None if bias is None else bias[t], noisy)
            M[t, s] = np.r_[w_m, q_m]
    return np.concatenate([M[:, :1], M[:, :-1]], axis=1) if latency else M


def moved(a, b, label):
    """a sensor effect has to show on the references before a kernel is looked at: final states differ by >= gg_common.MOVED"""
    d = float(np.max(np.abs(a["X_hist"][:, -1] - b["X_hist"][:, -1])))
    print(f"{label}: moves the reference's final state by {d:.2e}")
    assert d >= gc.MOVED, f"{label} does not show on this case"
    return d


def conditions(ref_of, bias, label, batch, po):
    """the conditions of a case on references alone. ``ref_of(**over)`` is the reference of the test's call with the named arguments
    (sens, bias, latency) replaced. The call itself meets ``mpc_held_common.condition``; sensor noise, gyro bias, attitude bias and
    latency 1 against 0 each move the final state by at least ``gg_common.MOVED``. Returns the reference of the call itself."""
    ref = ref_of()
    hc.condition(ref, batch, po, label)
    moved(ref, ref_of(sens=IDEAL), f"{label}: sensor noise on against off")
    for name, sl in (("gyro", slice(0, 3)), ("attitude", slice(3, 6))):
        z = bias.copy()
        z[..., sl] = 0.0
        moved(ref, ref_of(bias=z), f"{label}: {name} bias on against zero")
    moved(ref_of(latency=1), ref_of(latency=0), f"{label}: latency 1 against 0")
    return ref


class EmuMpcSensed:
    """ctypes binding of tests/emu/libtsat_emu_mpc_sensed.so, built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_sensed.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_sensed.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, sens=None, bias=None, latency=0, plant=None, sat=None, noise_id=None,
            step0=0, Rtab=None, gm=0.0):
        """emu_mpc_held_sensed_batch; the result of ``mpc_held_common.EmuMpcHeld.run`` plus Y_hist and x0_after (T, 7), x0 of the
        parameter records as the call leaves them"""
        T, N = batch.T, batch.N
        o = opts.copy()
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        plant, Rtab, bias = c(plant), c(Rtab), c(bias)
        so = sc.sensor_options(self.abi, IDEAL if sens is None else sens, latency)
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
        Xh = np.zeros((T, n_steps + 1, 7)); Uh = np.zeros((T, n_steps, 3)); Yh = np.full((T, n_steps, 7), np.nan)
        X = np.zeros((T, N, 7)); U = np.zeros((T, N - 1, 3)); x0a = np.zeros((T, 7))
        st = np.zeros(T, dtype=self.abi.STATS_DTYPE)
        ts = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        ncl = np.full(T, -1, dtype=np.int32)
        d = self.abi.as_dp
        rc = self.lib.emu_mpc_held_sensed_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every),
            C.c_int32(feedback), d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)), d(Rtab),
            C.c_double(gm), C.byref(so), d(bias), d(Yh), d(x0a))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_sensed_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, Y_hist=Yh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl, x0_after=x0a)

    def check(self, so, sensor, T, Rtab=None, gm=0.0):
        """check_mpc_sensed on the arguments tsat_mpc_run_held_sensed adds"""
        text = C.create_string_buffer(256)
        sensor = None if sensor is None else np.ascontiguousarray(sensor, dtype=np.float64)
        R = None if Rtab is None else np.ascontiguousarray(Rtab, dtype=np.float64)
        rc = self.lib.emu_mpc_sensed_check(None if so is None else C.byref(so), self.abi.as_dp(sensor), C.c_int64(T), self.abi.as_dp(R),
                                           C.c_double(gm), text, C.c_int32(256))
        return rc, text.value.decode()
