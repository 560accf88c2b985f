"""Shared pieces of tests/test_mpc_filtered.py (CPU tier) and tests/test_gpu_mpc_filtered.py (GPU tier): the held re-planning loop
BEHIND THE FILTER (tsat_mpc_run_held_filtered).

THE REFERENCE (``reference_loop``) is ``mpc_sensed_common.reference_loop`` restated with ``filtered_common.Ekf`` — the recursion of
include/tortoise_hip.h, line for line — between ``measure`` and solver / gains: numpy and the oracle's primitives only. Per control
step s, counted FROM THE CALL: the raw sample the sensor hands over (m_s, or m_max(s-1, 0) at latency 1) makes ``first`` at s = 0 (a
``step`` when a record ``filt_init`` is given), no step at s = 1 of latency 1 (m_0 handed over a second time), a ``step`` otherwise;
the solver's x0, the gains' state and Y_hist read (w^, q^), with q^ predicted across the delay for s >= 1 at latency 1. With
``filt=None`` it has to equal ``mpc_sensed_common.reference_loop`` with max |d| = 0
(test_mpc_filtered.py::test_reference_with_the_filter_off_is_the_sensed_reference).

The flat record (T, 31) is q^ 4, b^ 3, w^ 3, A 6, B 9, D 6 — A and D as upper triangles 00 01 02 11 12 22, B row-major.

Workloads, plants, limits, ids, sensor levels and bars are the sensed tests' own (mpc_sensed_common); the filter levels are
``filtered_common.FILT``.

Also: ``estimates`` (the Ekf run over given raw samples, independent of every solve) and the ctypes binding of the emulated loop
(tests/emu/tsat_emu_mpc_filtered.cpp, built on demand by the emulator's pattern rule)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import filtered_common as fc
import gg_common as gc
import mpc_held_common as hc
import mpc_sensed_common as mc
import sensed_common as sc
from conftest import ROOT

FILT = fc.FILT
STATE_W = 31
EST_BAR = 1e-9               # Y_hist, filt_state, filt_final: the state bar of the sensed and filtered tests
_IU = np.triu_indices(3)


def record_of(ekf):
    """the flat record of an ``Ekf``"""
    return np.r_[ekf.q, ekf.b, ekf.w, ekf.A[_IU], ekf.B.reshape(9), ekf.D[_IU]]


def load_record(ekf, rec):
    ekf.q, ekf.b, ekf.w = np.array(rec[0:4]), np.array(rec[4:7]), np.array(rec[7:10])
    ekf.A, ekf.D = np.zeros((3, 3)), np.zeros((3, 3))
    ekf.A[_IU], ekf.D[_IU] = rec[10:16], rec[25:31]
    ekf.A, ekf.D = fc._sym(ekf.A), fc._sym(ekf.D)
    ekf.B = np.array(rec[16:25]).reshape(3, 3)


def _sample(ekf, s, latency, m, given, predict=True):
    """sample handed over at step s of the call through the filter: y_s"""
    if s == 0:
        if given is None:
            ekf.first(m[:3], m[3:7])
        else:
            load_record(ekf, given)
            ekf.step(m[:3], m[3:7])
    elif not (latency and s == 1):
        ekf.step(m[:3], m[3:7])
    return np.r_[ekf.w, ekf.predicted() if (latency and s > 0 and predict) else ekf.q]


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, filt=None, filt_init=None, predict=True):
    """arguments and result as ``mpc_sensed_common.reference_loop`` plus ``filt`` (the five levels, None: no filter — the sensed
    reference itself), ``filt_init`` (T, 31) or None, ``predict`` (False leaves the prediction across the delay out: a condition of
    the tests, not a mode of the product); and ``filt_state`` (T, 31), ``filt_final`` (T, 9)"""
    T, R = batch.T, int(replan_every)
    sens = mc.IDEAL if sens is None else sens
    nk = ec.horizons(batch)
    us = float(opts.u_scale)
    es = int(opts.error_state)
    nh = 6 if es else 7
    noisy = int(po.noise_mode) == 1
    ids = np.arange(T, dtype=np.int64) if noise_id is None else np.asarray(noise_id, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    x, U0, tau = batch.x0.copy(), batch.U0.copy(), batch.tau0.copy()          # x: the TRUE state
    y, held = np.zeros((T, 7)), [None] * T                                    # y: what the solver and the gains are given
    ekf = None if filt is None else [fc.Ekf(ol, batch.dt[t], filt) for t in range(T)]
    Xh, Uh, Yh = np.zeros((T, n_steps + 1, 7)), np.zeros((T, n_steps, 3)), np.zeros((T, n_steps, 7))
    n_sure, n_maybe = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    statuses, tally = [], np.zeros((T, 4), dtype=np.int64)
    ol.load()
    for sb in range(0, n_steps, R):
        r_len = min(R, n_steps - sb)
        for j in range(r_len):
            s = sb + j
            clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
            for t in range(T):                               # the sample handed over: m_s, or m_max(s-1, 0); s counts from the call
                w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, x[t], po, ids[t], sens, None if bias is None else bias[t], noisy)
                m = np.r_[w_m, q_m]
                y[t] = held[t] if (latency and s > 0) else m
                held[t] = m
                if ekf is not None:                          # the filter between the sample and everything that reads y
                    y[t] = _sample(ekf[t], s, latency, y[t], None if filt_init is None else filt_init[t], predict)
            if j == 0:                                       # the block's solve starts from the estimate
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
    out = dict(X_hist=Xh, U_hist=Uh, Y_hist=Yh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
               n_solves=len(statuses), statuses=np.array(statuses), tally=tally)
    if ekf is not None:
        out.update(filt_state=np.stack([record_of(e) for e in ekf]), filt_final=np.stack([e.final() for e in ekf]))
    return out


def estimates(ol, batch, filt, handed, latency, filt_init=None):
    """the ``Ekf`` run over the samples ``handed`` (T, n, 7) as the sensor hands them over (``mpc_sensed_common.measured``: with the
    latency shift): (Y (T, n, 7), filt_state (T, 31), filt_final (T, 9)). No solve, no plant."""
    T, n = handed.shape[:2]
    Y, S, F = np.zeros((T, n, 7)), np.zeros((T, STATE_W)), np.zeros((T, 9))
    for t in range(T):
        e = fc.Ekf(ol, batch.dt[t], filt)
        for s in range(n):
            Y[t, s] = _sample(e, s, latency, handed[t, s], None if filt_init is None else filt_init[t])
        S[t], F[t] = record_of(e), e.final()
    return Y, S, F


def conditions(ref_of, bias, label, batch, po):
    """the conditions of a case on references alone. ``ref_of(**over)`` is the reference of the test's call with the named arguments
    (filt, bias, latency, predict) replaced. The call itself meets ``mpc_held_common.condition``; the filter on against off, the gyro
    bias, latency 1 against 0 and the prediction across the delay against the unpredicted estimate each move the final state by at
    least ``gg_common.MOVED``. Returns the reference of the call itself."""
    ref = ref_of()
    hc.condition(ref, batch, po, label)
    mc.moved(ref, ref_of(filt=None), f"{label}: filter on against off")
    z = bias.copy()
    z[..., 0:3] = 0.0
    mc.moved(ref, ref_of(bias=z), f"{label}: gyro bias on against zero")
    mc.moved(ref_of(latency=1), ref_of(latency=0), f"{label}: latency 1 against 0")
    mc.moved(ref_of(latency=1), ref_of(latency=1, predict=False), f"{label}: prediction across the delay on against off")
    return ref


def same_estimates(ref, got, keys=("Y_hist", "filt_state", "filt_final")):
    for k in keys:
        d = float(np.max(np.abs(ref[k] - got[k])))
        print(f"max|d{k}| {d:.2e}")
        assert d < EST_BAR, k


class EmuMpcFiltered:
    """ctypes binding of tests/emu/libtsat_emu_mpc_filtered.so, built here by the emulator's pattern rule"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_filtered.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_filtered.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, sens=None, bias=None, latency=0, plant=None, sat=None, noise_id=None,
            step0=0, Rtab=None, gm=0.0, filt=FILT, filt_init=None):
        """emu_mpc_held_filtered_batch; the result of ``mpc_sensed_common.EmuMpcSensed.run`` plus filt_state (T, 31) and filt_final
        (T, 9), both None with ``filt`` None (f = NULL)"""
        T, N = batch.T, batch.N
        o = opts.copy()
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        plant, Rtab, bias, filt_init = c(plant), c(Rtab), c(bias), c(filt_init)
        so = sc.sensor_options(self.abi, mc.IDEAL if sens is None else sens, latency)
        fo = None if filt is None else fc.filter_options(self.abi, filt)
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
        Xh = np.zeros((T, n_steps + 1, 7)); Uh = np.zeros((T, n_steps, 3)); Yh = np.full((T, n_steps, 7), np.nan)
        X = np.zeros((T, N, 7)); U = np.zeros((T, N - 1, 3)); x0a = np.zeros((T, 7))
        fs = None if fo is None else np.full((T, STATE_W), np.nan)
        ff = None if fo is None else np.full((T, 9), np.nan)
        st = np.zeros(T, dtype=self.abi.STATS_DTYPE)
        ts = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        ncl = np.full(T, -1, dtype=np.int32)
        d = self.abi.as_dp
        rc = self.lib.emu_mpc_held_filtered_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every),
            C.c_int32(feedback), d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)), d(Rtab),
            C.c_double(gm), C.byref(so), d(bias), d(Yh), None if fo is None else C.byref(fo), d(filt_init), d(fs), d(ff), d(x0a))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_filtered_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, Y_hist=Yh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl, x0_after=x0a, filt_state=fs,
                    filt_final=ff)

    def check(self, fo, filt_init, T, filt_state=None, filt_final=None):
        """check_mpc_filtered on the arguments tsat_mpc_run_held_filtered adds"""
        text = C.create_string_buffer(256)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rc = self.lib.emu_mpc_filtered_check(None if fo is None else C.byref(fo), self.abi.as_dp(c(filt_init)), self.abi.as_dp(c(filt_state)),
                                             self.abi.as_dp(c(filt_final)), C.c_int64(T), text, C.c_int32(256))
        return rc, text.value.decode()
