"""Shared pieces of tests/test_mpc_model_filtered.py (CPU tier) and tests/test_gpu_mpc_model_filtered.py (GPU tier): the held
re-planning loop BEHIND THE NINE-STATE FILTER (tsat_mpc_run_held_model_filtered).

THE REFERENCE (``reference_loop``) is ``mpc_filtered_common.reference_loop`` restated with ``model_filtered_common.ModelEkf`` — the
recursion of include/tortoise_hip.h, line for line — between ``measure`` and solver / gains: numpy and the oracle's primitives only.
Per control step s, counted FROM THE CALL, the raw sample the sensor hands over (m_s, or m_max(s-1, 0) at latency 1) meets

    latency 0:  s = 0 first(m_0);  s >= 1 predict(u_{s-1}, rows_{s-1}), update(m_s);            y_s = (w^, q^)
    latency 1:  s = 0 first(m_0);  s = 1 predict(u_0, rows_0) and no update;  s >= 2 update(m_{s-1}), predict(u_{s-1}, rows_{s-1});
                y_s = (w-, q-) for s >= 1

with u the CLIPPED command of the step before, rows the three ``dispersed_common._row(clock, t, 0, c)`` of that step's clock, and
the model inertia ``batch.Jmat[t]`` — never the plant's. With a record ``filt_init`` sample 0 makes ``update(m_0)`` on it in place of
``first``. After the last control step comes ONE MORE predict(u_{n-1}, rows_{n-1}) without an update, at either latency: the record
left is the prior for x_n. With ``filt=None`` the loop has to equal ``mpc_sensed_common.reference_loop`` with max |d| = 0
(test_mpc_model_filtered.py::test_reference_with_the_filter_off_is_the_sensed_reference).

The flat record (T, 58) is q^ 4, w^ 3, b^ 3, the command of the last predict 3, then the covariance by blocks: A (theta theta),
W (w w), D (b b) as upper triangles 00 01 02 11 12 22, X (theta w), B (theta b), Y (w b) row-major.

``VARIANT`` switches terms of the reference for the conditions of the tests (not modes of the product): ``command`` False predicts
under u = 0; ``predict`` False hands out the posterior at latency 1; ``rows`` "next" predicts across step s - 1 with the rows of step
s (the off-by-one of the clock); ``inertia`` "plant" gives the filter the dispersed plant's inertia.

Workloads, plants, limits, ids, sensor levels and bars are the sensed tests' own (mpc_sensed_common); the filter levels are
``model_filtered_common.FILT``.

Also: ``estimates`` (the ModelEkf run over ``measure`` of a returned X_hist with the returned U_hist and the clock's rows, independent
of every solve) and the ctypes binding of the emulated loop (tests/emu/tsat_emu_mpc_model_filtered.cpp, built on demand by the
emulator's pattern rule)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import model_filtered_common as mm
import mpc_filtered_common as mf6
import mpc_held_common as hc
import mpc_sensed_common as mc
import sensed_common as sc
from conftest import ROOT

FILT = mm.FILT
STATE_W, FINAL_W = 58, 12
EST_BAR = mf6.EST_BAR        # Y_hist, filt_state, filt_final: the state bar of the sensed and filtered tests (1e-9)
VARIANT = dict(command=True, predict=True, rows="flown", inertia="model")
_IU = np.triu_indices(3)


ROW_DT = 10.0                # seconds of orbit per field row in the tests' tables (``coarse_rows``)


def coarse_rows(pkg, batch, dt_row=ROW_DT):
    """the batch (in place) on a dipole table of the same orbit and row count whose rows are ``dt_row`` seconds apart. On the held
    tests' own table (0.2 s a row, one row a step) the rows of two neighbouring steps differ so little that the off-by-one of the
    clock moves the CPU case's final state by 1.4e-8 only, below ``gg_common.MOVED``; the condition stays, the table's step is the
    level that was changed."""
    B = pkg.slew_setup.dipole_btable(batch.n_tab, dt_row, 6771.0, 96.6)
    batch.Btab = np.ascontiguousarray(B[None])
    return batch


def _variant(v):
    """the ModelEkf's own switches of a VARIANT of this module"""
    return dict(mm.VARIANT, command=v["command"])


def record_of(ekf):
    """the flat record of a ``ModelEkf`` (``ekf.u``: the command of its last predict)"""
    P = ekf.P
    return np.r_[ekf.q, ekf.w, ekf.b, ekf.u, P[0:3, 0:3][_IU], P[3:6, 3:6][_IU], P[6:9, 6:9][_IU], P[0:3, 3:6].reshape(9),
                 P[0:3, 6:9].reshape(9), P[3:6, 6:9].reshape(9)]


def load_record(ekf, rec):
    rec = np.asarray(rec, dtype=np.float64)
    ekf.q, ekf.w, ekf.b, ekf.u = rec[0:4].copy(), rec[4:7].copy(), rec[7:10].copy(), rec[10:13].copy()
    A, W, D = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    A[_IU], W[_IU], D[_IU] = rec[13:19], rec[19:25], rec[25:31]
    A, W, D = mm._sym(A), mm._sym(W), mm._sym(D)
    X, B, Y = rec[31:40].reshape(3, 3), rec[40:49].reshape(3, 3), rec[49:58].reshape(3, 3)
    ekf.P = np.block([[A, X, B], [X.T, W, Y], [B.T, Y.T, D]])


def _predict(ekf, flown):
    u, rows = flown
    ekf.u = np.array(u, dtype=np.float64)
    ekf.predict(u, rows)


def _sample(ekf, s, latency, m, given, flown, predict=True):
    """sample handed over at step s of the call through the filter: y_s. ``flown`` = (u, rows) of step s - 1"""
    if s == 0:
        if given is None:
            ekf.first(m[:3], m[3:7])
            ekf.u = np.zeros(3)
        else:
            load_record(ekf, given)
            ekf.update(m[:3], m[3:7])
        return np.r_[ekf.w, ekf.q]
    if latency:
        if s > 1:
            ekf.update(m[:3], m[3:7])
        post = np.r_[ekf.w, ekf.q]
        _predict(ekf, flown)
        return np.r_[ekf.w, ekf.q] if predict else post
    _predict(ekf, flown)
    ekf.update(m[:3], m[3:7])
    return np.r_[ekf.w, ekf.q]


def _filters(ol, batch, us, filt, plant, variant):
    out = []
    for t in range(batch.T):
        J = np.asarray(batch.Jmat[t]).reshape(3, 3).T
        if variant["inertia"] == "plant":
            J = plant[t, 0:9].reshape(3, 3).T
        out.append(mm.ModelEkf(ol, batch.dt[t], J, us, filt, _variant(variant)))
    return out


def _rows(clock, t):
    return tuple(dc._row(clock, t, 0, c) for c in (0.0, 0.5, 1.0))


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, filt=None, filt_init=None, variant=VARIANT):
    """arguments and result as ``mpc_sensed_common.reference_loop`` plus ``filt`` (the seven levels, None: no filter — the sensed
    reference itself), ``filt_init`` (T, 58) or None, ``variant``; and ``filt_state`` (T, 58), ``filt_final`` (T, 12)"""
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
    ekf = None if filt is None else _filters(ol, batch, us, filt, plant, variant)
    flown = [None] * T                                                        # (limited command, field rows) of the step before
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
                    fl = flown[t]
                    if s > 0 and variant["rows"] == "next":  # the off-by-one: the rows of THIS step's clock
                        fl = (fl[0], _rows(clock, t))
                    y[t] = _sample(ekf[t], s, latency, y[t], None if filt_init is None else filt_init[t], fl, variant["predict"])
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
                b0, b1, b2r = _rows(clock, t)
                flown[t] = (np.array(u, dtype=np.float64), (b0, b1, b2r))     # what the filter's next predict crosses
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
        for t in range(T):                                   # the closing predict across the last step: the prior for x_n
            _predict(ekf[t], flown[t])
        out.update(filt_state=np.stack([record_of(e) for e in ekf]), filt_final=np.stack([e.final() for e in ekf]))
    return out


def estimates(ol, batch, us, filt, handed, U_hist, latency, filt_init=None):
    """the ``ModelEkf`` run over the samples ``handed`` (T, n, 7) as the sensor hands them over (``mpc_sensed_common.measured`` of a
    returned X_hist: with the latency shift), with the returned U_hist (T, n, 3) and the rows of the batch's clock advanced by one
    rounded addition per step, the closing predict included: (Y (T, n, 7), filt_state (T, 58), filt_final (T, 12)). No solve, no
    plant."""
    T, n = handed.shape[:2]
    Y, S, F = np.zeros((T, n, 7)), np.zeros((T, STATE_W)), np.zeros((T, FINAL_W))
    ekf = _filters(ol, batch, float(us), filt, None, VARIANT)
    tau = batch.tau0.copy()
    flown = [None] * T
    for s in range(n):
        clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
        for t in range(T):
            Y[t, s] = _sample(ekf[t], s, latency, handed[t, s], None if filt_init is None else filt_init[t], flown[t])
            flown[t] = (U_hist[t, s], _rows(clock, t))
        tau = tau + batch.dtau
    for t in range(T):
        _predict(ekf[t], flown[t])
        S[t], F[t] = record_of(ekf[t]), ekf[t].final()
    return Y, S, F


def conditions(ref_of, label, batch, po, six=None, skip=()):
    """the conditions of a parity case on references alone. ``ref_of(**over)`` is the reference of the test's call with the named
    arguments (filt, latency, variant) replaced; ``six()`` the six-state reference (``mpc_filtered_common.reference_loop``) of the
    same call, or None. The call itself meets ``mpc_held_common.condition``; each of the seven terms moves the final state by at
    least ``gg_common.MOVED``. Every figure is printed. ``skip`` names the labels a case leaves to the cases on which they show
    (``model_filtered_common.conditions`` has the same device). Returns the reference of the call itself."""
    ref = ref_of()
    hc.condition(ref, batch, po, label)
    lat1 = lambda: ref_of(latency=1)
    terms = [(ON_OFF, ref, lambda: ref_of(filt=None))]
    if six is not None:
        terms.append((SIX, ref, six))
    terms += [(COMMAND, ref, lambda: ref_of(variant=dict(VARIANT, command=False))),
              (ROWS, ref, lambda: ref_of(variant=dict(VARIANT, rows="next"))),
              (INERTIA, ref, lambda: ref_of(variant=dict(VARIANT, inertia="plant"))),
              (LATENCY, lat1, lambda: ref_of(latency=0)),
              (DELAY, lat1, lambda: ref_of(latency=1, variant=dict(VARIANT, predict=False)))]
    short = []
    for name, a, other in terms:
        a = a() if callable(a) else a
        d = float(np.max(np.abs(a["X_hist"][:, -1] - other()["X_hist"][:, -1])))
        print(f"{label}: {name}: moves the reference's final state by {d:.2e}" + ("  (left to the cases that show it)" if name in skip else ""))
        if name not in skip and not d >= gc.MOVED:
            short.append(f"{name} moves the final state by {d:.2e} only")
    assert not short, short
    return ref


ON_OFF = "filter on against off"
SIX = "this filter against the six-state one"
COMMAND = "the command in predict against u = 0"
ROWS = "the rows of step s - 1 against the rows of step s"
INERTIA = "the model inertia against the plant's inside the filter"
LATENCY = "latency 1 against 0"
DELAY = "the prediction across the delay against the posterior"


def same_estimates(ref, got, keys=("Y_hist", "filt_state", "filt_final")):
    for k in keys:
        d = float(np.max(np.abs(ref[k] - got[k])))
        print(f"max|d{k}| {d:.2e}")
        assert d < EST_BAR, k


class EmuMpcModelFiltered:
    """ctypes binding of tests/emu/libtsat_emu_mpc_model_filtered.so, built here by the emulator's pattern rule"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_model_filtered.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_model_filtered.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, sens=None, bias=None, latency=0, plant=None, sat=None, noise_id=None,
            step0=0, Rtab=None, gm=0.0, filt=FILT, filt_init=None):
        """emu_mpc_held_model_filtered_batch; the result of ``mpc_sensed_common.EmuMpcSensed.run`` plus filt_state (T, 58) and
        filt_final (T, 12), both None with ``filt`` None (f = NULL)"""
        T, N = batch.T, batch.N
        o = opts.copy()
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        plant, Rtab, bias, filt_init = c(plant), c(Rtab), c(bias), c(filt_init)
        so = sc.sensor_options(self.abi, mc.IDEAL if sens is None else sens, latency)
        fo = None if filt is None else mm.filter_options(self.abi, filt)
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
        Xh = np.zeros((T, n_steps + 1, 7)); Uh = np.zeros((T, n_steps, 3)); Yh = np.full((T, n_steps, 7), np.nan)
        X = np.zeros((T, N, 7)); U = np.zeros((T, N - 1, 3)); x0a = np.zeros((T, 7))
        fs = None if fo is None else np.full((T, STATE_W), np.nan)
        ff = None if fo is None else np.full((T, FINAL_W), np.nan)
        st = np.zeros(T, dtype=self.abi.STATS_DTYPE)
        ts = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        ncl = np.full(T, -1, dtype=np.int32)
        d = self.abi.as_dp
        rc = self.lib.emu_mpc_held_model_filtered_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every),
            C.c_int32(feedback), d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)), d(Rtab),
            C.c_double(gm), C.byref(so), d(bias), d(Yh), None if fo is None else C.byref(fo), d(filt_init), d(fs), d(ff), d(x0a))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_model_filtered_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, Y_hist=Yh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl, x0_after=x0a, filt_state=fs,
                    filt_final=ff)

    def check(self, fo, filt_init, T, filt_state=None, filt_final=None):
        """check_mpc_model_filtered on the arguments tsat_mpc_run_held_model_filtered adds"""
        text = C.create_string_buffer(256)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rc = self.lib.emu_mpc_model_filtered_check(None if fo is None else C.byref(fo), self.abi.as_dp(c(filt_init)),
                                                   self.abi.as_dp(c(filt_state)), self.abi.as_dp(c(filt_final)), C.c_int64(T), text,
                                                   C.c_int32(256))
        return rc, text.value.decode()
