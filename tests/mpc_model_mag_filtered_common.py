"""Shared pieces of tests/test_mpc_model_mag_filtered.py (CPU tier) and tests/test_gpu_mpc_model_mag_filtered.py (GPU tier): the held
re-planning loop BEHIND THE MAGNETOMETER-UPDATED NINE-STATE FILTER (tsat_mpc_run_held_model_mag_filtered).

THE REFERENCE. ``reference_rollout.held_loop`` hands its estimator ``None, None`` for the magnetometer sample and its row, and drops
the third value of ``sensed_common.measure`` — which it forms with knot ``step0 + s`` of an already advanced clock, not with the row the
plant reads. ``held_loop`` below therefore states that loop once more with the magnetometer handed over, from the existing pieces
(``rr.plant_step``, ``rr.limit``, ``rr.rows_of``, ``ol.solve_batch``, ``ol.plant_noise``, ``dc.stats_of``, ``sc.measure`` for w_m and
q_m): per control step s, counted FROM THE CALL,

    b_m,s = qrot(x_s / |x_s|, r_s) + bias_m + n_m(step0 + s),      r_s = dispersed_common._row(clock, t, 0, 0.0) of the clock at step s

on the TRUE state, n_m the gyro triple of stage 5 of generator (id, step0 + s) at sigma_mag — the draw of ``sensed_common.measure``.
At latency 1 the estimator is handed (w_m, q_m, b_m, r) of step max(s - 1, 0): a one-sample memory that restarts with the call.
It is pinned to the old references with max |d| = 0: with no estimator to ``mpc_sensed_common.reference_loop``, with the
attitude-updated ``reference_rollout.ModelState`` (which ignores b_m) to ``mpc_model_filtered_common.reference_loop``
(test_mpc_model_mag_filtered.py). Folding it into ``reference_rollout.held_loop`` is left to a change that may touch that module.

The estimator is ``model_mag_filtered_common.ModelMagEkf`` — the recursion of include/tortoise_hip.h — behind ``HeldModelMagState``:
``model_mag_filtered_common.ModelMagState``'s sequencing, resumable from a 58-value record (sample 0 then makes
update(w_m,0, b_m,0, r_0) on it) and with the parent's ``rows`` condition:

    latency 0:  s = 0 first(m_0);  s >= 1 predict(u_{s-1}, rows_{s-1}), update(w_m,s, b_m,s, r_s);              y_s = (w^, q^)
    latency 1:  s = 0 first(m_0);  s = 1 predict(u_0, rows_0) and no update;  s >= 2 update(w_m,s-1, b_m,s-1, r_{s-1}),
                predict(u_{s-1}, rows_{s-1});  y_s = (w-, q-) for s >= 1

and one closing predict after the last step. ``VARIANT`` switches terms of the reference for the conditions of the tests (not modes of
the product): the parent's ``command``, ``predict``, ``rows``, ``inertia``; ``mag`` False leaves the magnetometer update out; ``pair``
"current" pairs the delayed sample of latency 1 with r_s instead of r_{s-1}.

Workloads, plants, limits, ids, sensor levels and bars are the parent's (mpc_model_filtered_common, mpc_sensed_common); the filter
levels are ``model_mag_filtered_common.FILT``."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import model_mag_filtered_common as mg
import mpc_filtered_common as mf6
import mpc_held_common as hc
import mpc_model_filtered_common as mf
import reference_rollout as rr
import sensed_common as sc
from conftest import ROOT

FILT = mg.FILT
STATE_W, FINAL_W = mf.STATE_W, mf.FINAL_W
EST_BAR = mf.EST_BAR
VARIANT = dict(mf.VARIANT, mag=True, pair="own")
coarse_rows = mf.coarse_rows
same_estimates = mf.same_estimates


def field_sample(ol, x, row, po, gid, knot, sens, bias, noisy):
    """b_m of the true state x against the field row ``row``: the third value of ``sensed_common.measure``, with the row handed over"""
    bm = np.zeros(3) if bias is None else bias[6:9]
    n_m = ol.plant_noise(int(po.noise_seed), int(gid), int(knot), 5, sens["sigma_mag"], 0.0, 0.0)[0:3] if noisy else np.zeros(3)
    return ol.qrot(x[3:7] / math.sqrt(float(x[3:7] @ x[3:7])), row) + bm + n_m


def held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
              noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, est=None):
    """``reference_rollout.held_loop`` with the estimator handed the magnetometer: (w_m, q_m, b_m, the row b_m was formed with) of
    step s, or of step max(s - 1, 0) at ``latency`` 1. Arguments and result are that function's (``sens`` the three sigmas)."""
    T, R = batch.T, int(replan_every)
    nk = ec.horizons(batch)
    us = float(opts.u_scale)
    es = int(opts.error_state)
    nh = 6 if es else 7
    noisy = int(po.noise_mode) == 1
    ids = np.arange(T, dtype=np.int64) if noise_id is None else np.asarray(noise_id, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    x, U0, tau = batch.x0.copy(), batch.U0.copy(), batch.tau0.copy()          # x: the TRUE state
    y, held = np.zeros((T, 7)), [None] * T                                    # y: what the solver and the gains are given
    ests = [rr.Raw() if est is None else est(t) for t in range(T)]
    rows, rows_prev, u_prev = [None] * T, [None] * T, [None] * T
    Xh, Uh, Yh = np.zeros((T, n_steps + 1, 7)), np.zeros((T, n_steps, 3)), np.zeros((T, n_steps, 7))
    n_sure, n_maybe = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    statuses, tally = [], np.zeros((T, 4), dtype=np.int64)
    ol.load()
    for sb in range(0, n_steps, R):
        r_len = min(R, n_steps - sb)
        for j in range(r_len):
            s = sb + j
            clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
            for t in range(T):
                rows[t] = rr.rows_of(clock, t, 0)
                bt = None if bias is None else bias[t]
                w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, x[t], po, ids[t], sens, bt, noisy)
                b_m = field_sample(ol, x[t], rows[t][0], po, ids[t], int(step0) + s, sens, bt, noisy)
                now = (np.r_[w_m, q_m], b_m, rows[t][0])
                m, b_m, row_m = held[t] if (latency and s > 0) else now        # the sample handed over, and the row it was formed with
                held[t] = now
                y[t] = m
                w, q = ests[t].sample(s, latency, m[:3], m[3:7], b_m, row_m, rows[t], rows_prev[t], u_prev[t])
                if ests[t].estimates:
                    y[t] = np.r_[w, q]
            if j == 0:                                       # the block's solve starts from y
                b2 = batch.slice(0, T)
                b2.x0, b2.U0, b2.tau0 = np.ascontiguousarray(y), np.ascontiguousarray(U0), np.ascontiguousarray(tau)
                r = ol.solve_batch(b2, opts, nthreads=min(nthreads, ol.num_procs()), want_K=True)
                statuses.append(r["stats"]["status"].copy())
                rs = r["stats"]
                tally += np.stack([rs["n_backward"], rs["n_forward"], np.maximum(rs["outer_iters"] - 1, 0), rs["inner_iters"]], axis=1)
            Xh[:, s] = x
            Yh[:, s] = y
            for t in range(T):
                u = r["U"][t, j].copy()
                if j > 0 and feedback:
                    dx = ol.quaternion_error(y[t], r["X"][t, j]) if es else y[t] - r["X"][t, j]
                    for a in range(3):
                        v = float(u[a])
                        for i in range(nh):
                            v += float(r["K"][t, j, i, a]) * float(dx[i])
                        u[a] = v
                u, (sure, maybe), _ = rr.limit(u, None if lo is None else lo[t], None if hi is None else hi[t])
                n_sure[t] += sure
                n_maybe[t] += maybe
                Uh[t, s] = u
                u_prev[t], rows_prev[t] = np.array(u, dtype=np.float64), rows[t]
                x[t] = rr.plant_step(ol, clock, t, 0, x[t], u, rr.plant_of(batch, t, None if plant is None else plant[t]), us,
                                     float(batch.dt[t]), po, ids[t], int(step0) + s, noisy, Rtab, gm)
            tau = tau + batch.dtau                           # one rounded addition per step
        for t in range(T):                                   # the shift by the block's steps inside the trajectory's own horizon
            n = int(nk[t])
            U0[t, :n - 1] = r["U"][t, np.minimum(np.arange(n - 1) + r_len, n - 2)]
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    out = dict(X_hist=Xh, U_hist=Uh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
               n_solves=len(statuses), statuses=np.array(statuses), tally=tally, Y_hist=Yh)
    if est is not None:
        for t in range(T):                                   # the closing predict across the last step
            ests[t].flown(u_prev[t], rows_prev[t])
        out.update(filt_state=np.stack([e.record() for e in ests]), filt_final=np.stack([e.final() for e in ests]))
    return out


class HeldModelMagState(mg.ModelMagState):
    """``model_mag_filtered_common.ModelMagState`` for the held loop: resumable from a record ``given`` (58,) — sample 0 then makes
    update(w_m,0, b_m,0, r_0) on it in place of ``first`` — and with ``rows`` "next" predicting across step s - 1 with the rows of
    step s (a condition of the tests)"""

    def __init__(self, ekf, predict=True, pair_own_row=True, rows="flown", given=None):
        rr.ModelState.__init__(self, ekf, predict, rows, given, FINAL_W)
        self.pair_own_row = pair_own_row

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev):
        e = self.ekf
        r = row_m if self.pair_own_row else rows[0]
        crossed = rows if self.rows == "next" else rows_prev
        if k == 0:
            if self.resumed:
                e.update(w_m, b_m, r)
            else:
                e.first(w_m, q_m)
                e.u = np.zeros(3)
            self.fin, post = e.final(), (e.w, e.q)
        elif latency:
            if k > 1:                                       # m_0 handed over a second time: no update
                e.update(w_m, b_m, r)
            self.fin, post = e.final(), (e.w, e.q)
            self._predict(u_prev, crossed)
        else:
            self._predict(u_prev, crossed)
            e.update(w_m, b_m, r)
            self.fin, post = e.final(), (e.w, e.q)
        return (e.w, e.q) if self.predict else post


def estimator(ol, batch, us, filt, plant=None, filt_init=None, variant=VARIANT):
    """t -> the estimator of trajectory t: ``ModelMagEkf`` behind ``HeldModelMagState``, resumed from filt_init[t] where one is
    given. ``filt`` None: no filter"""
    if filt is None:
        return None

    def make(t):
        J = plant[t, 0:9].reshape(3, 3).T if variant["inertia"] == "plant" else np.asarray(batch.Jmat[t]).reshape(3, 3).T
        ekf = mg.ModelMagEkf(ol, batch.dt[t], J, us, filt, dict(mg.VARIANT, command=variant["command"], mag=variant["mag"]))
        return HeldModelMagState(ekf, variant["predict"], variant["pair"] == "own", variant["rows"], None if filt_init is None else filt_init[t])

    return make


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, filt=None, filt_init=None, variant=VARIANT, est=None):
    """arguments and result as ``mpc_model_filtered_common.reference_loop``, ``filt`` the seven levels of this filter (None: no
    filter — the sensed reference); ``est`` replaces the estimator (the pin to the parent's reference)"""
    if est is None:
        est = estimator(ol, batch, float(opts.u_scale), filt, plant, filt_init, variant)
    return held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sc.IDEAL if sens is None else sens, bias, latency, plant, sat,
                     noise_id, step0, Rtab, gm, nthreads, est)


def measured(ol, batch, po, X_hist, sens, bias, latency, noise_id, step0=0):
    """the samples of the true states X_hist (T, n + 1, 7) as the sensor hands them over: (w_m, q_m) (T, n, 7), b_m (T, n, 3) and the
    rows they were formed with (T, n, 3) — the stage-0 row of a clock advanced by one rounded addition per step —, with the latency
    shift. No solve, no plant"""
    T, n = X_hist.shape[0], X_hist.shape[1] - 1
    noisy = int(po.noise_mode) == 1
    M, Bm, Rw = np.zeros((T, n, 7)), np.zeros((T, n, 3)), np.zeros((T, n, 3))
    tau = batch.tau0.copy()
    for s in range(n):
        clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
        for t in range(T):
            bt = None if bias is None else bias[t]
            w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, X_hist[t, s], po, noise_id[t], sens, bt, noisy)
            Rw[t, s] = dc._row(clock, t, 0, 0.0)
            M[t, s] = np.r_[w_m, q_m]
            Bm[t, s] = field_sample(ol, X_hist[t, s], Rw[t, s], po, noise_id[t], int(step0) + s, sens, bt, noisy)
        tau = tau + batch.dtau
    if latency:
        M, Bm, Rw = (np.concatenate([a[:, :1], a[:, :-1]], axis=1) for a in (M, Bm, Rw))
    return M, Bm, Rw


def estimates(ol, batch, us, filt, handed, U_hist, latency, filt_init=None):
    """the ``ModelMagEkf`` run over the samples ``handed`` = ``measured(...)`` with the returned U_hist (T, n, 3) and the rows of the
    batch's clock, the closing predict included: (Y (T, n, 7), filt_state (T, 58), filt_final (T, 12)). No solve, no plant."""
    M, Bm, Rw = handed
    T, n = M.shape[:2]
    Y, S, F = np.zeros((T, n, 7)), np.zeros((T, STATE_W)), np.zeros((T, FINAL_W))
    make = estimator(ol, batch, float(us), filt, None, filt_init)
    ests = [make(t) for t in range(T)]
    tau = batch.tau0.copy()
    rows_prev = [None] * T
    for s in range(n):
        clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
        for t in range(T):
            rows = rr.rows_of(clock, t, 0)
            Y[t, s] = np.r_[ests[t].sample(s, latency, M[t, s, :3], M[t, s, 3:7], Bm[t, s], Rw[t, s], rows, rows_prev[t],
                                           U_hist[t, s - 1] if s else None)]
            rows_prev[t] = rows
        tau = tau + batch.dtau
    for t in range(T):
        ests[t].flown(U_hist[t, n - 1], rows_prev[t])
        S[t], F[t] = ests[t].record(), ests[t].final()
    return Y, S, F


ON_OFF, ROWS, LATENCY, DELAY = mf.ON_OFF, mf.ROWS, mf.LATENCY, mf.DELAY
ATTITUDE = "this filter against the attitude-updated model filter"
MAG = "the magnetometer update on against off"
PAIRING = "the delayed sample paired with r_{s-1} against r_s"


def conditions(ref_of, label, batch, po, parent=None, skip=()):
    """the conditions of a parity case on references alone. ``ref_of(**over)`` is the reference of the test's call with the named
    arguments (filt, latency, variant) replaced; ``parent()`` the attitude-updated model filter's reference of the same call, or
    None. The call itself meets ``mpc_held_common.condition``; each term moves the final state by at least ``gg_common.MOVED``.
    Every figure is printed. ``skip`` names the labels a case leaves to the cases on which they show. Returns the reference of the
    call itself."""
    ref = ref_of()
    hc.condition(ref, batch, po, label)
    lat1 = lambda: ref_of(latency=1)
    terms = [(ON_OFF, ref, lambda: ref_of(filt=None))]
    if parent is not None:
        terms.append((ATTITUDE, ref, parent))
    terms += [(MAG, ref, lambda: ref_of(variant=dict(VARIANT, mag=False))),
              (PAIRING, lat1, lambda: ref_of(latency=1, variant=dict(VARIANT, pair="current"))),
              (ROWS, ref, lambda: ref_of(variant=dict(VARIANT, rows="next"))),
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


class EmuMpcModelMagFiltered:
    """ctypes binding of tests/emu/libtsat_emu_mpc_model_mag_filtered.so, built here by the emulator's pattern rule"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_model_mag_filtered.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_model_mag_filtered.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, sens=None, bias=None, latency=0, plant=None, sat=None, noise_id=None,
            step0=0, Rtab=None, gm=0.0, filt=FILT, filt_init=None):
        """emu_mpc_held_model_mag_filtered_batch; the result of ``mpc_model_filtered_common.EmuMpcModelFiltered.run``"""
        fo = None if filt is None else mg.filter_options(self.abi, filt)
        return mf6.filtered_run(self.lib.emu_mpc_held_model_mag_filtered_batch, self.abi, fo, (STATE_W, FINAL_W), filt_init, batch, opts,
                                po, n_steps, replan_every, feedback, sens, bias, latency, plant, sat, noise_id, step0, Rtab, gm)

    def check(self, fo, filt_init, T, filt_state=None, filt_final=None):
        """check_mpc_model_mag_filtered on the arguments tsat_mpc_run_held_model_mag_filtered adds"""
        text = C.create_string_buffer(256)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rc = self.lib.emu_mpc_model_mag_filtered_check(None if fo is None else C.byref(fo), self.abi.as_dp(c(filt_init)),
                                                       self.abi.as_dp(c(filt_state)), self.abi.as_dp(c(filt_final)), C.c_int64(T), text,
                                                       C.c_int32(256))
        return rc, text.value.decode()
