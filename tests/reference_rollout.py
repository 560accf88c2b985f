"""THE NUMPY REFERENCE ROLL-OUTS of the ensemble and held-loop tests, once each: what the per-feature ``*_common.py`` modules compare
the product against. Everything is built from the unchanged oracle's primitives only (``ol.qmult``, ``ol.qrot``, ``ol.inv3``,
``ol.dyn7``, ``ol.plant_noise``, ``ol.quaternion_error``, ``ol.solve_batch``) and numpy, in the manner of include/tortoise_hip.h:

    plant_step     one RK4 step of the true plant: ``ol.dyn7`` on Jp per stage under G u + m_res / u_scale, the noise injection of
                   src/simulator.jl:5-23 (``dispersed_common._noisy``), table rows floor((k + c) dtau + tau0) clamped
                   (``dispersed_common._row``), the gravity-gradient increment of ``gg_common`` where an orbit table is given
    limit          the component clip and the direction-preserving scale-back (limit_mode 1) with their CLIP_BAND brackets
    law_tv, law_pd the two laws, as functions of what the law is handed: (w, q, b)
    Raw, SixState, MagState, ModelState
                   the estimator between sensor and law, the numpy mirror of the product's ``Sensor``: the sequencing of first /
                   step / "m_0 handed over twice makes no step" / the prediction across the delay, once per filter. The filters'
                   arithmetic stays in ``filtered_common.Ekf``, ``mag_filtered_common.MagEkf``, ``model_filtered_common.ModelEkf``
    ensemble_loop  one closed loop of a (t, m) realisation; ``pairs_of`` drives it over pairs
    held_loop      the loop that re-plans every R control steps, for the whole batch

The per-feature modules keep their entry points as delegations to these, so a test that compares two of them ("filter None is the
sensed reference", "R = 1 is the every-step reference", "gm = 0 is the parent") checks the delegation and the switch it names."""
import collections
import math
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import sensed_common as sc

_IU = np.triu_indices(3)
STAGES = (0.0, 0.5, 1.0)


def plant_of(batch, t, plant):
    """(Jp, G, mres) of a plant record (21,); None: the model's inertia, ideal actuators"""
    if plant is None:
        return np.asarray(batch.Jmat[t]).reshape(3, 3).T, np.eye(3), np.zeros(3)
    return plant[0:9].reshape(3, 3).T, plant[9:18].reshape(3, 3).T, plant[18:21]


def rows_of(clock, t, k):
    """the field rows of knot k at c = 0, 1/2, 1"""
    return tuple(dc._row(clock, t, k, c) for c in STAGES)


def plant_step(ol, clock, t, k, x, u, plant, us, h, nopts, gid, knot, noisy, Rtab=None, gm=0.0, noise_fn=None):
    """x after one step of length h under the limited command u. ``clock`` carries the table clock (a batch, or the namespace the
    held loops advance) and k the knot on it; ``plant`` = (Jp, G, mres); the draws are those of generator ``gid`` at ``knot`` under
    the noise options ``nopts`` (noise_fn(t, knot, stage) -> nine values replaces ``ol.plant_noise``); Rtab None: no
    gravity-gradient term"""
    Jp, G, mres = plant
    ua = G @ u + mres / us
    draw = noise_fn or (lambda t_, k_, st_: ol.plant_noise(int(nopts.noise_seed), int(gid), k_, st_, nopts.sigma_gyro, nopts.sigma_att,
                                                           nopts.field_amp))
    nz = [draw(t, knot, st) if noisy else None for st in range(4)]
    b0, b1, b2 = rows_of(clock, t, k)
    r0, r1, r2 = [None] * 3 if Rtab is None else [gc._grow(clock, Rtab, t, k, c) for c in STAGES]

    def f(xx, bb, n, rr):
        xn, bn = dc._noisy(ol, xx, bb, n)
        kk = h * ol.dyn7(xn, ua, bn, Jp, us)
        if rr is not None:
            kk[0:3] = kk[0:3] + gc.gg_increment(ol, xx, rr, gm, Jp, h)
        return kk

    k1 = f(x, b0, nz[0], r0)
    k2 = f(x + k1 / 2, b1, nz[1], r1)
    k3 = f(x + k2 / 2, b1, nz[2], r1)
    k4 = f(x + k3, b2, nz[3], r2)
    return x + (k1 + 2 * k2 + 2 * k3 + k4) / 6


def limit(u, lo, hi, limit_mode=0):
    """the limited command, the (sure, maybe) increments of the clip counter's bracket — beyond a limit by more than the band;
    within the band of a limit, or beyond — and beta (limit_mode 1, where the band is applied to beta - 1; else None)"""
    if limit_mode == 1:
        r = np.array([u[c] / hi[c] if u[c] > 0 else (u[c] / lo[c] if u[c] < 0 else 0.0) for c in range(3)])
        beta = float(r.max())
        return (u * (1.0 / beta) if beta > 1.0 else u), (bool(beta - 1.0 > dc.CLIP_BAND), bool(beta - 1.0 > -dc.CLIP_BAND)), beta
    if lo is None:
        return u, (False, False), None
    bl, bh = dc.CLIP_BAND * np.abs(lo), dc.CLIP_BAND * np.abs(hi)
    sure, maybe = bool(np.any((lo - u > bl) | (u - hi > bh))), bool(np.any((lo - u > -bl) | (u - hi > -bh)))
    return np.minimum(np.maximum(u, lo), hi), (sure, maybe), None


def law_tv(ol, xr, ur, K, w, q, b, us, sign_rule=True):
    """u = Ur[k] - K[k]^T dX. ``b``, ``us`` and ``sign_rule`` are unused: they are here so that both laws are called alike"""
    qe = ol.qmult(np.r_[xr[3], -xr[4:7]], q)
    dX = np.r_[w - xr[:3], qe[1:4]]
    return ur - K.T @ dX


def law_pd(ol, xr, ur, gains, w, q, b, us, sign_rule=True):
    """the projection PD law of include/tortoise_hip.h on the body field b; ur None: no feed-forward; ``sign_rule`` False forces
    s = +1"""
    kd, kp = gains
    qe = ol.qmult(np.r_[xr[3], -xr[4:7]], q)
    dw = w - xr[:3]
    s = -1.0 if (sign_rule and qe[0] < 0) else 1.0
    treq = -(kd * dw + kp * (s * qe[1:4]))
    bb = float(b @ b)
    m = np.cross(b, treq) / bb if bb != 0.0 else np.zeros(3)
    return (ur if ur is not None else np.zeros(3)) + m / us


LAWS = dict(tv=law_tv, pd=law_pd)


def _full(tri):
    """the symmetric matrix of an upper triangle 00 01 02 11 12 22"""
    A = np.zeros((3, 3))
    A[_IU] = tri
    return np.triu(A) + np.triu(A, 1).T


class Raw:
    """THE ESTIMATOR PROTOCOL, and its trivial case: no filter, the law reads the sample itself. A roll-out calls ``sample`` once per
    knot (ensembles) or control step (held loops), k counted from the start of the loop, with the sample the sensor hands over at
    the call's ``latency`` — (w_m, q_m, b_m), knot max(k - 1, 0)'s at latency 1, and ``row_m``, the field row b_m was formed with
    (None in the held loops, which hand over no b_m) —, the field rows of knot k and of knot k - 1 (None at k = 0) and the limited
    command of knot k - 1; it gets back the (w, q) the law reads. ``flown`` is called once after the last
    step of a held loop with that step's command and rows. ``final`` is the filt_final record, ``record`` the flat filt_state."""
    estimates = False        # whether (w, q) is an estimate to be recorded (X_hat, filt_state)

    def __init__(self, final_w=9):
        self.final_w = final_w

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev):
        return w_m, q_m

    def flown(self, u, rows):
        pass

    def final(self):
        return np.zeros(self.final_w)


class SixState(Raw):
    """around a ``filtered_common.Ekf``: ``first`` at k = 0 (a ``step`` on the record ``given``, (31,), when there is one), no step
    at k = 1 of latency 1 (m_0 handed over a second time), a ``step`` otherwise; at latency 1 the attitude handed out from k = 1 on
    is predicted across the delay. ``predict`` False leaves that prediction out: a condition of the tests, not a mode of the product.
    The flat record is q^ 4, b^ 3, w^ 3, A 6, B 9, D 6 — A and D as upper triangles, B row-major."""
    estimates = True

    def __init__(self, ekf, predict=True, given=None):
        self.ekf, self.predict, self.resumed = ekf, predict, given is not None
        if self.resumed:
            ekf.q, ekf.b, ekf.w = np.array(given[0:4]), np.array(given[4:7]), np.array(given[7:10])
            ekf.A, ekf.B, ekf.D = _full(given[10:16]), np.array(given[16:25]).reshape(3, 3), _full(given[25:31])

    def _step(self, w_m, q_m, b_m, row_m, rows):
        self.ekf.step(w_m, q_m)

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev):
        e = self.ekf
        if k == 0 and not self.resumed:
            e.first(w_m, q_m)
        elif k == 0 or not (latency and k == 1):
            self._step(w_m, q_m, b_m, row_m, rows)
        return e.w, (e.predicted() if (latency and k > 0 and self.predict) else e.q)

    def final(self):
        return self.ekf.final()

    def record(self):
        e = self.ekf
        return np.r_[e.q, e.b, e.w, e.A[_IU], e.B.reshape(9), e.D[_IU]]


class MagState(SixState):
    """around a ``mag_filtered_common.MagEkf``: the sequencing of ``SixState``, each step against the sample's b_m and the row it
    was formed with (``row_m``: r_{k-1} for the delayed sample of latency 1). ``pair_own_row`` False pairs it with r_k: a condition
    of the tests (and so is the filter's own ``update`` False)"""

    def __init__(self, ekf, predict=True, pair_own_row=True):
        super().__init__(ekf, predict)
        self.pair_own_row = pair_own_row

    def _step(self, w_m, q_m, b_m, row_m, rows):
        self.ekf.step(w_m, b_m, row_m if self.pair_own_row else rows[0])


class ModelState(Raw):
    """around a ``model_filtered_common.ModelEkf``:

        latency 0:  k = 0 first(m_0);  k >= 1 predict(u_{k-1}, rows_{k-1}), update(m_k);                     (w^, q^) handed out
        latency 1:  k = 0 first(m_0);  k = 1 predict(u_0, rows_0) and no update;  k >= 2 update(m_{k-1}), predict(u_{k-1},
                    rows_{k-1});  (w-, q-) handed out for k >= 1

    With a record ``given`` (58,) sample 0 makes ``update(m_0)`` on it in place of ``first``. ``final`` is the record at the last
    update — or, in a held loop, after ``flown``: ONE MORE predict across the last step, the prior for x_n. Conditions of the tests,
    not modes of the product: ``predict`` False hands out the posterior at latency 1; ``rows`` "next" predicts across knot k - 1
    with the rows of knot k (the off-by-one of the clock). The flat record is q^ 4, w^ 3, b^ 3, the command of the last predict 3,
    then the covariance by blocks: A (theta theta), W (w w), D (b b) as upper triangles, X (theta w), B (theta b), Y (w b)
    row-major."""
    estimates = True

    def __init__(self, ekf, predict=True, rows="flown", given=None, final_w=12):
        self.ekf, self.predict, self.rows, self.resumed, self.fin = ekf, predict, rows, given is not None, np.zeros(final_w)
        if self.resumed:
            rec = np.asarray(given, dtype=np.float64)
            ekf.q, ekf.w, ekf.b, ekf.u = rec[0:4].copy(), rec[4:7].copy(), rec[7:10].copy(), rec[10:13].copy()
            A, W, D = _full(rec[13:19]), _full(rec[19:25]), _full(rec[25:31])
            X, B, Y = rec[31:40].reshape(3, 3), rec[40:49].reshape(3, 3), rec[49:58].reshape(3, 3)
            ekf.P = np.block([[A, X, B], [X.T, W, Y], [B.T, Y.T, D]])

    def _predict(self, u, rows):
        self.ekf.u = np.array(u, dtype=np.float64)
        self.ekf.predict(u, rows)

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev):
        e = self.ekf
        crossed = rows if self.rows == "next" else rows_prev
        if k == 0:
            if self.resumed:
                e.update(w_m, q_m)
            else:
                e.first(w_m, q_m)
                e.u = np.zeros(3)
            self.fin, post = e.final(), (e.w, e.q)
        elif latency:
            if k > 1:                                       # m_0 handed over a second time: no update
                e.update(w_m, q_m)
            self.fin, post = e.final(), (e.w, e.q)
            self._predict(u_prev, crossed)
        else:
            self._predict(u_prev, crossed)
            e.update(w_m, q_m)
            self.fin, post = e.final(), (e.w, e.q)
        return (e.w, e.q) if self.predict else post

    def flown(self, u, rows):
        self._predict(u, rows)
        self.fin = self.ekf.final()

    def final(self):
        return self.fin

    def record(self):
        e, P = self.ekf, self.ekf.P
        return np.r_[e.q, e.w, e.b, e.u, P[0:3, 0:3][_IU], P[3:6, 3:6][_IU], P[6:9, 6:9][_IU], P[0:3, 3:6].reshape(9),
                     P[0:3, 6:9].reshape(9), P[3:6, 6:9].reshape(9)]


Rollout = collections.namedtuple("Rollout", "X_sim clips U_cmd betas X_hat filt_final Y_raw")


def ensemble_loop(ol, law, batch, t, Xr, Ur, gains, x0, opts, gid, Rtab=None, gm=0.0, plant=None, lo=None, hi=None, limit_mode=0,
                  noisy=True, sens=None, latency=0, bias=None, est=None, sign_rule=True, k_start=0, k_stop=None, x_before=None):
    """one closed loop of slew t. law "tv": Xr (N, 7), Ur (N-1, 3) the plan, gains = K (N-1, 6, 3); law "pd": gains = (kd, kp), Xr
    None regulates (the record of every knot is xf), Ur None flies no feed-forward. plant (21,) or None for the model's, lo / hi
    (3,) or None, gid the generator id, Rtab (n_btab, n_tab, 3) or None (no gravity-gradient term). ``sens`` None: the law is handed
    the true state; else the three sigmas of ``sensed_common.measure``, with ``bias`` (9,) or None and the sample of knot
    max(k - 1, 0) handed over at ``latency`` 1. ``est`` is the estimator between sample and law (None: ``Raw``). k_start > 0: x0 is
    the state at that knot and ``x_before`` the state one knot earlier (latency 1); the loop stops at k_stop. Returns a ``Rollout``:
    X_sim (N, 7) zero-filled beyond the horizon, (n_sure, n_maybe), the commands before the limit (N-1, 3), the beta of every knot
    (limit_mode 1), X_hat (N, 7) (zero without a filter), filt_final, the raw (w_m, q_m) handed over per knot (N, 7)."""
    NS = batch.N
    N = NS if batch.n_knots is None else int(batch.n_knots[t])
    us, h = float(opts.u_scale), float(batch.dt[t])
    P = plant_of(batch, t, plant)
    est = Raw() if est is None else est
    Xs, Uc, Xh, Ym = np.zeros((NS, 7)), np.zeros((NS - 1, 3)), np.zeros((NS, 7)), np.zeros((NS, 7))
    x = np.array(x0, dtype=np.float64)
    n_sure = n_maybe = 0
    betas = []
    held = u_prev = None
    if sens is not None and latency and k_start > 0:
        held = sc.measure(ol, batch, t, k_start - 1, np.asarray(x_before, dtype=np.float64), opts, gid, sens, bias, noisy)
    rows_prev = rows_of(batch, t, k_start - 1) if k_start > 0 else None
    last = N - 1 if k_stop is None else min(N - 1, k_stop)
    for k in range(k_start, last):
        Xs[k] = x
        xr = batch.xf[t] if Xr is None else Xr[k]
        rows = rows_of(batch, t, k)
        row_m = rows[0]
        if sens is None:
            w_m, q_m = x[:3], x[3:7]
            b_m = ol.qrot(x[3:7] / math.sqrt(float(x[3:7] @ x[3:7])), rows[0]) if law == "pd" else None
        else:
            y = sc.measure(ol, batch, t, k, x, opts, gid, sens, bias, noisy)
            if latency and held is not None:                                    # y_max(k-1, 0), and the row it was formed with
                y, held, row_m = held, y, rows_prev[0]
            else:
                held = y
            w_m, q_m, b_m = y
        Ym[k] = np.r_[w_m, q_m]
        w, q = est.sample(k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev)
        if est.estimates:
            Xh[k] = np.r_[w, q]
        u = LAWS[law](ol, xr, None if Ur is None else Ur[k], gains[k] if law == "tv" else gains, w, q, b_m, us, sign_rule)
        Uc[k] = u
        u, (sure, maybe), beta = limit(u, lo, hi, limit_mode)
        n_sure, n_maybe = n_sure + sure, n_maybe + maybe
        if beta is not None:
            betas.append(beta)
        u_prev, rows_prev = np.array(u, dtype=np.float64), rows                # as the law issued it: what goes to the actuators
        x = plant_step(ol, batch, t, k, x, u, P, us, h, opts, gid, k, noisy, Rtab, gm)
    Xs[last] = x
    return Rollout(Xs, (n_sure, n_maybe), Uc, betas, Xh, est.final(), Ym)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=None, limit_mode=0,
             x0_nom=None, noise_id0=None, sens=None, latency=0, sensor=None, est=None, sign_rule=True):
    """``ensemble_loop`` on the (t, m) pairs (n, 2); m = -1 is the noise-free MODEL plant with the ideal sensor at the call's
    latency, from x0_nom[t] (default X[t, 0]); a realisation draws with the generator id0[t] + m. gains: K (T, N-1, 6, 3) for "tv",
    (kd, kp) each (T, 3) or (3,) for "pd"; plant (T, M, 21), sensor (T, M, 9), sat = (lo, hi) broadcastable to (T, 3), or None;
    ``est(t)`` makes the estimator of one loop (None: ``Raw``). Returns dict(X_sim (n, N, 7), stats (n,), n_sure (n,), n_maybe
    (n,), xf (n, 7), n_knots (n,), U_cmd (n, N-1, 3), betas (list per pair), X_hat (n, N, 7), filt_final (n, w), Y_raw (n, N, 7))."""
    T, M = x0_sim.shape[:2]
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    if law == "pd":
        gains = (np.broadcast_to(gains[0], (T, 3)), np.broadcast_to(gains[1], (T, 3)))
    ol.load()
    res = []
    for p in pairs:
        t, m = int(p[0]), int(p[1])
        g = gains[t] if law == "tv" else (gains[0][t], gains[1][t])
        kw = dict(lo=None if lo is None else lo[t], hi=None if hi is None else hi[t], limit_mode=limit_mode, sens=sens, latency=latency,
                  est=None if est is None else est(t), sign_rule=sign_rule)
        Xr, Ur = None if X is None else X[t], None if U is None else U[t]
        if m < 0:
            x0 = x0_nom[t] if x0_nom is not None else X[t, 0]
            res.append(ensemble_loop(ol, law, batch, t, Xr, Ur, g, x0, opts, 0, Rtab, gm, None, noisy=False, **kw))
        else:
            res.append(ensemble_loop(ol, law, batch, t, Xr, Ur, g, x0_sim[t, m], opts, id0[t] + m, Rtab, gm,
                                     None if plant is None else plant[t, m], bias=None if sensor is None else sensor[t, m], **kw))
    pairs = np.asarray(pairs)
    Xs = np.stack([r.X_sim for r in res])
    nk = ec.horizons(batch)[pairs[:, 0]]
    xf = batch.xf[pairs[:, 0]]
    st = dc.stats_of(abi, Xs, xf, nk, batch.dt[pairs[:, 0]], opts.min_steps, opts.w_tol, opts.angle_tol)
    return dict(X_sim=Xs, stats=st, n_sure=np.array([r.clips[0] for r in res]), n_maybe=np.array([r.clips[1] for r in res]), xf=xf,
                n_knots=nk, U_cmd=np.stack([r.U_cmd for r in res]), betas=[r.betas for r in res], X_hat=np.stack([r.X_hat for r in res]),
                filt_final=np.stack([r.filt_final for r in res]), Y_raw=np.stack([r.Y_raw for r in res]))


def held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
              noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, est=None, want_K=True, noise_fn=None):
    """the loop that re-plans every ``replan_every`` control steps, for the whole batch: ``ol.solve_batch`` with the advanced x0,
    tau0 and warm start once per block; the command rule of include/tortoise_hip.h (U_0 at j = 0; U_j + K_j dx at j > 0 with
    ``feedback``, the sum started from U_j with the columns ascending, dx = y - X_j or ``ol.quaternion_error(y, X_j)``; U_j
    without); the clip; ``plant_step`` at knot 0 of a clock advanced by ``tau += dtau`` once per step; the plan shifted by the
    block's steps inside the trajectory's own horizon; ``dispersed_common.stats_of`` on the history.

    plant (T, 21) or None (the model's), sat = (lo, hi) broadcastable to (T, 3) or None, noise_id (T,) or None (= t), po the noise
    options and the statistic's thresholds, Rtab the orbit table or None. ``sens`` None: solver and gains are given the true state;
    else y_s = ``sensed_common.measure`` of the true state — which the plant advances, the statistic judges and X_hist records —
    with ``bias`` (T, 9) or None, m_max(s-1, 0) at ``latency`` 1, s counted FROM THE CALL, through the estimator ``est(t)`` (None:
    ``Raw``). Returns dict(X_hist, U_hist, stats, X, U of the last solve, tracking_stats, n_sure, n_maybe, n_solves, statuses
    (n_solves, T), tally (T, 4): the sums of tsat_mpc_tally over the solves — column 1, n_forward, counts the ORACLE's roll-outs: a
    backend's own count, not comparable across backends), with Y_hist (T, n_steps, 7) under a sensor and filt_state, filt_final
    behind a filter."""
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
    ests = [Raw() if est is None else est(t) for t in range(T)]
    rows, rows_prev, u_prev = [None] * T, [None] * T, [None] * T              # the limited command and field rows of the step before
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
                rows[t] = rows_of(clock, t, 0)
                if sens is None:
                    y[t] = x[t]
                else:                                        # the sample handed over: m_s, or m_max(s-1, 0)
                    w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, x[t], po, ids[t], sens, None if bias is None else bias[t], noisy)
                    m = np.r_[w_m, q_m]
                    y[t] = held[t] if (latency and s > 0) else m
                    held[t] = m
                w, q = ests[t].sample(s, latency, y[t, :3], y[t, 3:7], None, None, rows[t], rows_prev[t], u_prev[t])
                if ests[t].estimates:                        # the filter between the sample and everything that reads y
                    y[t] = np.r_[w, q]
            if j == 0:                                       # the block's solve starts from y
                b2 = batch.slice(0, T)
                b2.x0, b2.U0, b2.tau0 = np.ascontiguousarray(y), np.ascontiguousarray(U0), np.ascontiguousarray(tau)
                r = ol.solve_batch(b2, opts, nthreads=min(nthreads, ol.num_procs()), want_K=want_K)
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
                u, (sure, maybe), _ = limit(u, None if lo is None else lo[t], None if hi is None else hi[t])
                n_sure[t] += sure
                n_maybe[t] += maybe
                Uh[t, s] = u
                u_prev[t], rows_prev[t] = np.array(u, dtype=np.float64), rows[t]
                x[t] = plant_step(ol, clock, t, 0, x[t], u, plant_of(batch, t, None if plant is None else plant[t]), us, float(batch.dt[t]),
                                  po, ids[t], int(step0) + s, noisy, Rtab, gm, noise_fn)
            tau = tau + batch.dtau                           # one rounded addition per step
        for t in range(T):                                   # the shift by the block's steps inside the trajectory's own horizon
            n = int(nk[t])
            U0[t, :n - 1] = r["U"][t, np.minimum(np.arange(n - 1) + r_len, n - 2)]
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    out = dict(X_hist=Xh, U_hist=Uh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
               n_solves=len(statuses), statuses=np.array(statuses), tally=tally)
    if sens is not None:
        out["Y_hist"] = Yh
    if est is not None:
        for t in range(T):                                   # the nine-state filter's closing predict across the last step
            ests[t].flown(u_prev[t], rows_prev[t])
        out.update(filt_state=np.stack([e.record() for e in ests]), filt_final=np.stack([e.final() for e in ests]))
    return out
