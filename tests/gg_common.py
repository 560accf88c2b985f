"""Shared pieces of tests/test_gg.py (CPU tier) and tests/test_gpu_gg.py (GPU tier): the dispersed ensemble and the held loop UNDER
GRAVITY-GRADIENT TORQUE (tsat_tvlqr_ensemble_gg, tsat_mpc_run_held_gg).

THE REFERENCES are ``dispersed_common.reference_loop`` and ``mpc_held_common.reference_loop`` restated with the three lines of the
definition (include/tortoise_hip.h) added to every RK4 stage — ``gg_increment`` below, built from ``ol.qrot``, ``ol.inv3`` and
numpy's cross product only —, everything else operation for operation as there. With gm = 0 they have to equal their parents with
max |d| = 0 (test_gg.py::test_references_at_gm0_are_their_parents).

Inputs: the model flies the reference's 3U inertia (src/input_parameters.jl:46-51, diag(0.020833, 0.020833, 0.0041666) kg m^2:
``slew_setup.INERTIA["3U"]``) — on the isotropic 1U of the workloads r x (c r) vanishes and a test would show nothing —, the plants
are ``dispersed_common.all_five_plants`` / ``mpc_held_common.plants`` around it, the orbit rows those of the circular orbit the
synthetic field tables are sampled on. Every parity test first calls ``moved`` on the two references: the term has to move the
final state by at least 1e-7, 100 x the X_sim bar.

Also: the ctypes binding of the emulated kernels (tests/emu/tsat_emu_gg.cpp, built on demand by its own make fragment)."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import mpc_held_common as hc
from conftest import ROOT

GM = 3.986004418e5          # km^3 / s^2
MOVED = 1e-7                # what the term has to change on the references before a kernel is looked at
A_KM, INC = 6771.0, 96.6    # the orbit of the workloads' synthetic field tables


def use_3u(pkg, batch):
    """the batch with the 3U inertia as the model's (in place); returns it"""
    batch.Jmat[:] = pkg.slew_setup.jmat_cm(pkg.slew_setup.INERTIA["3U"])
    return batch


def orbit(pkg, n_tab, dt_row, raan=0.0, nu=0.0):
    return pkg.slew_setup.circular_orbit_rows(n_tab, dt_row, A_KM, INC, raan, nu)


def _grow(clock, Rtab, t, k, c):
    """the orbit row of a stage: the index dispersed_common._row computes for the field row"""
    v = dc._fma(k + c, float(clock.dtau[t]), float(clock.tau0[t])) if dc._fma else (k + c) * float(clock.dtau[t]) + float(clock.tau0[t])
    r = math.floor(v)
    i = 0 if not r >= 0 else min(int(r), clock.n_tab - 1)
    return Rtab[clock.btab_idx[t], i]


def gg_increment(ol, x, r_km, gm, Jp, h):
    """what the definition adds to k[0:3] of a stage evaluated at the state x (as integrated, before the noise injection)"""
    q = x[3:7] / math.sqrt(float(x[3:7] @ x[3:7]))
    n = math.sqrt(float(r_km @ r_km))
    rb = ol.qrot(q, r_km / n)
    tau = (3.0 * gm / n ** 3) * np.cross(rb, Jp @ rb)
    return (h * ol.inv3(Jp)) @ tau


def ensemble_loop(ol, batch, t, Xr, Ur, K, x0, opts, gid, Rtab, gm, plant=None, lo=None, hi=None, noisy=True):
    """dispersed_common.reference_loop with the term; arguments as there, then the orbit table (n_btab, n_tab, 3) and gm"""
    NS = batch.N
    N = NS if batch.n_knots is None else int(batch.n_knots[t])
    us, h = float(opts.u_scale), float(batch.dt[t])
    if plant is None:
        Jp, G, mres = np.asarray(batch.Jmat[t]).reshape(3, 3).T, np.eye(3), np.zeros(3)
    else:
        Jp, G, mres = plant[0:9].reshape(3, 3).T, plant[9:18].reshape(3, 3).T, plant[18:21]
    Xs = np.zeros((NS, 7))
    x = np.array(x0, dtype=np.float64)
    n_sure = n_maybe = 0
    for k in range(N - 1):
        Xs[k] = x
        xr = Xr[k]
        qe = ol.qmult(np.r_[xr[3], -xr[4:7]], x[3:7])
        dX = np.r_[x[:3] - xr[:3], qe[1:4]]
        u = Ur[k] - K[k].T @ dX
        if lo is not None:
            bl, bh = dc.CLIP_BAND * np.abs(lo), dc.CLIP_BAND * np.abs(hi)
            n_sure += bool(np.any((lo - u > bl) | (u - hi > bh)))
            n_maybe += bool(np.any((lo - u > -bl) | (u - hi > -bh)))
            u = np.minimum(np.maximum(u, lo), hi)
        ua = G @ u + mres / us
        nz = [ol.plant_noise(int(opts.noise_seed), int(gid), k, s, opts.sigma_gyro, opts.sigma_att, opts.field_amp) if noisy else None
              for s in range(4)]
        b0, b1, b2 = dc._row(batch, t, k, 0.0), dc._row(batch, t, k, 0.5), dc._row(batch, t, k, 1.0)
        r0, r1, r2 = _grow(batch, Rtab, t, k, 0.0), _grow(batch, Rtab, t, k, 0.5), _grow(batch, Rtab, t, k, 1.0)

        def f(xx, bb, n, rr):
            xn, bn = dc._noisy(ol, xx, bb, n)
            kk = h * ol.dyn7(xn, ua, bn, Jp, us)
            kk[0:3] = kk[0:3] + gg_increment(ol, xx, rr, gm, Jp, h)
            return kk

        k1 = f(x, b0, nz[0], r0)
        k2 = f(x + k1 / 2, b1, nz[1], r1)
        k3 = f(x + k2 / 2, b1, nz[2], r1)
        k4 = f(x + k3, b2, nz[3], r2)
        x = x + (k1 + 2 * k2 + 2 * k3 + k4) / 6
    Xs[N - 1] = x
    return Xs, (n_sure, n_maybe)


def ensemble_pairs(ol, abi, batch, X, U, K, x0_sim, opts, pairs, Rtab, gm, plant=None, sat=None, noise_id0=None):
    """dispersed_common.reference_pairs with the term: the (t, m) pairs (n, 2), m = -1 the noise-free MODEL plant"""
    T, M = x0_sim.shape[:2]
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    ol.load()
    res = []
    for p in pairs:
        t, m = int(p[0]), int(p[1])
        kw = dict(lo=None if lo is None else lo[t], hi=None if hi is None else hi[t])
        if m < 0:
            res.append(ensemble_loop(ol, batch, t, X[t], U[t], K[t], X[t, 0], opts, 0, Rtab, gm, None, noisy=False, **kw))
        else:
            res.append(ensemble_loop(ol, batch, t, X[t], U[t], K[t], x0_sim[t, m], opts, id0[t] + m, Rtab, gm,
                                     None if plant is None else plant[t, m], **kw))
    pairs = np.asarray(pairs)
    Xs = np.stack([r[0] for r in res])
    nk = ec.horizons(batch)[pairs[:, 0]]
    xf = batch.xf[pairs[:, 0]]
    st = dc.stats_of(abi, Xs, xf, nk, batch.dt[pairs[:, 0]], opts.min_steps, opts.w_tol, opts.angle_tol)
    return dict(X_sim=Xs, stats=st, n_sure=np.array([r[1][0] for r in res]), n_maybe=np.array([r[1][1] for r in res]), xf=xf, n_knots=nk)


def kept(ref, opts):
    """dispersed_common.kept under the statistic of `opts` (that function judges with the default thresholds, which a 20-knot
    horizon never meets): the first N_KEPT sampled realisations off the thresholds, the same replacement cap (2 of 34)"""
    ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], opts.min_steps, opts.w_tol,
                             opts.angle_tol) > dc.MARGIN for i in range(len(ref["stats"]))])
    keep = np.flatnonzero(ok)[:dc.N_KEPT]
    print(f"sampled pairs that fail the margin: {int(np.count_nonzero(~ok))} of {len(ok)}; arrivals among the kept: "
          f"{int(np.count_nonzero(ref['stats']['failed'][keep] == 0))}")
    assert keep.size == dc.N_KEPT, "more than 2 of 34 sampled realisations sit on a threshold"
    return keep


def held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, Rtab, gm, plant=None, sat=None, noise_id=None, step0=0, nthreads=4):
    """mpc_held_common.reference_loop with the term in every plant step; arguments as there, then the orbit table and gm"""
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
    statuses, tally = [], np.zeros((T, 4), dtype=np.int64)
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
                    bl, bh = hc.CLIP_BAND * np.abs(lo[t]), hc.CLIP_BAND * np.abs(hi[t])
                    n_sure[t] += bool(np.any((lo[t] - u > bl) | (u - hi[t] > bh)))
                    n_maybe[t] += bool(np.any((lo[t] - u > -bl) | (u - hi[t] > -bh)))
                    u = np.minimum(np.maximum(u, lo[t]), hi[t])
                Uh[t, s] = u
                ua = G @ u + mres / us
                nz = [ol.plant_noise(int(po.noise_seed), int(ids[t]), int(step0) + s, st, po.sigma_gyro, po.sigma_att, po.field_amp)
                      if noisy else None for st in range(4)]
                b0, b1, b2r = dc._row(clock, t, 0, 0.0), dc._row(clock, t, 0, 0.5), dc._row(clock, t, 0, 1.0)
                r0, r1, r2 = _grow(clock, Rtab, t, 0, 0.0), _grow(clock, Rtab, t, 0, 0.5), _grow(clock, Rtab, t, 0, 1.0)
                h = float(batch.dt[t])

                def f(xx, bb, n, rr):
                    xn, bn = dc._noisy(ol, xx, bb, n)
                    kk = h * ol.dyn7(xn, ua, bn, Jp, us)
                    kk[0:3] = kk[0:3] + gg_increment(ol, xx, rr, gm, Jp, h)
                    return kk

                k1 = f(x[t], b0, nz[0], r0)
                k2 = f(x[t] + k1 / 2, b1, nz[1], r1)
                k3 = f(x[t] + k2 / 2, b1, nz[2], r1)
                k4 = f(x[t] + k3, b2r, nz[3], r2)
                x[t] = x[t] + (k1 + 2 * k2 + 2 * k3 + k4) / 6
            tau = tau + batch.dtau                           # one rounded addition per step
        for t in range(T):                                   # the shift by the block's steps inside the trajectory's own horizon
            n = int(nk[t])
            U0[t, :n - 1] = r["U"][t, np.minimum(np.arange(n - 1) + r_len, n - 2)]
    Xh[:, n_steps] = x
    ts = dc.stats_of(ol._abi, Xh, batch.xf, np.full(T, n_steps + 1), batch.dt, po.min_steps, po.w_tol, po.angle_tol)
    return dict(X_hist=Xh, U_hist=Uh, stats=r["stats"], X=r["X"], U=r["U"], tracking_stats=ts, n_sure=n_sure, n_maybe=n_maybe,
                n_solves=len(statuses), statuses=np.array(statuses), tally=tally)


def moved(final_with, final_without, label):
    """the condition of every parity test, on the two references alone: the term moves the final state by >= MOVED"""
    d = float(np.max(np.abs(np.asarray(final_with) - np.asarray(final_without))))
    print(f"{label}: the term moves the reference's final state by {d:.2e}")
    assert d >= MOVED, "the gravity-gradient term does not show on this case: a kernel that ignores the table would pass"
    return d


class EmuGg:
    """ctypes binding of tests/emu/libtsat_emu_gg.so (both emulated kernels), built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_gg.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_gg.so"))
        self.abi = abi

    def ensemble(self, batch, X, U, Qd, Qfd, Rd, x0_sim, K, opts, plant, Rtab, gm, sat=None, noise_id0=None):
        """emu_tvlqr_ensemble_gg; arguments and result as ensemble_common.EmuEnsemble.run with plants"""
        T, N, M = batch.T, batch.N, x0_sim.shape[1]
        o = self.abi.TvlqrOptions.from_buffer_copy(opts)
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        X, U, Qd, Qfd, Rd, x0_sim, K, plant, Rtab = c(X), c(U), c(Qd), c(Qfd), c(Rd), c(x0_sim), c(K), c(plant), c(Rtab)
        assert plant.shape == (T, M, 21) and Rtab.shape == batch.Btab.shape
        st = np.zeros((T, M), dtype=self.abi.TVLQR_STATS_DTYPE)
        nom = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        summary = np.zeros((T, 8))
        Xs = np.full((T, M, N, 7), np.nan)
        ncl = np.full((T, M), -1, dtype=np.int32)
        d = self.abi.as_dp
        id0 = None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64)
        nk = None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32)
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        rc = self.lib.emu_tvlqr_ensemble_gg(
            C.byref(o), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), C.c_int32(M), d(X), d(U), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(Qd), d(Qfd), d(Rd), d(x0_sim),
            None if id0 is None else id0.ctypes.data_as(C.POINTER(C.c_int64)), self.abi.as_ip(nk), d(plant), d(lo), d(hi), d(K),
            st.ctypes.data_as(C.c_void_p), d(summary), nom.ctypes.data_as(C.c_void_p), d(Xs), self.abi.as_ip(ncl), d(Rtab), C.c_double(gm))
        if rc != 0:
            raise RuntimeError(f"emu_tvlqr_ensemble_gg rc={rc}")
        return dict(stats=st, summary=summary, nominal=nom, X_sim=Xs, n_clipped=ncl)

    def held(self, batch, opts, po, n_steps, replan_every, feedback, Rtab, gm, plant=None, sat=None, noise_id=None, step0=0):
        """emu_mpc_held_gg_batch; arguments and result as mpc_held_common.EmuMpcHeld.run"""
        T, N = batch.T, batch.N
        o = opts.copy()
        o.n_knots, o.n_tab = N, batch.n_tab
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        plant, Rtab = c(plant), c(Rtab)
        assert Rtab.shape == batch.Btab.shape
        lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
        ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
        Xh = np.zeros((T, n_steps + 1, 7)); Uh = np.zeros((T, n_steps, 3))
        X = np.zeros((T, N, 7)); U = np.zeros((T, N - 1, 3))
        st = np.zeros(T, dtype=self.abi.STATS_DTYPE)
        ts = np.zeros(T, dtype=self.abi.TVLQR_STATS_DTYPE)
        ncl = np.full(T, -1, dtype=np.int32)
        d = self.abi.as_dp
        rc = self.lib.emu_mpc_held_gg_batch(
            C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            self.abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd),
            d(batch.Rd), d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every),
            C.c_int32(feedback), d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), self.abi.as_ip(ncl), d(X), d(U),
            None if batch.n_knots is None else self.abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32)), d(Rtab),
            C.c_double(gm))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_gg_batch rc={rc}")
        return dict(X_hist=Xh, U_hist=Uh, stats=st, X=X, U=U, tracking_stats=ts, n_clipped=ncl)

    def check(self, Rtab, gm):
        text = C.create_string_buffer(256)
        R = None if Rtab is None else np.ascontiguousarray(Rtab, dtype=np.float64)
        rc = self.lib.emu_gg_check(self.abi.as_dp(R), C.c_double(gm), C.c_int64(0 if R is None else R.size // 3), text, C.c_int32(256))
        return rc, text.value.decode()
