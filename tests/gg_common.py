"""Shared pieces of tests/test_gg.py (CPU tier) and tests/test_gpu_gg.py (GPU tier): the dispersed ensemble and the held loop UNDER
GRAVITY-GRADIENT TORQUE (tsat_tvlqr_ensemble_gg, tsat_mpc_run_held_gg).

THE REFERENCES are ``dispersed_common.reference_loop`` and ``mpc_held_common.reference_loop`` with the three lines of the
definition (include/tortoise_hip.h) added to every RK4 stage — ``gg_increment`` below, built from ``ol.qrot``, ``ol.inv3`` and
numpy's cross product only, which ``reference_rollout.plant_step`` adds where it is given an orbit table. With gm = 0 they have to equal their parents with
max |d| = 0 (test_gg.py::test_references_at_gm0_are_their_parents).

Inputs: the model flies the reference's 3U inertia (src/input_parameters.jl:46-51, diag(0.020833, 0.020833, 0.0041666) kg m^2:
``slew_setup.INERTIA["3U"]``) — on the isotropic 1U of the workloads r x (c r) vanishes and a test would show nothing —, the plants
are ``dispersed_common.all_five_plants`` / ``mpc_held_common.plants`` around it, the orbit rows those of the circular orbit the
synthetic field tables are sampled on. Every parity test first calls ``moved`` on the two references: the term has to move the
final state by at least 1e-7, 100 x the X_sim bar.

Also: the ctypes binding of the emulated kernels (tests/emu/tsat_emu_gg.cpp, built on demand by its own make fragment)."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import helpers
import mpc_held_common as hc

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
    import reference_rollout as rr          # here: that module is built on this one
    return rr.ensemble_loop(ol, "tv", batch, t, Xr, Ur, K, x0, opts, gid, Rtab, gm, plant, lo, hi, noisy=noisy)[:2]


def ensemble_pairs(ol, abi, batch, X, U, K, x0_sim, opts, pairs, Rtab, gm, plant=None, sat=None, noise_id0=None):
    """dispersed_common.reference_pairs with the term: the (t, m) pairs (n, 2), m = -1 the noise-free MODEL plant"""
    import reference_rollout as rr
    return rr.pairs_of(ol, abi, "tv", batch, x0_sim, K, opts, pairs, X=X, U=U, Rtab=Rtab, gm=gm, plant=plant, sat=sat, noise_id0=noise_id0)


def held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, Rtab, gm, plant=None, sat=None, noise_id=None, step0=0, nthreads=4):
    """mpc_held_common.reference_loop with the term in every plant step; arguments as there, then the orbit table and gm"""
    import reference_rollout as rr
    return rr.held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, plant=plant, sat=sat, noise_id=noise_id, step0=step0,
                        Rtab=Rtab, gm=gm, nthreads=nthreads)


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


def moved(final_with, final_without, label):
    """the condition of every parity test, on the two references alone: the term moves the final state by >= MOVED"""
    d = float(np.max(np.abs(np.asarray(final_with) - np.asarray(final_without))))
    print(f"{label}: the term moves the reference's final state by {d:.2e}")
    assert d >= MOVED, "the gravity-gradient term does not show on this case: a kernel that ignores the table would pass"
    return d


class EmuGg:
    """ctypes binding of tests/emu/libtsat_emu_gg.so (both emulated kernels), built here by its own make fragment"""

    def __init__(self, abi):
        self.lib = helpers.emu_library("libtsat_emu_gg.so")
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
        Rtab = np.ascontiguousarray(Rtab, dtype=np.float64)
        assert Rtab.shape == batch.Btab.shape
        args, out = hc.held_call(self.abi, batch, opts, po, n_steps, replan_every, feedback, plant, sat, noise_id, step0)
        rc = self.lib.emu_mpc_held_gg_batch(*args, self.abi.as_dp(Rtab), C.c_double(gm))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_gg_batch rc={rc}")
        return out

    def check(self, Rtab, gm):
        text = C.create_string_buffer(256)
        R = None if Rtab is None else np.ascontiguousarray(Rtab, dtype=np.float64)
        rc = self.lib.emu_gg_check(self.abi.as_dp(R), C.c_double(gm), C.c_int64(0 if R is None else R.size // 3), text, C.c_int32(256))
        return rc, text.value.decode()
