"""Closed-loop tracking of solved slews on the GPU — the caller right after ``solve!`` in the reference.

``attitude_simulation(f!, f_gains!, integration, X, U, dt, x0_lqr, t0, tf, Q_lqr, R_lqr, Qf_lqr)``
(src/attitude_controller.jl:1-48) computes TVLQR gains around the optimised trajectory (``attitude_lqr``, :50-119),
simulates the noisy plant (src/simulator.jl) under ``U_sim = U - K dX`` and returns ``X_sim, U_sim, dX, K``;
src/monte_carlo.jl:242-262 then turns ``X_sim`` into a slew time / failure flag. Here the same call runs for a whole
batch through ``tsat_tvlqr_batch``; randomness is an explicit input so that runs are reproducible and checkable.
"""
import ctypes as C

import numpy as np

from . import _abi
from .slew_setup import SlewBatch, qmult


def tvlqr_weights(T, alpha=10.0, beta=10.0, r=7.5e3):
    """Q_lqr = diag(alpha 1_3, beta 1_3), Qf_lqr = 100 Q_lqr, R_lqr = r I (src/TortoiseSat.jl:251-260; the
    Monte-Carlo uses r = 0.5e3, src/monte_carlo.jl:228)."""
    Qd = np.tile(np.r_[np.full(3, alpha), np.full(3, beta)], (T, 1))
    return Qd, 100.0 * Qd, np.full((T, 3), float(r))


def perturbed_initial_state(x0, rng, sigma=(np.pi / 180.0) ** 2):
    """x0_lqr of src/TortoiseSat.jl:227-234: rates kept, attitude rotated by a random small rotation vector."""
    x0 = np.asarray(x0, dtype=np.float64)
    out = x0.copy()
    for t in range(x0.shape[0]):
        nq = rng.standard_normal(3) * sigma
        th = np.linalg.norm(nq)
        out[t, 3:7] = qmult(x0[t, 3:7], np.r_[np.cos(th / 2.0), nq / th * np.sin(th / 2.0)])
    return out


def simulator_noise(T, N, rng):
    """The draws ``simulator`` makes per dynamics evaluation (src/simulator.jl:5,10,22), laid out (T, N-1, 4, 9):
    gyro noise randn(3)(0.38 deg)^2, attitude-noise rotation vector randn(3)(1 deg)^2, field noise rand(3) 1e-10."""
    g = rng.standard_normal((T, N - 1, 4, 3)) * (0.38 * np.pi / 180.0) ** 2
    a = rng.standard_normal((T, N - 1, 4, 3)) * (1.0 * np.pi / 180.0) ** 2
    b = rng.random((T, N - 1, 4, 3)) * (1.0e-5) ** 2
    return np.ascontiguousarray(np.concatenate([g, a, b], axis=3))


_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr):
    """Philox4x32-10 on arrays: key (2,) or (..., 2), ctr (..., 4) of 32-bit words held in uint64. Returns (..., 4)."""
    k0, k1 = np.uint64(key[..., 0]) + np.zeros(ctr.shape[:-1], np.uint64), np.uint64(key[..., 1]) + np.zeros(ctr.shape[:-1], np.uint64)
    c0, c1, c2, c3 = (ctr[..., i].astype(np.uint64) for i in range(4))
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _LO, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _LO
    return np.stack([c0, c1, c2, c3], axis=-1)


def generated_noise(seed, ids, N, sigma_gyro=(0.38 * np.pi / 180.0) ** 2, sigma_att=(np.pi / 180.0) ** 2, field_amp=1e-10):
    """What ``noise_mode = 1`` draws inside the kernel (include/tortoise_hip.h), as an array (T, N-1, 4, 9) — the same
    run can then be repeated in array mode, or inspected."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    T = ids.shape[0]
    key = np.array([np.uint64(seed) & _LO, np.uint64(seed) >> np.uint64(32)], dtype=np.uint64)
    ctr = np.zeros((T, N - 1, 4, 3, 4), dtype=np.uint64)
    ctr[..., 0] = (ids & _LO)[:, None, None, None]
    ctr[..., 1] = (ids >> np.uint64(32))[:, None, None, None]
    ctr[..., 2] = np.arange(N - 1, dtype=np.uint64)[None, :, None, None]
    ctr[..., 3] = (4 * np.arange(4, dtype=np.uint64))[None, None, :, None] + np.arange(3, dtype=np.uint64)[None, None, None, :]
    w = philox4x32_10(key, ctr).astype(np.float64)                       # (T, N-1, 4, 3, 4)
    u = (w + 0.5) / 4294967296.0

    def bm(a, b):
        r, th = np.sqrt(-2.0 * np.log(a)), 2.0 * np.pi * b
        return r * np.cos(th), r * np.sin(th)

    z0, z1 = bm(u[..., 0, 0], u[..., 0, 1]); z2, z3 = bm(u[..., 0, 2], u[..., 0, 3]); z4, z5 = bm(u[..., 1, 0], u[..., 1, 1])
    out = np.stack([sigma_gyro * z0, sigma_gyro * z1, sigma_gyro * z2, sigma_att * z3, sigma_att * z4, sigma_att * z5,
                    field_amp * u[..., 1, 2], field_amp * u[..., 1, 3], field_amp * u[..., 2, 0]], axis=-1)
    return np.ascontiguousarray(out)


def attitude_simulation(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise=None, linearize_dt_sq=True,
                        u_scale=1e-2, min_steps=10, w_tol=0.05, angle_tol=0.08727, noise_seed=None, noise_ids=None,
                        want_K=True, want_trajectories=True, rate_as_written=False, trial_ids=None):
    """Batched ``attitude_simulation`` + slew-time statistic. ``solver`` is an AugmentedLagrangianSolver (owns the GPU
    handle); X (T,N,7), U (T,N-1,3) are the solved trajectories — or both ``None`` to track the batch that is resident on
    the device right after ``solve_`` (no re-upload of trajectories and tables; ``batch`` must be the one just solved).
    Plant noise: ``noise`` array (T,N-1,4,9), or ``noise_seed`` (+ optional per-trajectory ``noise_ids``) to have the
    kernel draw it, or neither for the noise-free plant. Returns dict(X_sim, U_sim, K (T,N-1,6,3), stats);
    ``want_trajectories=False`` brings only the slew-time statistic back (X_sim = U_sim = None).
    ``rate_as_written=True`` evaluates the statistic as the reference's line reads, ``norm(sim_states[i][1:3,i])``
    (src/monte_carlo.jl:247): for every sample j the rate of sample i, the 1-based number of the trial — ``trial_ids`` (0-based,
    default: ``noise_ids``, else the position in the batch); the default takes the rate of sample j, which the line means."""
    lib = _abi.load()
    T, N = batch.T, batch.N
    o = _abi.TvlqrOptions()
    lib.tsat_tvlqr_default_options(C.byref(o))
    ids = None
    if noise_seed is not None:
        if noise is not None:
            raise ValueError("give either a noise array or a noise seed")
        o.noise_mode, o.noise_seed = 1, int(noise_seed)
        ids = None if noise_ids is None else np.ascontiguousarray(noise_ids, dtype=np.int64)
    elif noise_ids is not None and not rate_as_written:
        raise ValueError("noise_ids key the noise the kernel draws: they need noise_seed (or rate_as_written, whose trial numbers they are)")
    if rate_as_written:
        o.rate_as_written = 1
        if ids is None and noise_ids is not None:      # the trial numbers, whatever the noise comes from (an array, or none)
            ids = np.ascontiguousarray(noise_ids, dtype=np.int64)
        if trial_ids is not None:
            if ids is not None and not np.array_equal(ids, np.asarray(trial_ids, dtype=np.int64)):
                raise ValueError("trial_ids and noise_ids are the same index of the reference's loop: give one, or equal arrays")
            ids = np.ascontiguousarray(trial_ids, dtype=np.int64)
    o.n_knots, o.n_tab, o.linearize_dt_sq, o.min_steps = N, batch.n_tab, int(bool(linearize_dt_sq)), int(min_steps)
    o.u_scale, o.w_tol, o.angle_tol = float(u_scale), float(w_tol), float(angle_tol)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    resident = X is None and U is None
    x0_sim, Qd, Qfd, Rd = c(x0_sim), c(Qd), c(Qfd), c(Rd)
    if not resident:
        X, U = c(X), c(U)
        if X.shape != (T, N, 7) or U.shape != (T, N - 1, 3):
            raise ValueError("array shapes do not match the batch")
    if x0_sim.shape != (T, 7) or Qd.shape != (T, 6) or Qfd.shape != (T, 6) or Rd.shape != (T, 3):
        raise ValueError("array shapes do not match the batch")
    if noise is not None:
        noise = c(noise)
        if noise.shape != (T, N - 1, 4, 9):
            raise ValueError("noise must be (T, N-1, 4, 9)")
    Xs = np.empty((T, N, 7)) if want_trajectories else None
    Us = np.empty((T, N - 1, 3)) if want_trajectories else None
    K = np.empty((T, N - 1, 6, 3)) if want_K else None
    nk = None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32)
    st = np.zeros(T, dtype=_abi.TVLQR_STATS_DTYPE)
    d = _abi.as_dp
    idp = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64))
    if resident:
        rc = lib.tsat_tvlqr_resident(solver._h, C.byref(o), d(Qd), d(Qfd), d(Rd), d(x0_sim), d(noise), d(Xs), d(Us), d(K),
                                     st.ctypes.data_as(C.c_void_p), idp)
        solver._check(rc, "tsat_tvlqr_resident")
        return dict(X_sim=Xs, U_sim=Us, K=K, stats=st)
    rc = lib.tsat_tvlqr_batch(solver._h, C.byref(o), T, batch.Btab.shape[0], d(X), d(U), d(batch.xf), d(batch.Btab),
                              _abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat),
                              d(Qd), d(Qfd), d(Rd), d(x0_sim), d(noise), d(Xs), d(Us), d(K), st.ctypes.data_as(C.c_void_p),
                              _abi.as_ip(nk), idp)
    solver._check(rc, "tsat_tvlqr_batch")
    return dict(X_sim=Xs, U_sim=Us, K=K, stats=st)


def ensemble_initial_states(x0, M, rng):
    """x0_lqr of M realisations per slew, (T, M, 7): the ``perturbed_initial_state`` rule (src/monte_carlo.jl:204-210) drawn
    once per realisation, realisation after realisation."""
    x0 = np.asarray(x0, dtype=np.float64)
    return np.ascontiguousarray(np.stack([perturbed_initial_state(x0, rng) for _ in range(int(M))], axis=1))


def ensemble_noise_ids(T, M, noise_id0=None):
    """Generator ids of an ensemble, (T, M): ``noise_id0[t] + m`` (default ``t * M + m``) — the ``noise_ids`` under which
    ``attitude_simulation`` (or the oracle) repeats realisation m of slew t."""
    id0 = np.arange(T, dtype=np.int64) * int(M) if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    return id0[:, None] + np.arange(int(M), dtype=np.int64)[None, :]


def _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K, want_trajectories,
                   linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol):
    """What ``tsat_tvlqr_ensemble`` and ``tsat_tvlqr_ensemble_dispersed`` have in common: the shape checks, the option block and
    the output buffers. Returns (lib, head, tail, out): the C arguments from the handle to ``n_knots`` and from ``stats`` to
    ``X_sim`` — the dispersed call puts its own between and after them — and the dict the caller returns."""
    lib = _abi.load()
    T, N = batch.T, batch.N
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    X, U, x0_sim, Qd, Qfd, Rd = c(X), c(U), c(x0_sim), c(Qd), c(Qfd), c(Rd)
    if X.shape != (T, N, 7) or U.shape != (T, N - 1, 3) or Qd.shape != (T, 6) or Qfd.shape != (T, 6) or Rd.shape != (T, 3):
        raise ValueError("array shapes do not match the batch")
    if x0_sim.ndim != 3 or x0_sim.shape[0] != T or x0_sim.shape[2] != 7:
        raise ValueError("x0_sim must be (T, M, 7)")
    M = x0_sim.shape[1]
    o = _abi.TvlqrOptions()
    lib.tsat_tvlqr_default_options(C.byref(o))
    o.n_knots, o.n_tab, o.linearize_dt_sq, o.min_steps = N, batch.n_tab, int(bool(linearize_dt_sq)), int(min_steps)
    o.u_scale, o.w_tol, o.angle_tol = float(u_scale), float(w_tol), float(angle_tol)
    o.noise_mode, o.noise_seed = 1, int(noise_seed)
    o.sigma_gyro, o.sigma_att = o.sigma_gyro * float(sigma_scale), o.sigma_att * float(sigma_scale)
    id0 = None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64)
    if id0 is not None and id0.shape != (T,):
        raise ValueError("noise_id0 must be (T,)")
    nk = None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32)
    st = np.zeros((T, M), dtype=_abi.TVLQR_STATS_DTYPE)
    nom = np.zeros(T, dtype=_abi.TVLQR_STATS_DTYPE)
    summary = np.zeros((T, 8))
    K = np.empty((T, N - 1, 6, 3)) if want_K else None
    Xs = np.empty((T, M, N, 7)) if want_trajectories else None
    d = _abi.as_dp
    head = [solver._h, C.byref(o), T, batch.Btab.shape[0], M, d(X), d(U), d(batch.xf), d(batch.Btab), _abi.as_ip(batch.btab_idx),
            d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(Qd), d(Qfd), d(Rd), d(x0_sim),
            None if id0 is None else id0.ctypes.data_as(C.POINTER(C.c_int64)), _abi.as_ip(nk)]
    tail = [st.ctypes.data_as(C.c_void_p), d(summary), nom.ctypes.data_as(C.c_void_p), d(K), d(Xs)]
    return lib, head, tail, dict(stats=st, summary=summary, nominal=nom, K=K, X_sim=Xs)


def attitude_ensemble(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0=None, sigma_scale=1.0,
                      want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2, min_steps=10, w_tol=0.05,
                      angle_tol=0.08727):
    """Track every solved slew under M noise realisations in ONE call (``tsat_tvlqr_ensemble``): the TVLQR gains once per
    slew, then M closed loops per slew on the noisy plant, one realisation per GPU lane — the failure probability and the
    slew-time spread of a plan, where src/monte_carlo.jl:199-262 draws a single realisation per slew.
    X (T,N,7), U (T,N-1,3) are the solved trajectories, x0_sim (T,M,7) the perturbed initial states
    (``ensemble_initial_states``). Realisation m of slew t draws generator id ``noise_id0[t] + m`` (default t M + m) under
    ``noise_seed``: it is the run ``attitude_simulation(..., x0_sim[:, m], noise_seed=noise_seed, noise_ids=noise_id0 + m)``
    makes. ``sigma_scale`` multiplies the reference's gyro and attitude noise levels. Returns dict(stats (T,M) records, summary (T,8) =
    [M, failures, mean / min / max slew time of the realisations that arrived, mean slew time of all, max final angle, max
    final rate], nominal (T,) statistic of the noise-free plant from X[:,0], K (T,N-1,6,3) or None, X_sim (T,M,N,7) or None)."""
    lib, head, tail, out = _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K,
                                          want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol)
    rc = lib.tsat_tvlqr_ensemble(*head, *tail)
    if rc != 0:
        raise RuntimeError(f"tsat_tvlqr_ensemble failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return out


PLANT_W = 21


def _rotation(v):
    """rotation matrix of the rotation vector v (rad), Rodrigues' formula; exactly I for v = 0"""
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(v, dtype=np.float64) / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def disperse_plant(Jmat, M, rng, inertia_rel=0.0, axes_deg=0.0, gain_rel=0.0, misalign_deg=0.0, residual_dipole=0.0):
    """Plants of M realisations per slew for ``attitude_ensemble_dispersed``, (T, M, 21) = [Jp (9), G (9), m_res (3)], around
    the model inertias Jmat ((T, 9) column-major as ``SlewBatch.Jmat``, or (T, 3, 3)):
      Jp    principal moments scaled by (1 + inertia_rel z), principal axes turned by a rotation vector of sigma axes_deg (per axis);
      G     R(rotation vector of sigma misalign_deg) diag(1 + gain_rel z): per-axis gain error behind a misaligned mounting;
      m_res residual dipole ~ N(0, residual_dipole^2) per axis, A m^2.
    z is standard normal clipped to +-3, so Jp stays positive definite for inertia_rel < 1/3 (larger is rejected); Jp is
    symmetrised exactly. All-zero levels return exactly (Jmat, I, 0). Every realisation consumes the same 15 normals per slew,
    realisation after realisation: the first M' realisations of a larger ensemble are the ensemble of size M'."""
    Jmat = np.asarray(Jmat, dtype=np.float64)
    if Jmat.ndim == 2 and Jmat.shape[1] == 9:
        Jmat = Jmat.reshape(-1, 3, 3).transpose(0, 2, 1)
    if Jmat.ndim != 3 or Jmat.shape[1:] != (3, 3):
        raise ValueError("Jmat must be (T, 9) or (T, 3, 3)")
    if not (0.0 <= inertia_rel < 1.0 / 3.0):
        raise ValueError("inertia_rel must be in [0, 1/3): with z clipped to +-3 a larger level can give a non-positive moment")
    if not (0.0 <= gain_rel < 1.0 / 3.0):
        raise ValueError("gain_rel must be in [0, 1/3)")
    if min(axes_deg, misalign_deg, residual_dipole) < 0.0:
        raise ValueError("dispersion levels must not be negative")
    T = Jmat.shape[0]
    out = np.zeros((T, int(M), PLANT_W))
    lam, V = (None, None) if inertia_rel == 0.0 and axes_deg == 0.0 else np.linalg.eigh(0.5 * (Jmat + Jmat.transpose(0, 2, 1)))
    for m in range(int(M)):
        z = rng.standard_normal((T, 15))
        zc = np.clip(z, -3.0, 3.0)
        for t in range(T):
            if lam is None:
                Jp = Jmat[t]
            else:
                A = _rotation(np.deg2rad(axes_deg) * z[t, 3:6]) @ V[t]
                Jp = (A * (lam[t] * (1.0 + inertia_rel * zc[t, 0:3]))) @ A.T
                Jp = 0.5 * (Jp + Jp.T)
            G = _rotation(np.deg2rad(misalign_deg) * z[t, 9:12]) * (1.0 + gain_rel * zc[t, 6:9])[None, :]
            out[t, m, 0:9] = Jp.T.reshape(9)              # column-major
            out[t, m, 9:18] = G.T.reshape(9)
            out[t, m, 18:21] = residual_dipole * z[t, 12:15]
    return out


def attitude_ensemble_dispersed(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant, sat=None, noise_id0=None,
                                sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                                min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """``attitude_ensemble`` with a plant of its own per realisation and the actuator's limit on the feedback command
    (``tsat_tvlqr_ensemble_dispersed``): the gains once per slew from the MODEL inertia ``batch.Jmat``, then realisation (t, m)
    flies inertia Jp, actuator matrix G and residual dipole m_res of ``plant[t, m]`` ((T, M, 21), ``disperse_plant``) under the
    command ``clip(U - K dX, lo, hi)``. ``sat`` = (lo, hi), each (T, 3) or (3,), in units of ``u_scale`` A m^2 — the plan's own
    box is ``(batch.ulo, batch.uhi)`` — or None for an unlimited command. Everything else as ``attitude_ensemble``; returns
    its dict plus ``n_clipped`` (T, M), the knots at which the limit changed the command. ``nominal`` is the noise-free MODEL
    plant under the same limits."""
    lib, head, tail, out = _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K,
                                          want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol)
    T, M = out["stats"].shape
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    plant = c(plant)
    if plant.shape != (T, M, PLANT_W):
        raise ValueError("plant must be (T, M, 21)")
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    ncl = np.zeros((T, M), dtype=np.int32)
    d = _abi.as_dp
    rc = lib.tsat_tvlqr_ensemble_dispersed(*head, d(plant), d(lo), d(hi), *tail, _abi.as_ip(ncl))
    if rc != 0:
        raise RuntimeError(f"tsat_tvlqr_ensemble_dispersed failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return dict(out, n_clipped=ncl)


GM_EARTH = 3.986004418e5    # km^3 / s^2


def orbit_table(batch, Rtab):
    """``Rtab`` as the C ABI takes it: (n_btab, n_tab, 3) float64, km, the shape of ``batch.Btab``"""
    Rtab = np.ascontiguousarray(Rtab, dtype=np.float64)
    if Rtab.shape != (batch.Btab.shape[0], batch.n_tab, 3):
        raise ValueError("Rtab must be (n_btab, n_tab, 3): one orbit position per field row")
    return Rtab


def attitude_ensemble_gg(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant, Rtab, gm=GM_EARTH, sat=None,
                         noise_id0=None, sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                         min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """``attitude_ensemble_dispersed`` under gravity-gradient torque (``tsat_tvlqr_ensemble_gg``): every realisation also feels
    3 gm / |r|^3 (r_b x Jp r_b) with its own inertia Jp, r_b the orbit position in the body frame — a disturbance neither the plan
    nor the gains know of. ``Rtab`` (n_btab, n_tab, 3) km holds the orbit position of every field row (``magnetic.orbit_rows``)
    and follows ``batch.btab_idx``; ``gm`` in km^3 / s^2, 0 switches the term off (then the result is that of
    ``attitude_ensemble_dispersed`` bit for bit). ``nominal`` is the noise-free MODEL plant in the same gravity field."""
    lib, head, tail, out = _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K,
                                          want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol)
    T, M = out["stats"].shape
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    plant = c(plant)
    if plant.shape != (T, M, PLANT_W):
        raise ValueError("plant must be (T, M, 21)")
    Rtab = orbit_table(batch, Rtab)
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    ncl = np.zeros((T, M), dtype=np.int32)
    d = _abi.as_dp
    rc = lib.tsat_tvlqr_ensemble_gg(*head, d(plant), d(lo), d(hi), *tail, _abi.as_ip(ncl), d(Rtab), float(gm))
    if rc != 0:
        raise RuntimeError(f"tsat_tvlqr_ensemble_gg failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return dict(out, n_clipped=ncl)


def pd_gains(Jmat, wn, zeta):
    """Per-axis gains of the projection PD law for a closed loop of natural frequency ``wn`` (rad/s) and damping ``zeta`` on the
    principal moments J_ii of ``Jmat`` ((T, 9) column-major as ``SlewBatch.Jmat``, or (T, 3, 3)); ``wn`` and ``zeta`` scalars or (T,).
    Returns (kd, kp), each (T, 3): kp = 2 J_ii wn^2 (the vector part of the error quaternion is half the angle), kd = 2 zeta wn J_ii."""
    Jmat = np.asarray(Jmat, dtype=np.float64)
    if Jmat.ndim == 2 and Jmat.shape[1] == 9:
        Jmat = Jmat.reshape(-1, 3, 3)
    if Jmat.ndim != 3 or Jmat.shape[1:] != (3, 3):
        raise ValueError("Jmat must be (T, 9) or (T, 3, 3)")
    Jd = np.stack([Jmat[:, 0, 0], Jmat[:, 1, 1], Jmat[:, 2, 2]], axis=1)
    wn = np.broadcast_to(np.asarray(wn, dtype=np.float64), (Jd.shape[0],))[:, None]
    zeta = np.broadcast_to(np.asarray(zeta, dtype=np.float64), (Jd.shape[0],))[:, None]
    return np.ascontiguousarray(2.0 * zeta * wn * Jd), np.ascontiguousarray(2.0 * Jd * wn * wn)


def attitude_ensemble_pd(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None, gm=0.0, sat=None,
                         limit_mode=0, x0_nom=None, noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2,
                         min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """The projection PD law on the plants of ``attitude_ensemble_gg`` (``tsat_pd_ensemble``): the baseline a tracked plan is
    compared against — no plan, gains or Riccati pass needed. Per knot T_req = -(kd dw + kp s e), m = (b x T_req) / |b|^2 with dw
    the rate error, e the vector part of conj(q_ref) (x) q, s the sign of its scalar part and b the body-frame field
    (include/tortoise_hip.h; the reference's src/comparison/psiaki_dynamics.jl:1-26).
    ``kd``, ``kp`` (T, 3) or (3,) in N m s / rad and N m (``pd_gains``). ``X`` (T, N, 7) is the trajectory to track, ``None``
    regulates to ``batch.xf`` over ``batch.N`` knots (nothing of size N goes to the device); ``U`` (T, N-1, 3) adds the plan's
    feed-forward (needs ``X``). ``plant`` (T, M, 21) or None for the model's plant; ``Rtab``, ``gm`` as ``attitude_ensemble_gg``
    (``Rtab=None`` needs gm = 0). ``sat`` as ``attitude_ensemble_dispersed``; ``limit_mode`` 0 clips each component, 1 scales the
    whole command back onto the box (needs lo < 0 < hi). ``x0_nom`` (T, 7) starts the noise-free MODEL plant (default X[:, 0];
    when regulating without it ``nominal`` is None). Returns dict(stats (T, M), summary (T, 8), nominal (T,) or None, X_sim
    (T, M, N, 7) or None, n_clipped (T, M))."""
    return _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                    want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol)


def _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0, want_trajectories,
             sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=None, filtering=None, aplqr=False, sun=None):
    """``tsat_pd_ensemble`` — with ``aplqr`` ``tsat_aplqr_ensemble``, ``kd`` being Kg (T, 6, 3) and ``kp`` rd —, or with ``sensing`` = (SensorOptions, sensor array or None) ``tsat_pd_ensemble_sensed``, or with
    ``filtering`` = (FilterOptions, X_hat or None, filt_final or None) besides ``tsat_pd_ensemble_filtered`` — with ModelFilterOptions
    in its place ``tsat_pd_ensemble_model_filtered``, with MagFilterOptions ``tsat_pd_ensemble_mag_filtered``, with
    MagBiasFilterOptions ``tsat_pd_ensemble_mag_bias_filtered``, with ModelMagFilterOptions ``tsat_pd_ensemble_model_mag_filtered``,
    with ModelMagSunFilterOptions and ``sun`` = (Stab or None, sigma_sun) ``tsat_pd_ensemble_model_mag_sun_filtered``"""
    lib = _abi.load()
    T, N = batch.T, batch.N
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    x0_sim = c(x0_sim)
    if x0_sim.ndim != 3 or x0_sim.shape[0] != T or x0_sim.shape[2] != 7:
        raise ValueError("x0_sim must be (T, M, 7)")
    M = x0_sim.shape[1]
    if aplqr:
        if kd is None or kp is None:
            raise ValueError("Kg and rd must be given")
        kd, kp = c(kd), c(np.broadcast_to(np.asarray(kp, dtype=np.float64), (T, 3)))
        if kd.shape != (T, 6, 3):
            raise ValueError("Kg must be (T, 6, 3)")
    else:
        kd, kp = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in (kd, kp))
    X, U, plant, x0_nom = c(X), c(U), c(plant), c(x0_nom)
    if U is not None and X is None:
        raise ValueError("the feed-forward U needs the trajectory X it belongs to")
    if (X is not None and X.shape != (T, N, 7)) or (U is not None and U.shape != (T, N - 1, 3)):
        raise ValueError("array shapes do not match the batch")
    if plant is not None and plant.shape != (T, M, PLANT_W):
        raise ValueError("plant must be (T, M, 21)")
    if x0_nom is not None and x0_nom.shape != (T, 7):
        raise ValueError("x0_nom must be (T, 7)")
    if Rtab is not None:
        Rtab = orbit_table(batch, Rtab)
    o = _abi.TvlqrOptions()
    lib.tsat_tvlqr_default_options(C.byref(o))
    o.n_knots, o.n_tab, o.min_steps = N, batch.n_tab, int(min_steps)
    o.u_scale, o.w_tol, o.angle_tol = float(u_scale), float(w_tol), float(angle_tol)
    o.noise_mode, o.noise_seed = 1, int(noise_seed)
    o.sigma_gyro, o.sigma_att = o.sigma_gyro * float(sigma_scale), o.sigma_att * float(sigma_scale)
    id0 = None if noise_id0 is None else np.ascontiguousarray(noise_id0, dtype=np.int64)
    if id0 is not None and id0.shape != (T,):
        raise ValueError("noise_id0 must be (T,)")
    nk = None if batch.n_knots is None else np.ascontiguousarray(batch.n_knots, dtype=np.int32)
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    st = np.zeros((T, M), dtype=_abi.TVLQR_STATS_DTYPE)
    nom = np.zeros(T, dtype=_abi.TVLQR_STATS_DTYPE) if (X is not None or x0_nom is not None) else None
    summary = np.zeros((T, 8))
    Xs = np.empty((T, M, N, 7)) if want_trajectories else None
    ncl = np.zeros((T, M), dtype=np.int32)
    d = _abi.as_dp
    args = (solver._h, C.byref(o), T, batch.Btab.shape[0], M, d(X), d(U), d(batch.xf), d(batch.Btab),
            _abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(kd), d(kp),
            0 if U is None else 1, int(limit_mode), d(x0_sim), d(x0_nom),
            None if id0 is None else id0.ctypes.data_as(C.POINTER(C.c_int64)), _abi.as_ip(nk), d(plant), d(lo), d(hi),
            st.ctypes.data_as(C.c_void_p), d(summary), None if nom is None else nom.ctypes.data_as(C.c_void_p), d(Xs),
            _abi.as_ip(ncl), d(Rtab), float(gm))
    if aplqr:
        name, rc = "tsat_aplqr_ensemble", lib.tsat_aplqr_ensemble(*args)
    elif sensing is None:
        name, rc = "tsat_pd_ensemble", lib.tsat_pd_ensemble(*args)
    elif filtering is not None:
        name = {_abi.ModelFilterOptions: "tsat_pd_ensemble_model_filtered", _abi.MagFilterOptions: "tsat_pd_ensemble_mag_filtered",
                _abi.MagBiasFilterOptions: "tsat_pd_ensemble_mag_bias_filtered",
                _abi.ModelMagFilterOptions: "tsat_pd_ensemble_model_mag_filtered",
                _abi.ModelMagSunFilterOptions: "tsat_pd_ensemble_model_mag_sun_filtered"}.get(type(filtering[0]), "tsat_pd_ensemble_filtered")
        rc = getattr(lib, name)(*args, C.byref(sensing[0]), d(sensing[1]), C.byref(filtering[0]), d(filtering[1]), d(filtering[2]),
                                *([] if sun is None else [d(sun[0]), float(sun[1])]))
    else:
        name, rc = "tsat_pd_ensemble_sensed", lib.tsat_pd_ensemble_sensed(*args, C.byref(sensing[0]), d(sensing[1]))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return dict(stats=st, summary=summary, nominal=nom, X_sim=Xs, n_clipped=ncl)


#: default ``res_tol`` of ``aplqr_gains``: 100 x the largest relative residual a numpy-double restatement of the sign iteration
#: leaves on the cases of tests/test_aplqr.py, 3.26e-14 (profiles/aplqr/care_e_ref.txt)
APLQR_RES_TOL = 3.3e-12


def aplqr_gains(solver, batch: SlewBatch, qd, rd, alpha=1.0, rows=None, res_tol=APLQR_RES_TOL, allow_failed=False):
    """Gains of the asymptotic periodic LQR (``tsat_aplqr_gains``), one wavefront per slew on the device: the control-effectiveness
    Gramian Gamma = mean_j B_j diag(1/rd) B_j', B_j = -inv(J) hat(beta_j), beta_j the field rows ``rows`` = (lo, hi) — ints or
    (T,) arrays, default the whole table — rotated into the goal's body frame; P of A'P + P A - P G P + diag(qd) = 0 on the
    double integrator with G = blockdiag(0, Gamma); Kg = alpha inv(J) P[3:6, :] (include/tortoise_hip.h; the reference's
    src/comparison/psiaki_dynamics.jl:75-125). ``qd`` (T, 6) or (6,) weights [theta (3); dw (3)], ``rd`` (T, 3) or (3,), ``alpha``
    scalar or (T,). Returns (Kg (T, 6, 3), info) with info = dict(status, iterations, residual, pivot_min (T,) each, P (T, 6, 6),
    Gamma (T, 3, 3)). A non-zero status (1 not converged, 2 singular elimination, 3 residual > res_tol) raises unless
    ``allow_failed``; the Kg and P of such a slew are zero."""
    lib = _abi.load()
    T = batch.T
    c = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))
    qd, rd, alpha = c(qd, (T, 6)), c(rd, (T, 3)), c(alpha, (T,))
    lo = hi = None
    if rows is not None:
        lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v), (T,)), dtype=np.int32) for v in rows)
    Kg, P, Gm = np.zeros((T, 6, 3)), np.zeros((T, 6, 6)), np.zeros((T, 3, 3))
    info = np.zeros(T, dtype=_abi.APLQR_INFO_DTYPE)
    d = _abi.as_dp
    rc = lib.tsat_aplqr_gains(solver._h, T, batch.Btab.shape[0], batch.n_tab, d(batch.xf), d(batch.Btab), _abi.as_ip(batch.btab_idx),
                              _abi.as_ip(lo), _abi.as_ip(hi), d(batch.Jmat), d(qd), d(rd), d(alpha), float(res_tol), d(Kg), d(P), d(Gm),
                              info.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"tsat_aplqr_gains failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    if info["status"].any() and not allow_failed:
        t = int(np.flatnonzero(info["status"])[0])
        raise RuntimeError(f"tsat_aplqr_gains: slew {t} has status {int(info['status'][t])} after {int(info['iterations'][t])} iterations "
                           f"(residual {float(info['residual'][t]):.2e}, smallest pivot {float(info['pivot_min'][t]):.2e})")
    return Kg, dict(status=info["status"].copy(), iterations=info["iterations"].copy(), residual=info["residual"].copy(),
                    pivot_min=info["pivot_min"].copy(), P=P, Gamma=Gm)


def attitude_ensemble_aplqr(solver, batch: SlewBatch, x0_sim, Kg, rd, noise_seed, X=None, U=None, plant=None, Rtab=None, gm=0.0, sat=None,
                            limit_mode=0, x0_nom=None, noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2,
                            min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """The asymptotic periodic LQR on the plants of ``attitude_ensemble_pd`` (``tsat_aplqr_ensemble``): per knot
    m = -diag(1/rd) (b x Kg [theta; dw]) with theta = 2 s e the rotation-vector error, dw the rate error and b the body-frame field.
    ``Kg`` (T, 6, 3) from ``aplqr_gains`` or the caller's own, ``rd`` (T, 3) or (3,). Every other keyword and the returned dict are
    those of ``attitude_ensemble_pd``."""
    return _pd_call(solver, batch, x0_sim, Kg, rd, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                    want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, aplqr=True)


SENSOR_W = 9
#: the reference's gyro and attitude figures read UN-SQUARED (src/simulator.jl:5,10): 0.38 deg (rad/s) and 1 deg (rad)
SENSOR_SIGMA_GYRO = 0.38 * np.pi / 180.0
SENSOR_SIGMA_ATT = 1.0 * np.pi / 180.0


def disperse_sensor(T, M, rng, gyro_bias=0.0, att_bias_deg=0.0, mag_bias=0.0):
    """Sensor biases of M realisations per slew for the sensed ensembles, (T, M, 9) = [bw (3, rad/s), ba (3, rotation vector, rad,
    body frame), bm (3, units of the field table)]: normal per axis with sigma ``gyro_bias``, ``att_bias_deg`` (degrees) and
    ``mag_bias``. All-zero levels return exactly zeros. Every realisation consumes the same 9 normals per slew, realisation after
    realisation, as ``disperse_plant``: the first M' realisations of a larger ensemble are the ensemble of size M'."""
    if min(gyro_bias, att_bias_deg, mag_bias) < 0.0:
        raise ValueError("bias levels must not be negative")
    out = np.zeros((int(T), int(M), SENSOR_W))
    lev = np.repeat([float(gyro_bias), float(np.deg2rad(att_bias_deg)), float(mag_bias)], 3)
    for m in range(int(M)):
        out[:, m, :] = lev * rng.standard_normal((int(T), SENSOR_W))
    return out


def _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency):
    """(SensorOptions, biases (T, M, 9) or None) of a sensed call"""
    so = _abi.SensorOptions()
    _abi.load().tsat_sensor_default_options(C.byref(so))
    so.sigma_gyro, so.sigma_att, so.sigma_mag, so.latency = float(sigma_gyro), float(sigma_att), float(sigma_mag), int(latency)
    if sensor is not None:
        sensor = np.ascontiguousarray(sensor, dtype=np.float64)
        if sensor.shape != (T, M, SENSOR_W):
            raise ValueError("sensor must be (T, M, 9)")
    return so, sensor


def attitude_ensemble_sensed(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0, sat=None,
                             sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None, sigma_scale=1.0,
                             want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2, min_steps=10, w_tol=0.05,
                             angle_tol=0.08727):
    """``attitude_ensemble_gg`` with the TVLQR feedback reading a MEASUREMENT of the state instead of the state
    (``tsat_tvlqr_ensemble_sensed``): w_m = w + bw + n_w and q_m = q (x) dq(ba + n_a) per knot, with the biases of ``sensor``
    ((T, M, 9), ``disperse_sensor``; None: zeros), white noise of ``sigma_gyro`` (rad/s) and ``sigma_att`` (rad) drawn in the kernel
    from the realisation's generator id, and ``latency`` 0 or 1 knots between measurement and command (include/tortoise_hip.h).
    ``sigma_mag`` is accepted for symmetry with ``attitude_ensemble_pd_sensed``: this law reads no magnetometer. ``plant`` None
    flies the model's plant, ``Rtab`` None (needs gm = 0) no gravity-gradient term. The plant, the statistic and ``X_sim`` are the
    TRUE states; ``nominal`` flies the ideal sensor at the same latency. Returns the dict of ``attitude_ensemble_gg``."""
    lib, head, tail, out = _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K,
                                          want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol)
    T, M = out["stats"].shape
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    plant = c(plant)
    if plant is not None and plant.shape != (T, M, PLANT_W):
        raise ValueError("plant must be (T, M, 21)")
    if Rtab is not None:
        Rtab = orbit_table(batch, Rtab)
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    so, sensor = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    ncl = np.zeros((T, M), dtype=np.int32)
    d = _abi.as_dp
    rc = lib.tsat_tvlqr_ensemble_sensed(*head, d(plant), d(lo), d(hi), *tail, _abi.as_ip(ncl), d(Rtab), float(gm), C.byref(so), d(sensor))
    if rc != 0:
        raise RuntimeError(f"tsat_tvlqr_ensemble_sensed failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return dict(out, n_clipped=ncl)


def attitude_ensemble_pd_sensed(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None, gm=0.0,
                                sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0,
                                noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2, min_steps=10, w_tol=0.05,
                                angle_tol=0.08727):
    """``attitude_ensemble_pd`` with the law reading MEASUREMENTS (``tsat_pd_ensemble_sensed``): rate and attitude errors from
    (w_m, q_m) as ``attitude_ensemble_sensed``, and the body-frame field from a magnetometer, b_m = (true body field) + bm + n_m
    with noise of ``sigma_mag`` (units of the field table). ``sensor``, ``sigma_*`` and ``latency`` as there; everything else and
    the returned dict as ``attitude_ensemble_pd``."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    sensing = _sensing(batch.T, x0.shape[1], sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    return _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                    want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing)


FILTER_W = 9


def filter_options(sigma_v, sigma_a, sigma_u=0.0, p0_att=None, p0_bias=0.0):
    """The ``tsat_filter_options`` of the filtered ensembles: what the multiplicative EKF assumes, all standard deviations — gyro
    white noise ``sigma_v`` (rad/s), attitude measurement noise ``sigma_a`` (rad, > 0), bias random walk per knot ``sigma_u``
    (rad/s), initial attitude ``p0_att`` (rad; None: ``sigma_a``) and initial bias ``p0_bias`` (rad/s). ``p0_bias`` = ``sigma_u`` = 0
    estimates no bias at all."""
    fo = _abi.FilterOptions()
    _abi.load().tsat_filter_default_options(C.byref(fo))
    fo.sigma_v, fo.sigma_a, fo.sigma_u = float(sigma_v), float(sigma_a), float(sigma_u)
    fo.p0_att, fo.p0_bias = float(sigma_a if p0_att is None else p0_att), float(p0_bias)
    if min(fo.sigma_v, fo.sigma_u, fo.p0_att, fo.p0_bias) < 0.0 or not fo.sigma_a > 0.0:
        raise ValueError("filter levels must not be negative, and sigma_a must be positive")
    return fo


def _filtering(T, M, N, filter, want_estimates):
    """(FilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 9)) of a filtered call; ``filter`` None: the default options"""
    if filter is None:
        filter = _abi.FilterOptions()
        _abi.load().tsat_filter_default_options(C.byref(filter))
    if not isinstance(filter, _abi.FilterOptions):
        raise ValueError("filter must come from filter_options()")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, FILTER_W))


def attitude_ensemble_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0, sat=None,
                               sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None, sigma_scale=1.0,
                               want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2, min_steps=10, w_tol=0.05,
                               angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_sensed`` with a multiplicative EKF between the measurement and the TVLQR feedback
    (``tsat_tvlqr_ensemble_filtered``): six states — attitude error and gyro bias —, propagated by the gyro, updated by the attitude
    measurement; the recursion is in include/tortoise_hip.h. It removes attitude-sensor noise and estimates the gyro bias; it does
    NOT smooth white gyro noise (the rate the law sees is w_m - b^). At ``latency`` 1 the law sees the estimate predicted across the
    delay. ``filter`` from ``filter_options`` (None: the reference's figures, sigma_v = 0.38 deg/s, sigma_a = p0_att = 1 deg, no bias
    state). Returns the dict of ``attitude_ensemble_sensed`` plus ``filt_final`` (T, M, 9) = [b^, sqrt(diag A), sqrt(diag D)] after
    the last sample processed and ``X_hat`` (T, M, N, 7), what the law saw per knot (zero from the slew's last knot on), or None
    without ``want_estimates``. ``nominal`` flies the ideal sensor through the same filter."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_filtered", _filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant, Rtab, gm,
                             sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0, sigma_scale, want_K, want_trajectories,
                             linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter, want_estimates)


def _tv_filtered_call(name, filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant, Rtab, gm, sat, sensor, sigma_gyro,
                      sigma_att, sigma_mag, latency, noise_id0, sigma_scale, want_K, want_trajectories, linearize_dt_sq, u_scale,
                      min_steps, w_tol, angle_tol, filter, want_estimates, sun=None):
    """``tsat_tvlqr_ensemble_filtered`` or ``tsat_tvlqr_ensemble_model_filtered`` (``name``), ``filtering`` the function that makes
    the call's (options, X_hat, filt_final); ``sun`` = (Stab or None, sigma_sun): the two arguments a sun-sensor call ends with"""
    lib, head, tail, out = _ensemble_call(solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, noise_id0, sigma_scale, want_K,
                                          want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol)
    T, M = out["stats"].shape
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    plant = c(plant)
    if plant is not None and plant.shape != (T, M, PLANT_W):
        raise ValueError("plant must be (T, M, 21)")
    if Rtab is not None:
        Rtab = orbit_table(batch, Rtab)
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    so, sensor = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = filtering(T, M, batch.N, filter, want_estimates)
    ncl = np.zeros((T, M), dtype=np.int32)
    d = _abi.as_dp
    rc = getattr(lib, name)(*head, d(plant), d(lo), d(hi), *tail, _abi.as_ip(ncl), d(Rtab), float(gm), C.byref(so), d(sensor),
                            C.byref(fo), d(Xh), d(ff), *([] if sun is None else [d(sun[0]), float(sun[1])]))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}: {lib.tsat_ensemble_last_error().decode()}")
    return dict(out, n_clipped=ncl, X_hat=Xh, filt_final=ff)


def attitude_ensemble_pd_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None, gm=0.0,
                                  sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0,
                                  latency=0, noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2, min_steps=10,
                                  w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_pd_sensed`` with the filter of ``attitude_ensemble_filtered`` between (w_m, q_m) and the law
    (``tsat_pd_ensemble_filtered``); the magnetometer reading b_m is not filtered. Returns the dict of ``attitude_ensemble_pd_sensed``
    plus ``X_hat`` and ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff))
    return dict(out, X_hat=Xh, filt_final=ff)


MODEL_FILTER_W = 12


def model_filter_options(sigma_w, sigma_g, sigma_a, sigma_v=0.0, sigma_u=0.0, p0_att=None, p0_bias=0.0):
    """The ``tsat_model_filter_options`` of the model-filtered ensembles: what the nine-state multiplicative EKF assumes, all
    standard deviations — un-modelled angular acceleration ``sigma_w`` (rad/s^2; it has no default: it has to cover what the
    filter's model leaves out — inertia and actuator mismatch, residual dipole, gravity gradient, plant noise), gyro measurement
    noise ``sigma_g`` (rad/s, > 0), attitude measurement noise ``sigma_a`` (rad, > 0), attitude process noise ``sigma_v`` (rad/s),
    bias random walk per knot ``sigma_u`` (rad/s), initial attitude ``p0_att`` (rad; None: ``sigma_a``) and initial bias
    ``p0_bias`` (rad/s)."""
    fo = _abi.ModelFilterOptions()
    _abi.load().tsat_model_filter_default_options(C.byref(fo))
    fo.sigma_w, fo.sigma_g, fo.sigma_a, fo.sigma_v, fo.sigma_u = float(sigma_w), float(sigma_g), float(sigma_a), float(sigma_v), float(sigma_u)
    fo.p0_att, fo.p0_bias = float(sigma_a if p0_att is None else p0_att), float(p0_bias)
    if min(fo.sigma_w, fo.sigma_v, fo.sigma_u, fo.p0_att, fo.p0_bias) < 0.0 or not fo.sigma_a > 0.0 or not fo.sigma_g > 0.0:
        raise ValueError("filter levels must not be negative, and sigma_a and sigma_g must be positive")
    if not all(np.isfinite([fo.sigma_w, fo.sigma_v, fo.sigma_u, fo.sigma_a, fo.sigma_g, fo.p0_att, fo.p0_bias])):
        raise ValueError("filter levels must be finite")
    return fo


def _model_filtering(T, M, N, filter, want_estimates):
    """(ModelFilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 12)) of a model-filtered call"""
    if not isinstance(filter, _abi.ModelFilterOptions):
        raise ValueError("filter must come from model_filter_options(): sigma_w has no default")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, MODEL_FILTER_W))


def attitude_ensemble_model_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0,
                                     sat=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None,
                                     sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                                     min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_sensed`` with a MODEL-BASED rate filter between the measurement and the TVLQR feedback
    (``tsat_tvlqr_ensemble_model_filtered``): nine states — attitude error, body rate and gyro bias —, rate and attitude propagated
    by the model's plant under the command the law has just issued, the gyro and the attitude sensor as measurements; the recursion
    is in include/tortoise_hip.h. Unlike ``attitude_ensemble_filtered`` it smooths white gyro noise. At ``latency`` 1 the law sees
    the model prediction across the delay. ``filter`` from ``model_filter_options`` (required: ``sigma_w`` has no default). Returns
    the dict of ``attitude_ensemble_filtered`` with ``filt_final`` (T, M, 12) = [b^, sqrt(diag P_tt), sqrt(diag P_ww),
    sqrt(diag P_bb)] after the last update made."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_model_filtered", _model_filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed,
                             plant, Rtab, gm, sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0, sigma_scale, want_K,
                             want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter, want_estimates)


def attitude_ensemble_pd_model_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None,
                                        gm=0.0, sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0,
                                        sigma_mag=0.0, latency=0, noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2,
                                        min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_pd_sensed`` with the filter of ``attitude_ensemble_model_filtered`` between (w_m, q_m) and the law
    (``tsat_pd_ensemble_model_filtered``); the magnetometer reading b_m is not filtered. Returns the dict of
    ``attitude_ensemble_pd_sensed`` plus ``X_hat`` and ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _model_filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff))
    return dict(out, X_hat=Xh, filt_final=ff)


def mag_filter_options(sigma_v, sigma_m, sigma_u=0.0, p0_att=None, p0_bias=0.0):
    """The ``tsat_mag_filter_options`` of the mag-filtered ensembles: what the magnetometer-updated EKF assumes, all standard
    deviations — gyro white noise ``sigma_v`` (rad/s), magnetometer noise ``sigma_m`` (units of the field table, > 0; it has no
    default), bias random walk per knot ``sigma_u`` (rad/s), initial attitude ``p0_att`` (rad; None: the default options' 1 deg, the
    accuracy of the one attitude fix) and initial bias ``p0_bias`` (rad/s)."""
    fo = _abi.MagFilterOptions()
    _abi.load().tsat_mag_filter_default_options(C.byref(fo))
    fo.sigma_v, fo.sigma_m, fo.sigma_u = float(sigma_v), float(sigma_m), float(sigma_u)
    fo.p0_att, fo.p0_bias = float(fo.p0_att if p0_att is None else p0_att), float(p0_bias)
    if min(fo.sigma_v, fo.sigma_u, fo.p0_att, fo.p0_bias) < 0.0 or not fo.sigma_m > 0.0:
        raise ValueError("filter levels must not be negative, and sigma_m must be positive")
    if not all(np.isfinite([fo.sigma_v, fo.sigma_m, fo.sigma_u, fo.p0_att, fo.p0_bias])):
        raise ValueError("filter levels must be finite")
    return fo


def _mag_filtering(T, M, N, filter, want_estimates):
    """(MagFilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 9)) of a mag-filtered call"""
    if not isinstance(filter, _abi.MagFilterOptions):
        raise ValueError("filter must come from mag_filter_options(): sigma_m has no default")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, FILTER_W))


def attitude_ensemble_mag_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0,
                                   sat=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None,
                                   sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                                   min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_filtered`` with the attitude update replaced by a MAGNETOMETER update
    (``tsat_tvlqr_ensemble_mag_filtered``): the attitude measurement is used once, at knot 0; from then on the gyro-propagated
    estimate is corrected by the magnetometer reading b_m (noise ``sigma_mag``, the magnetometer bias of ``sensor``) against the
    slew's field table; the recursion is in include/tortoise_hip.h. The magnetometer bias is not estimated. ``filter`` from
    ``mag_filter_options`` (required: ``sigma_m`` has no default). Returns the dict of ``attitude_ensemble_filtered``."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_mag_filtered", _mag_filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed,
                             plant, Rtab, gm, sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0, sigma_scale, want_K,
                             want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter, want_estimates)


def attitude_ensemble_pd_mag_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None,
                                      gm=0.0, sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0,
                                      sigma_mag=0.0, latency=0, noise_id0=None, want_trajectories=False, sigma_scale=1.0, u_scale=1e-2,
                                      min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_pd_sensed`` with the filter of ``attitude_ensemble_mag_filtered`` between the measurement and the law
    (``tsat_pd_ensemble_mag_filtered``); the law's field reading is the very magnetometer sample the filter used, taken once per
    knot. Returns the dict of ``attitude_ensemble_pd_sensed`` plus ``X_hat`` and ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _mag_filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff))
    return dict(out, X_hat=Xh, filt_final=ff)


MAG_BIAS_FILTER_W = 15


def mag_bias_filter_options(sigma_v, sigma_m, sigma_u=0.0, sigma_c=0.0, p0_att=None, p0_bias=0.0, p0_mag=0.0):
    """The ``tsat_mag_bias_filter_options`` of the mag-bias-filtered ensembles: ``mag_filter_options`` and, for the magnetometer-bias
    state, its random walk per knot ``sigma_c`` and its initial standard deviation ``p0_mag`` (both in the units of the field
    table). ``p0_mag`` = ``sigma_c`` = 0 estimates no magnetometer bias: the filter is then ``mag_filter_options``'."""
    fo = _abi.MagBiasFilterOptions()
    _abi.load().tsat_mag_bias_filter_default_options(C.byref(fo))
    fo.sigma_v, fo.sigma_m, fo.sigma_u, fo.sigma_c = float(sigma_v), float(sigma_m), float(sigma_u), float(sigma_c)
    fo.p0_att, fo.p0_bias, fo.p0_mag = float(fo.p0_att if p0_att is None else p0_att), float(p0_bias), float(p0_mag)
    if min(fo.sigma_v, fo.sigma_u, fo.sigma_c, fo.p0_att, fo.p0_bias, fo.p0_mag) < 0.0 or not fo.sigma_m > 0.0:
        raise ValueError("filter levels must not be negative, and sigma_m must be positive")
    if not all(np.isfinite([fo.sigma_v, fo.sigma_m, fo.sigma_u, fo.sigma_c, fo.p0_att, fo.p0_bias, fo.p0_mag])):
        raise ValueError("filter levels must be finite")
    return fo


def _mag_bias_filtering(T, M, N, filter, want_estimates):
    """(MagBiasFilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 15)) of a mag-bias-filtered call"""
    if not isinstance(filter, _abi.MagBiasFilterOptions):
        raise ValueError("filter must come from mag_bias_filter_options(): sigma_m has no default")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, MAG_BIAS_FILTER_W))


def attitude_ensemble_mag_bias_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0,
                                        sat=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None,
                                        sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                                        min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_mag_filtered`` with the MAGNETOMETER BIAS ESTIMATED (``tsat_tvlqr_ensemble_mag_bias_filtered``): nine
    error states — attitude error, gyro bias, magnetometer bias —, the measurement z = b_m - c^ - (predicted field); the recursion is
    in include/tortoise_hip.h. ``filter`` from ``mag_bias_filter_options`` (required: ``sigma_m`` has no default). Returns the dict
    of ``attitude_ensemble_mag_filtered`` with ``filt_final`` (T, M, 15) = [b^, sqrt(diag A), sqrt(diag D), c^, sqrt(diag M)] after
    the last sample processed."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_mag_bias_filtered", _mag_bias_filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd,
                             noise_seed, plant, Rtab, gm, sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0, sigma_scale,
                             want_K, want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter, want_estimates)


def attitude_ensemble_pd_mag_bias_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None,
                                           gm=0.0, sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0,
                                           sigma_mag=0.0, latency=0, noise_id0=None, want_trajectories=False, sigma_scale=1.0,
                                           u_scale=1e-2, min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_pd_sensed`` with the filter of ``attitude_ensemble_mag_bias_filtered`` between the measurement and the law
    (``tsat_pd_ensemble_mag_bias_filtered``); the law's field reading is the raw magnetometer sample the filter used, taken once per
    knot and not corrected by c^. Returns the dict of ``attitude_ensemble_pd_sensed`` plus ``X_hat`` and ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _mag_bias_filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff))
    return dict(out, X_hat=Xh, filt_final=ff)


MODEL_MAG_FILTER_W = 12


def model_mag_filter_options(sigma_w, sigma_g, sigma_m, sigma_v=0.0, sigma_u=0.0, p0_att=None, p0_bias=0.0):
    """The ``tsat_model_mag_filter_options`` of the model-mag-filtered ensembles: ``model_filter_options`` without the attitude
    sensor's ``sigma_a`` and with the magnetometer noise the filter assumes, ``sigma_m`` (units of the field table, > 0; it has no
    default, and neither has ``sigma_w``). ``p0_att`` (rad; None: the default options' 1 deg) is the accuracy of the one attitude
    fix."""
    fo = _abi.ModelMagFilterOptions()
    _abi.load().tsat_model_mag_filter_default_options(C.byref(fo))
    fo.sigma_w, fo.sigma_g, fo.sigma_m, fo.sigma_v, fo.sigma_u = float(sigma_w), float(sigma_g), float(sigma_m), float(sigma_v), float(sigma_u)
    fo.p0_att, fo.p0_bias = float(fo.p0_att if p0_att is None else p0_att), float(p0_bias)
    if min(fo.sigma_w, fo.sigma_v, fo.sigma_u, fo.p0_att, fo.p0_bias) < 0.0 or not fo.sigma_g > 0.0 or not fo.sigma_m > 0.0:
        raise ValueError("filter levels must not be negative, and sigma_g and sigma_m must be positive")
    if not all(np.isfinite([fo.sigma_w, fo.sigma_v, fo.sigma_u, fo.sigma_g, fo.sigma_m, fo.p0_att, fo.p0_bias])):
        raise ValueError("filter levels must be finite")
    return fo


def _model_mag_filtering(T, M, N, filter, want_estimates):
    """(ModelMagFilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 12)) of a model-mag-filtered call"""
    if not isinstance(filter, _abi.ModelMagFilterOptions):
        raise ValueError("filter must come from model_mag_filter_options(): sigma_w and sigma_m have no default")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, MODEL_MAG_FILTER_W))


def attitude_ensemble_model_mag_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None, gm=0.0,
                                         sat=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None,
                                         sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True, u_scale=1e-2,
                                         min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_model_filtered`` with the attitude update replaced by a MAGNETOMETER update
    (``tsat_tvlqr_ensemble_model_mag_filtered``): the attitude measurement is used once, at knot 0; rate and attitude are propagated
    on the model under the command just issued, the attitude is corrected by the magnetometer reading b_m against the slew's field
    table and the gyro is a measurement of w^ + b^; the recursion is in include/tortoise_hip.h. ``filter`` from
    ``model_mag_filter_options`` (required). Returns the dict of ``attitude_ensemble_model_filtered``."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_model_mag_filtered", _model_mag_filtering, solver, batch, X, U, x0_sim, Qd, Qfd, Rd,
                             noise_seed, plant, Rtab, gm, sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0, sigma_scale,
                             want_K, want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter, want_estimates)


def attitude_ensemble_pd_model_mag_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None, Rtab=None,
                                            gm=0.0, sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0,
                                            sigma_mag=0.0, latency=0, noise_id0=None, want_trajectories=False, sigma_scale=1.0,
                                            u_scale=1e-2, min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False):
    """``attitude_ensemble_pd_sensed`` with the filter of ``attitude_ensemble_model_mag_filtered`` between the measurement and the
    law (``tsat_pd_ensemble_model_mag_filtered``); the law's field reading is the very magnetometer sample the filter used, taken
    once per knot. Returns the dict of ``attitude_ensemble_pd_sensed`` plus ``X_hat`` and ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _model_mag_filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff))
    return dict(out, X_hat=Xh, filt_final=ff)


def model_mag_sun_filter_options(sigma_w, sigma_g, sigma_m, sigma_s, sigma_v=0.0, sigma_u=0.0, p0_att=None, p0_bias=0.0):
    """The ``tsat_model_mag_sun_filter_options`` of the model-mag-sun-filtered ensembles: ``model_mag_filter_options`` and the
    sun-sensor noise the filter assumes, ``sigma_s`` (dimensionless, radians for small angles, > 0; it has no default)."""
    g = model_mag_filter_options(sigma_w, sigma_g, sigma_m, sigma_v, sigma_u, p0_att, p0_bias)
    if not (np.isfinite(sigma_s) and float(sigma_s) > 0.0):
        raise ValueError("sigma_s must be finite and positive")
    return _abi.ModelMagSunFilterOptions(sigma_v=g.sigma_v, sigma_w=g.sigma_w, sigma_u=g.sigma_u, sigma_g=g.sigma_g, sigma_m=g.sigma_m,
                                         sigma_s=float(sigma_s), p0_att=g.p0_att, p0_bias=g.p0_bias, reserved=0)


def _model_mag_sun_filtering(T, M, N, filter, want_estimates):
    """(ModelMagSunFilterOptions, X_hat (T, M, N, 7) or None, filt_final (T, M, 12)) of a model-mag-sun-filtered call"""
    if not isinstance(filter, _abi.ModelMagSunFilterOptions):
        raise ValueError("filter must come from model_mag_sun_filter_options(): sigma_w, sigma_m and sigma_s have no default")
    return filter, (np.empty((T, M, N, 7)) if want_estimates else None), np.empty((T, M, MODEL_MAG_FILTER_W))


def _sun(batch, Stab, sigma_sun):
    """(Stab (n_btab, n_tab, 3) contiguous or None, sigma_sun) of a model-mag-sun-filtered call"""
    if Stab is None:
        if float(sigma_sun) != 0.0:
            raise ValueError("sigma_sun needs the sun table Stab")
        return None, 0.0
    Stab = np.ascontiguousarray(Stab, dtype=np.float64)
    if Stab.shape != (batch.Btab.shape[0], batch.n_tab, 3):
        raise ValueError("Stab must be (n_btab, n_tab, 3), indexed like the first n_tab rows of the field tables")
    if not (np.isfinite(sigma_sun) and float(sigma_sun) >= 0.0):
        raise ValueError("sigma_sun must be finite and not negative")
    return Stab, float(sigma_sun)


def attitude_ensemble_model_mag_sun_filtered(solver, batch: SlewBatch, X, U, x0_sim, Qd, Qfd, Rd, noise_seed, plant=None, Rtab=None,
                                             gm=0.0, sat=None, sensor=None, sigma_gyro=0.0, sigma_att=0.0, sigma_mag=0.0, latency=0,
                                             noise_id0=None, sigma_scale=1.0, want_K=False, want_trajectories=False, linearize_dt_sq=True,
                                             u_scale=1e-2, min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None, want_estimates=False,
                                             Stab=None, sigma_sun=0.0):
    """``attitude_ensemble_model_mag_filtered`` with a SUN SENSOR (``tsat_tvlqr_ensemble_model_mag_sun_filtered``): per knot one sun
    sample at noise ``sigma_sun`` (dimensionless) against the sun table ``Stab`` (n_btab, n_tab, 3; ``magnetic.sun_rows``), whose
    zero rows are eclipse — no sample and no update there; the recursion is in include/tortoise_hip.h. ``filter`` from
    ``model_mag_sun_filter_options`` (required). ``Stab`` None is the model-mag-filtered call. Returns its dict."""
    return _tv_filtered_call("tsat_tvlqr_ensemble_model_mag_sun_filtered", _model_mag_sun_filtering, solver, batch, X, U, x0_sim, Qd, Qfd,
                             Rd, noise_seed, plant, Rtab, gm, sat, sensor, sigma_gyro, sigma_att, sigma_mag, latency, noise_id0,
                             sigma_scale, want_K, want_trajectories, linearize_dt_sq, u_scale, min_steps, w_tol, angle_tol, filter,
                             want_estimates, sun=_sun(batch, Stab, sigma_sun))


def attitude_ensemble_pd_model_mag_sun_filtered(solver, batch: SlewBatch, x0_sim, kd, kp, noise_seed, X=None, U=None, plant=None,
                                                Rtab=None, gm=0.0, sat=None, limit_mode=0, x0_nom=None, sensor=None, sigma_gyro=0.0,
                                                sigma_att=0.0, sigma_mag=0.0, latency=0, noise_id0=None, want_trajectories=False,
                                                sigma_scale=1.0, u_scale=1e-2, min_steps=10, w_tol=0.05, angle_tol=0.08727, filter=None,
                                                want_estimates=False, Stab=None, sigma_sun=0.0):
    """``attitude_ensemble_pd_model_mag_filtered`` with the sun sensor of ``attitude_ensemble_model_mag_sun_filtered``
    (``tsat_pd_ensemble_model_mag_sun_filtered``). Returns the dict of ``attitude_ensemble_pd_sensed`` plus ``X_hat`` and
    ``filt_final`` as there."""
    x0 = np.asarray(x0_sim)
    if x0.ndim != 3:
        raise ValueError("x0_sim must be (T, M, 7)")
    T, M = batch.T, x0.shape[1]
    sensing = _sensing(T, M, sensor, sigma_gyro, sigma_att, sigma_mag, latency)
    fo, Xh, ff = _model_mag_sun_filtering(T, M, batch.N, filter, want_estimates)
    out = _pd_call(solver, batch, x0_sim, kd, kp, noise_seed, X, U, plant, Rtab, gm, sat, limit_mode, x0_nom, noise_id0,
                   want_trajectories, sigma_scale, u_scale, min_steps, w_tol, angle_tol, sensing=sensing, filtering=(fo, Xh, ff),
                   sun=_sun(batch, Stab, sigma_sun))
    return dict(out, X_hat=Xh, filt_final=ff)
