"""Field tables on the GPU — the first step of the reference's per-run setup.

``B_ECI, pos, vel = magnetic_simulation(p, t0, tf, N, mag_field)`` (src/magnetic_toolbox.jl:33-106) propagates the orbit
from Keplerian elements with a fixed-step Euler integrator, rotates to ECEF with GMST, evaluates IGRF-12 at every
sample and rotates the field back to ECI; the result has 2N rows, the last one left zero. ``magnetic_simulation`` here
does that for T orbits at once through ``tsat_btable_batch``.
"""
import ctypes as C

import numpy as np

from . import _abi


def magnetic_simulation(solver, kep, t0, tf, N, mjd=58155.0, gm=3.986004418e5, alt=400.0, R_E=6371.0, date=2019.0,
                        want_pos=True, host=True):
    """kep (T,6) = [e, a (km), i, RAAN, argp, anomaly] in degrees (src/TortoiseSat.jl:35-42); t0, tf scalars or (T,).
    Returns (B_ECI (T, 2N, 3) Tesla, pos (T, 2N+1, 3) km or None). ``host=False``: the tables are not downloaded (B_ECI is
    None) — they stay on the device, where ``horizon.condition_based_time(solver, None, ...)`` and an upload of a batch with
    ``Btab = None`` pick them up (the Monte-Carlo's tables never cross PCIe unless the caller wants to keep them)."""
    lib = _abi.load()
    kep = np.ascontiguousarray(np.atleast_2d(kep), dtype=np.float64)
    if kep.shape[1] != 6:
        raise ValueError("kep must be (T, 6)")
    T = kep.shape[0]
    t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (T,)))
    tf = np.ascontiguousarray(np.broadcast_to(np.asarray(tf, dtype=np.float64), (T,)))
    o = _abi.BtableOptions()
    lib.tsat_btable_default_options(C.byref(o))
    o.n_half, o.mjd, o.gm, o.r_igrf_km, o.date = int(N), float(mjd), float(gm), float(alt + R_E), float(date)
    B = np.empty((T, 2 * N, 3)) if host else None
    pos = np.empty((T, 2 * N + 1, 3)) if want_pos else None
    rc = lib.tsat_btable_batch(solver._h, C.byref(o), T, _abi.as_dp(kep), _abi.as_dp(t0), _abi.as_dp(tf), _abi.as_dp(B),
                               _abi.as_dp(pos))
    solver._check(rc, "tsat_btable_batch")
    return B, pos


def orbit_rows(pos, n_tab):
    """The orbit table ``Rtab`` (n_btab, n_tab, 3) of the gravity-gradient entry points (``tracking.attitude_ensemble_gg``,
    ``mpc.receding_horizon_held_gg``) from the ``pos`` (T, 2N+1, 3) km that ``magnetic_simulation`` returns: its first ``n_tab``
    rows — row i is the position at which field row i was evaluated, so the table is indexed like ``Btab[:, :n_tab]``."""
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim != 3 or pos.shape[2] != 3 or not 1 <= int(n_tab) <= pos.shape[1]:
        raise ValueError("pos must be (T, rows, 3) with rows >= n_tab >= 1")
    return np.ascontiguousarray(pos[:, :int(n_tab)])


def sun_direction(mjd, au=False):
    """The sun vector in ECI (mean equator of date) at modified Julian date ``mjd`` (a scalar or an array; the result is (3,) or
    (..., 3)) from the low-precision almanac series, with T the Julian centuries from J2000: mean longitude 280.460 + 36000.771 T,
    mean anomaly M = 357.5291092 + 35999.05034 T, ecliptic longitude = mean longitude + 1.914666471 sin M + 0.019994643 sin 2M,
    obliquity 23.439291 - 0.0130042 T (degrees); good to about 0.01 deg over 1950-2050. A unit vector; ``au=True`` scales it by the
    series' distance 1.000140612 - 0.016708617 cos M - 0.000139589 cos 2M (astronomical units)."""
    T = (np.asarray(mjd, dtype=np.float64) + 2400000.5 - 2451545.0) / 36525.0
    lm = 280.460 + 36000.771 * T
    M = np.radians(357.5291092 + 35999.05034 * T)
    lam = np.radians(lm + 1.914666471 * np.sin(M) + 0.019994643 * np.sin(2.0 * M))
    eps = np.radians(23.439291 - 0.0130042 * T)
    s = np.stack([np.cos(lam), np.cos(eps) * np.sin(lam), np.sin(eps) * np.sin(lam)], axis=-1)
    if au:
        s = s * (1.000140612 - 0.016708617 * np.cos(M) - 0.000139589 * np.cos(2.0 * M))[..., None]
    return s


def sun_rows(Rtab, mjd, R_E=6371.0):
    """The sun table ``Stab`` (n_btab, n_tab, 3) of the model-mag-sun-filtered ensembles (``tracking.attitude_ensemble_model_mag_sun_filtered``)
    from the orbit rows ``Rtab`` (n_btab, n_tab, 3) km of ``orbit_rows``: row i is ``sun_direction`` where the satellite at orbit row
    i is lit and exactly zero where it is in the cylindrical shadow of the Earth — r . s < 0 and |r - (r . s) s| < R_E. ``mjd`` is a
    scalar or (n_btab,): the direction is CONSTANT PER TABLE (the sun moves 0.04 deg per hour, far below a coarse sun sensor's noise
    over a slew). Penumbra and albedo are left out."""
    R = np.asarray(Rtab, dtype=np.float64)
    if R.ndim != 3 or R.shape[2] != 3:
        raise ValueError("Rtab must be (n_btab, n_tab, 3)")
    mjd = np.asarray(mjd, dtype=np.float64)
    if mjd.ndim > 1 or (mjd.ndim == 1 and mjd.shape != (R.shape[0],)) or not np.all(np.isfinite(mjd)):
        raise ValueError("mjd must be a finite scalar or (n_btab,)")
    if not np.all(np.isfinite(R)) or not float(R_E) > 0.0:
        raise ValueError("Rtab must be finite and R_E positive")
    s = np.broadcast_to(sun_direction(mjd), (R.shape[0], 3))[:, None, :]
    along = np.sum(R * s, axis=2, keepdims=True)
    dark = (along[..., 0] < 0.0) & (np.linalg.norm(R - along * s, axis=2) < float(R_E))
    S = np.ascontiguousarray(np.broadcast_to(s, R.shape))
    S[dark] = 0.0
    return S


def attach_igrf_tables(solver, batch, kep=None, chunk=4096):
    """Replace the field tables of a workload batch by IGRF-12 tables generated on the GPU for its orbits — what the
    reference does before every solve (``magnetic_simulation(A[i,:], t0, t_final, N, ...)``, src/monte_carlo.jl:149): one
    table per row of ``kep`` (default ``batch.meta["kep"]``), sampled over the slew horizon N dt with one row per knot step
    (2N rows, the last one zero; the solve reads rows 0 .. N, so only the first N + 8 travel on). One orbit for the whole
    batch, or one per trajectory."""
    kep = np.atleast_2d(np.asarray(batch.meta["kep"] if kep is None else kep, dtype=np.float64))
    if kep.shape[0] not in (1, batch.T):
        raise ValueError("one orbit for the batch or one per trajectory")
    N, dt = batch.N, float(batch.dt[0])
    if not np.all(batch.dt == dt):
        raise ValueError("attach_igrf_tables needs a common step")
    rows = min(2 * N, N + 8)
    parts = [np.ascontiguousarray(magnetic_simulation(solver, kep[a:a + chunk], 0.0, N * dt, N, want_pos=False)[0][:, :rows])
             for a in range(0, kep.shape[0], chunk)]
    batch.Btab = np.ascontiguousarray(np.concatenate(parts)) if len(parts) > 1 else parts[0]
    batch.n_tab = rows
    batch.btab_idx = np.zeros(batch.T, np.int32) if kep.shape[0] == 1 else np.arange(batch.T, dtype=np.int32)
    batch.tau0[:] = 0.0
    batch.dtau[:] = 1.0
    batch.meta = dict(batch.meta, field="IGRF-12 (tsat_btable_batch)")
    return batch
