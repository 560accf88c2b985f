"""Receding-horizon re-solve on the GPU (BASELINE.json configs[4]).

Not in the reference — it follows its optimised plan with TVLQR (src/attitude_controller.jl:1-48). Defined here as the
obvious closed loop around the same solve: at every control step re-solve the horizon from the
current state, warm-started with the previous plan shifted by one knot, apply the first control to the noise-free plant,
move on. The whole loop runs on the resident batch through ``tsat_mpc_run``; only the closed-loop history comes back.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _abi
from .trajopt import BatchProblem


def receding_horizon(prob, solver, n_steps, plant_integrator=4, max_outer=1, max_inner=3):
    """``prob``: BatchProblem (or SlewBatch via BatchProblem.from_arrays) — its N is the re-solve horizon, its field
    tables must cover ``n_steps`` further rows. Returns dict(X_hist (T, n_steps+1, 7), U_hist (T, n_steps, 3), stats
    (last solve), ms (device time of the loop)); the last plan stays resident (``solver.download()``)."""
    lib = _abi.load()
    b = prob.arrays
    opts = solver.opts
    o = opts.to_abi(b.N, b.n_tab, prob.integrator, prob.terminal_mask, error_state=prob.error_state)
    o.max_outer, o.max_inner = int(max_outer), int(max_inner)
    solver.upload(b, o.max_linesearch)
    T = b.T
    Xh = np.empty((T, n_steps + 1, 7)); Uh = np.empty((T, n_steps, 3))
    st = np.zeros(T, dtype=_abi.STATS_DTYPE)
    ms = C.c_float(0.0)
    rc = lib.tsat_mpc_run(solver._h, C.byref(o), int(n_steps), int(plant_integrator), _abi.as_dp(Xh), _abi.as_dp(Uh),
                          st.ctypes.data_as(C.c_void_p), C.byref(ms))
    solver._check(rc, "tsat_mpc_run")
    return dict(X_hist=Xh, U_hist=Uh, stats=st, ms=float(ms.value))


def _noise_options(lib, noise_opts):
    """``tsat_tvlqr_options`` of the dispersed loop: None = the defaults with a noise-free plant, a dict of field values
    (``noise_seed`` alone switches the generated noise on), or a ready ``_abi.TvlqrOptions``."""
    if isinstance(noise_opts, _abi.TvlqrOptions):
        return _abi.TvlqrOptions.from_buffer_copy(noise_opts)
    po = _abi.TvlqrOptions()
    lib.tsat_tvlqr_default_options(C.byref(po))
    kw = dict(noise_opts or {})
    if "noise_seed" in kw and "noise_mode" not in kw:
        kw["noise_mode"] = 1
    for k, v in kw.items():
        if k not in dict(_abi.TvlqrOptions._fields_):
            raise ValueError(f"unknown tsat_tvlqr_options field {k!r}")
        setattr(po, k, v)
    return po


def _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                gravity=None, sensed=None, filtered=None, model_filtered=None, model_mag_filtered=None):
    """``tsat_mpc_run_dispersed`` (``replan_every`` None), ``tsat_mpc_run_held``, — with ``gravity`` = (Rtab, gm) —
    ``tsat_mpc_run_held_gg`` or — with ``sensed`` = (SensorOptions, sensor (T, 9) or None) and ``gravity`` (Rtab may be None) —
    ``tsat_mpc_run_held_sensed`` or — with ``filtered`` = (FilterOptions or None, filt_init (T, 31) or None) besides —
    ``tsat_mpc_run_held_filtered`` or — with ``model_filtered`` = (ModelFilterOptions or None, filt_init (T, 58) or None) instead —
    ``tsat_mpc_run_held_model_filtered`` or — with ``model_mag_filtered`` = (ModelMagFilterOptions or None, filt_init (T, 58) or None)
    instead — ``tsat_mpc_run_held_model_mag_filtered`` on ``prob``: marshalling of all seven"""
    lib = _abi.load()
    b = prob.arrays
    o = solver.opts.to_abi(b.N, b.n_tab, prob.integrator, prob.terminal_mask, error_state=prob.error_state)
    o.max_outer, o.max_inner = int(max_outer), int(max_inner)
    po = _noise_options(lib, noise_opts)
    T = b.T
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    if plant is not None:
        plant = c(plant)
        if plant.shape != (T, 21):
            raise ValueError("plant must be (T, 21)")
    lo = hi = None
    if sat is not None:
        lo, hi = (c(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))) for v in sat)
    ids = None
    if noise_id is not None:
        ids = np.ascontiguousarray(noise_id, dtype=np.int64)
        if ids.shape != (T,):
            raise ValueError("noise_id must be (T,)")
    if upload:
        solver.upload(b, o.max_linesearch)
    Xh = np.empty((T, n_steps + 1, 7)); Uh = np.empty((T, n_steps, 3))
    st = np.zeros(T, dtype=_abi.STATS_DTYPE)
    ts = np.zeros(T, dtype=_abi.TVLQR_STATS_DTYPE)
    ncl = np.zeros(T, dtype=np.int32)
    ms = C.c_float(0.0)
    d = _abi.as_dp
    head = (solver._h, C.byref(o), C.byref(po), int(n_steps), int(step0))
    tail = (d(plant), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(Xh), d(Uh),
            st.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), _abi.as_ip(ncl), C.byref(ms))
    if sensed is not None:
        so, sensor = sensed
        Rtab = None
        if gravity[0] is not None:
            from .tracking import orbit_table
            Rtab = orbit_table(b, gravity[0])
        if sensor is not None:
            sensor = c(sensor)
            if sensor.shape != (T, 9):
                raise ValueError("sensor must be (T, 9)")
        Yh = np.empty((T, n_steps, 7))
        args = (*head, int(replan_every), int(feedback), *tail, d(Rtab), float(gravity[1]), C.byref(so), d(sensor), d(Yh))
        res = dict(X_hist=Xh, U_hist=Uh, stats=st, tracking_stats=ts, n_clipped=ncl, Y_hist=Yh)
        if model_filtered is not None or model_mag_filtered is not None:      # the two nine-state filters: one record, two entry points
            name = "tsat_mpc_run_held_model_filtered" if model_filtered is not None else "tsat_mpc_run_held_model_mag_filtered"
            fo, init = model_filtered if model_filtered is not None else model_mag_filtered
            if init is not None:
                init = c(init)
                if init.shape != (T, MODEL_FILTER_STATE_W):
                    raise ValueError("filt_init must be (T, 58)")
            fs, ff = (None, None) if fo is None else (np.empty((T, MODEL_FILTER_STATE_W)), np.empty((T, 12)))
            solver._check(getattr(lib, name)(*args, None if fo is None else C.byref(fo), d(init), d(fs), d(ff)), name)
            res.update(filt_state=fs, filt_final=ff)
        elif filtered is None:
            solver._check(lib.tsat_mpc_run_held_sensed(*args), "tsat_mpc_run_held_sensed")
        else:
            fo, init = filtered
            if init is not None:
                init = c(init)
                if init.shape != (T, FILTER_STATE_W):
                    raise ValueError("filt_init must be (T, 31)")
            fs, ff = (None, None) if fo is None else (np.empty((T, FILTER_STATE_W)), np.empty((T, 9)))
            solver._check(lib.tsat_mpc_run_held_filtered(*args, None if fo is None else C.byref(fo), d(init), d(fs), d(ff)),
                          "tsat_mpc_run_held_filtered")
            res.update(filt_state=fs, filt_final=ff)
        res["ms"] = float(ms.value)
        return res
    if gravity is not None:
        from .tracking import orbit_table
        Rtab = orbit_table(b, gravity[0])
        solver._check(lib.tsat_mpc_run_held_gg(*head, int(replan_every), int(feedback), *tail, d(Rtab), float(gravity[1])),
                      "tsat_mpc_run_held_gg")
    elif replan_every is None:
        solver._check(lib.tsat_mpc_run_dispersed(*head, *tail), "tsat_mpc_run_dispersed")
    else:
        solver._check(lib.tsat_mpc_run_held(*head, int(replan_every), int(feedback), *tail), "tsat_mpc_run_held")
    return dict(X_hist=Xh, U_hist=Uh, stats=st, tracking_stats=ts, n_clipped=ncl, ms=float(ms.value))


def receding_horizon_dispersed(prob, solver, n_steps, plant=None, sat=None, noise_opts=None, noise_id=None, step0=0,
                               max_outer=1, max_inner=3, upload=True):
    """``receding_horizon`` on a noisy, dispersed plant with limits (``tsat_mpc_run_dispersed``): trajectory t flies inertia Jp,
    actuator matrix G and residual dipole m_res of ``plant[t]`` ((T, 21), one realisation of ``tracking.disperse_plant``; None =
    the model's plant) under ``clip(U[0], lo, hi)`` — ``sat`` = (lo, hi), each (T, 3) or (3,), units of u_scale, or None —, with
    the plant noise the ensemble roll-out injects when ``noise_opts`` switches it on (``dict(noise_seed=...)``, any further
    ``tsat_tvlqr_options`` fields, e.g. min_steps / w_tol / angle_tol of the statistic), generator id ``noise_id[t]`` (default t),
    knots ``step0 + s``. The plant integrator is RK4. ``upload=False`` continues the resident simulation (give ``step0``).
    Returns dict(X_hist (T, n_steps+1, 7), U_hist (T, n_steps, 3) the limited commands, stats (last solve), tracking_stats (T,)
    slew-time statistic of the closed-loop history, n_clipped (T,), ms)."""
    return _plant_loop(prob, solver, n_steps, None, 0, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload)


def receding_horizon_held(prob, solver, n_steps, replan_every, feedback=True, plant=None, sat=None, noise_opts=None, noise_id=None,
                          step0=0, max_outer=1, max_inner=3, upload=True):
    """``receding_horizon_dispersed`` that re-solves every ``replan_every`` control steps only (``tsat_mpc_run_held``): in between,
    step j > 0 of a block flies the plan's control U[j] plus the solver's own gains on the state difference to the plan
    (``feedback=True``; the policy of the solver's forward sweep) or U[j] alone (``feedback=False``, the open-loop hold). Same plant,
    limits, noise draws and statistic; ``replan_every=1`` is ``receding_horizon_dispersed`` bit for bit. ``replan_every`` is at most
    the shortest horizon - 1. A continuation (``upload=False``, ``step0``) begins with a solve: it equals one longer run only when
    the first call's ``n_steps`` is a multiple of ``replan_every``. Returns the dict of ``receding_horizon_dispersed`` plus
    ``n_solves`` = ceil(n_steps / replan_every)."""
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload)
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


def receding_horizon_held_gg(prob, solver, n_steps, replan_every, Rtab, gm=3.986004418e5, feedback=True, plant=None, sat=None,
                             noise_opts=None, noise_id=None, step0=0, max_outer=1, max_inner=3, upload=True):
    """``receding_horizon_held`` under gravity-gradient torque (``tsat_mpc_run_held_gg``): every plant step also feels
    3 gm / |r|^3 (r_b x Jp r_b) with the trajectory's own inertia; the solve does not see it. ``Rtab`` (n_btab, n_tab, 3) km holds
    the orbit position of every field row of the batch (``magnetic.orbit_rows``) and follows its ``btab_idx`` — so it is shared by
    the realisations of ``tile_realisations`` as the field tables are; ``gm`` in km^3 / s^2, 0 switches the term off.
    ``replan_every=1`` is the every-step loop under gravity gradient."""
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                    gravity=(Rtab, gm))
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


def _sensor_options(sensor_opts, latency):
    """``tsat_sensor_options`` of the loops fed measurements: None = the ideal sensor, a dict of the three sigmas, or a ready
    ``_abi.SensorOptions``, whose latency then counts"""
    if isinstance(sensor_opts, _abi.SensorOptions):
        return _abi.SensorOptions.from_buffer_copy(sensor_opts)
    kw = dict(sensor_opts or {})
    unknown = set(kw) - {"sigma_gyro", "sigma_att", "sigma_mag"}
    if unknown:
        raise ValueError(f"unknown tsat_sensor_options field(s) {sorted(unknown)}")
    return _abi.SensorOptions(sigma_gyro=kw.get("sigma_gyro", 0.0), sigma_att=kw.get("sigma_att", 0.0), sigma_mag=kw.get("sigma_mag", 0.0),
                              latency=int(latency), reserved=0)


def receding_horizon_held_sensed(prob, solver, n_steps, replan_every, sensor_opts=None, sensor=None, latency=0, Rtab=None, gm=0.0,
                                 feedback=True, plant=None, sat=None, noise_opts=None, noise_id=None, step0=0, max_outer=1, max_inner=3,
                                 upload=True):
    """``receding_horizon_held`` (``Rtab`` None, ``gm`` 0) or ``receding_horizon_held_gg`` FED MEASUREMENTS
    (``tsat_mpc_run_held_sensed``): every block's solve starts from, and the held steps' gains act on, a measurement of the true
    state — gyro and attitude noise of ``sensor_opts`` (None = the ideal sensor, a dict of ``sigma_gyro`` / ``sigma_att`` /
    ``sigma_mag``, or a ready ``_abi.SensorOptions``, whose latency then counts), biases ``sensor`` ((T, 9): one realisation of
    ``tracking.disperse_sensor`` per trajectory; None = zeros), ``latency`` 0 or 1 control steps. The plant flies and the statistic
    judges the true state. The sensor draws are made when ``noise_opts`` switches the generated noise on, under its seed. The
    magnetometer figures are accepted and unused: the loop has no law that reads the field. A continuation equals one longer run
    only with ``latency=0`` (and whole blocks): latency 1 restarts its memory with every call. Returns the dict of
    ``receding_horizon_held`` plus ``Y_hist`` (T, n_steps, 7), the measurement each step's command or solve used."""
    so = _sensor_options(sensor_opts, latency)
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                    gravity=(Rtab, gm), sensed=(so, sensor))
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


FILTER_STATE_W = 31     # TSAT_FILTER_STATE_W: q^ 4, b^ 3, w^ 3, A 6, B 9, D 6


def receding_horizon_held_filtered(prob, solver, n_steps, replan_every, filter=None, filt_init=None, sensor_opts=None, sensor=None,
                                   latency=0, Rtab=None, gm=0.0, feedback=True, plant=None, sat=None, noise_opts=None, noise_id=None,
                                   step0=0, max_outer=1, max_inner=3, upload=True):
    """``receding_horizon_held_sensed`` BEHIND THE FILTER of ``tracking.attitude_ensemble_filtered`` (``tsat_mpc_run_held_filtered``):
    the multiplicative EKF runs over the raw measurements, one per control step, and the block solves' x0, the state the held steps'
    gains act on and ``Y_hist`` are its estimate (at latency 1 predicted across the delay). ``filter``: a ``tracking.filter_options``
    result, or a dict of that function's arguments; None passes f = NULL, which is ``receding_horizon_held_sensed`` itself
    (``filt_state`` and ``filt_final`` are then None, and ``filt_init`` must be None). ``filt_init`` (T, 31): the filter records a
    previous call returned as ``filt_state`` — sample 0 then makes a filter step instead of starting the filter; None starts it on
    the call's first measurement. At latency 0 a continuation (``upload=False``, ``step0`` = the steps made, ``filt_init`` = the
    previous ``filt_state``, whole blocks) equals one longer run; latency 1 still restarts the sensor's memory with every call.
    Returns the dict of ``receding_horizon_held_sensed`` plus ``filt_state`` (T, 31: q^ 4, b^ 3, w^ 3, A 6, B 9, D 6) and
    ``filt_final`` (T, 9: b^, sqrt diag A, sqrt diag D) after the last sample processed."""
    if isinstance(filter, dict):
        from .tracking import filter_options
        filter = filter_options(**filter)
    if filter is not None and not isinstance(filter, _abi.FilterOptions):
        raise ValueError("filter must be None, a tracking.filter_options() result or a dict of its arguments")
    so = _sensor_options(sensor_opts, latency)
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                    gravity=(Rtab, gm), sensed=(so, sensor), filtered=(filter, filt_init))
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


MODEL_FILTER_STATE_W = 58     # TSAT_MODEL_FILTER_STATE_W: q^ 4, w^ 3, b^ 3, u 3, A 6, W 6, D 6, X 9, B 9, Y 9


def receding_horizon_held_model_filtered(prob, solver, n_steps, replan_every, filter=None, filt_init=None, sensor_opts=None, sensor=None,
                                         latency=0, Rtab=None, gm=0.0, feedback=True, plant=None, sat=None, noise_opts=None,
                                         noise_id=None, step0=0, max_outer=1, max_inner=3, upload=True):
    """``receding_horizon_held_sensed`` BEHIND THE NINE-STATE FILTER of ``tracking.attitude_ensemble_model_filtered``
    (``tsat_mpc_run_held_model_filtered``): the model-based multiplicative EKF — body rate a state, propagated on the batch's own
    model (``Jmat``, u_scale) under the limited command and the field rows each plant step read, the gyro a measurement — runs over
    the raw measurements, one per control step, and the block solves' x0, the state the held steps' gains act on and ``Y_hist`` are
    its estimate (at latency 1 the model prediction across the delay, rate included). ``filter``: a ``tracking.model_filter_options``
    result, or a dict of that function's arguments; None passes f = NULL, which is ``receding_horizon_held_sensed`` itself
    (``filt_state`` and ``filt_final`` are then None, and ``filt_init`` must be None). ``filt_init`` (T, 58): the filter records a
    previous call returned as ``filt_state`` — sample 0 then makes an update on the record instead of starting the filter; None
    starts it on the call's first measurement. The record a call leaves is the prior for the state it leaves (one closing predict
    after the last control step). At latency 0 a continuation (``upload=False``, ``step0`` = the steps made, ``filt_init`` = the
    previous ``filt_state``, whole blocks) equals one longer run bit for bit; latency 1 still restarts the sensor's memory with every
    call. Returns the dict of ``receding_horizon_held_sensed`` plus ``filt_state`` (T, 58: q^ 4, w^ 3, b^ 3, u 3, A 6, W 6, D 6,
    X 9, B 9, Y 9) and ``filt_final`` (T, 12: b^, sqrt diag P_tt, sqrt diag P_ww, sqrt diag P_bb) of that record."""
    if isinstance(filter, dict):
        from .tracking import model_filter_options
        filter = model_filter_options(**filter)
    if filter is not None and not isinstance(filter, _abi.ModelFilterOptions):
        raise ValueError("filter must be None, a tracking.model_filter_options() result or a dict of its arguments")
    so = _sensor_options(sensor_opts, latency)
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                    gravity=(Rtab, gm), sensed=(so, sensor), model_filtered=(filter, filt_init))
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


def receding_horizon_held_model_mag_filtered(prob, solver, n_steps, replan_every, filter=None, filt_init=None, sensor_opts=None,
                                             sensor=None, latency=0, Rtab=None, gm=0.0, feedback=True, plant=None, sat=None,
                                             noise_opts=None, noise_id=None, step0=0, max_outer=1, max_inner=3, upload=True):
    """``receding_horizon_held_model_filtered`` WITH THE ATTITUDE UPDATE REPLACED BY THE MAGNETOMETER'S
    (``tsat_mpc_run_held_model_mag_filtered``): the filter of ``tracking.attitude_ensemble_model_mag_filtered`` in the held loop. The
    attitude sensor is read once — sample 0 of a call without ``filt_init`` —; after that the nine-state filter is corrected by one
    magnetometer reading per control step (the true body field of the row the plant's step reads, bias ``sensor[:, 6:9]``, noise
    ``sigma_mag`` of ``sensor_opts``) against the slew's own field table, and by the gyro. Model, predict, the closing predict, the
    record and every other argument are the parent's. ``filter``: a ``tracking.model_mag_filter_options`` result, or a dict of that
    function's arguments; None passes f = NULL, which is ``receding_horizon_held_sensed`` itself (``filt_state`` and ``filt_final``
    are then None, and ``filt_init`` must be None). ``filt_init`` (T, 58): sample 0 then makes an update — magnetometer and gyro — on
    the record instead of starting the filter. At latency 0 a continuation equals one longer run bit for bit under the parent's
    conditions; latency 1 restarts the sensor's memory, the field's included, with every call. Returns the parent's dict."""
    if isinstance(filter, dict):
        from .tracking import model_mag_filter_options
        filter = model_mag_filter_options(**filter)
    if filter is not None and not isinstance(filter, _abi.ModelMagFilterOptions):
        raise ValueError("filter must be None, a tracking.model_mag_filter_options() result or a dict of its arguments")
    so = _sensor_options(sensor_opts, latency)
    r = _plant_loop(prob, solver, n_steps, replan_every, feedback, plant, sat, noise_opts, noise_id, step0, max_outer, max_inner, upload,
                    gravity=(Rtab, gm), sensed=(so, sensor), model_mag_filtered=(filter, filt_init))
    r["n_solves"] = -(-int(n_steps) // int(replan_every))
    return r


_PER_SLEW = ("x0", "xf", "btab_idx", "tau0", "dtau", "dt", "Jmat", "Qd", "Qfd", "Rd", "ulo", "uhi", "U0")


def tile_realisations(batch, M, plant=None, noise_id0=None, sat=None, sensor=None):
    """M realisations per slew laid out as one batch of T M trajectories, slew-major (t M + m): the per-slew arrays repeated, the
    field tables shared through ``btab_idx``. ``plant`` (T, M, 21) straight from ``tracking.disperse_plant``; generator ids
    ``noise_id0[t] + m`` (default t M + m). Realisation (t, m) of ``receding_horizon_dispersed(BatchProblem.from_arrays(tiled),
    solver, n, **kw)`` then flies the plant and draws the noise of realisation (t, m) of ``tracking.attitude_ensemble_dispersed``.
    ``sensor`` (T, M, 9) straight from ``tracking.disperse_sensor``: the biases of ``receding_horizon_held_sensed``, realisation
    (t, m) those of realisation (t, m) of ``tracking.attitude_ensemble_sensed``.
    Returns (tiled batch, kw) with kw = dict(plant (T M, 21) or None, noise_id (T M,), sat) and, when given, sensor (T M, 9)."""
    T, M = batch.T, int(M)
    if batch.Btab is None:
        raise ValueError("the tiled batch shares host field tables through btab_idx: batch.Btab must be an array")
    idx = np.repeat(np.arange(T), M)
    rep = {k: np.ascontiguousarray(getattr(batch, k)[idx]) for k in _PER_SLEW}
    if batch.n_knots is not None:
        rep["n_knots"] = np.ascontiguousarray(np.asarray(batch.n_knots)[idx])
    tiled = dataclasses.replace(batch, **rep)
    if plant is not None:
        plant = np.asarray(plant, dtype=np.float64)
        if plant.shape != (T, M, 21):
            raise ValueError("plant must be (T, M, 21)")
        plant = np.ascontiguousarray(plant.reshape(T * M, 21))
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    if id0.shape != (T,):
        raise ValueError("noise_id0 must be (T,)")
    ids = np.ascontiguousarray((id0[:, None] + np.arange(M, dtype=np.int64)[None, :]).reshape(T * M))
    if sat is not None:
        sat = tuple(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (T, 3))[idx]) for v in sat)
    kw = dict(plant=plant, noise_id=ids, sat=sat)
    if sensor is not None:
        sensor = np.asarray(sensor, dtype=np.float64)
        if sensor.shape != (T, M, 9):
            raise ValueError("sensor must be (T, M, 9)")
        kw["sensor"] = np.ascontiguousarray(sensor.reshape(T * M, 9))
    return tiled, kw
