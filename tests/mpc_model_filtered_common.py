"""Shared pieces of tests/test_mpc_model_filtered.py (CPU tier) and tests/test_gpu_mpc_model_filtered.py (GPU tier): the held
re-planning loop BEHIND THE NINE-STATE FILTER (tsat_mpc_run_held_model_filtered).

THE REFERENCE (``reference_loop``) is ``reference_rollout.held_loop`` with ``model_filtered_common.ModelEkf`` — the recursion of
include/tortoise_hip.h, line for line — between ``measure`` and solver / gains: numpy and the oracle's primitives only. Per control
step s, counted FROM THE CALL, the raw sample the sensor hands over (m_s, or m_max(s-1, 0) at latency 1) meets
(``reference_rollout.ModelState``)

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

import gg_common as gc
import model_filtered_common as mm
import mpc_filtered_common as mf6
import mpc_held_common as hc
import mpc_sensed_common as mc
import reference_rollout as rr
from conftest import ROOT

FILT = mm.FILT
STATE_W, FINAL_W = 58, 12
EST_BAR = mf6.EST_BAR        # Y_hist, filt_state, filt_final: the state bar of the sensed and filtered tests (1e-9)
VARIANT = dict(command=True, predict=True, rows="flown", inertia="model")


ROW_DT = 10.0                # seconds of orbit per field row in the tests' tables (``coarse_rows``)


def coarse_rows(pkg, batch, dt_row=ROW_DT):
    """the batch (in place) on a dipole table of the same orbit and row count whose rows are ``dt_row`` seconds apart. On the held
    tests' own table (0.2 s a row, one row a step) the rows of two neighbouring steps differ so little that the off-by-one of the
    clock moves the CPU case's final state by 1.4e-8 only, below ``gg_common.MOVED``; the condition stays, the table's step is the
    level that was changed."""
    B = pkg.slew_setup.dipole_btable(batch.n_tab, dt_row, 6771.0, 96.6)
    batch.Btab = np.ascontiguousarray(B[None])
    return batch


def estimator(ol, batch, us, filt, plant=None, filt_init=None, variant=VARIANT):
    """t -> the estimator of trajectory t: ``model_filtered_common.ModelEkf`` behind ``reference_rollout.ModelState``, resumed from
    the record filt_init[t] where one is given. ``filt`` None: no filter. Of ``variant`` the filter takes ``command`` and its
    inertia, the adapter ``predict`` and ``rows``"""
    if filt is None:
        return None

    def make(t):
        J = plant[t, 0:9].reshape(3, 3).T if variant["inertia"] == "plant" else np.asarray(batch.Jmat[t]).reshape(3, 3).T
        ekf = mm.ModelEkf(ol, batch.dt[t], J, us, filt, dict(mm.VARIANT, command=variant["command"]))
        return rr.ModelState(ekf, variant["predict"], variant["rows"], None if filt_init is None else filt_init[t], FINAL_W)

    return make


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, filt=None, filt_init=None, variant=VARIANT):
    """arguments and result as ``mpc_sensed_common.reference_loop`` plus ``filt`` (the seven levels, None: no filter — the sensed
    reference itself), ``filt_init`` (T, 58) or None, ``variant``; and ``filt_state`` (T, 58), ``filt_final`` (T, 12)"""
    return mc.reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens, bias, latency, plant, sat, noise_id, step0, Rtab,
                             gm, nthreads, estimator(ol, batch, float(opts.u_scale), filt, plant, filt_init, variant))


def estimates(ol, batch, us, filt, handed, U_hist, latency, filt_init=None):
    """the ``ModelEkf`` run over the samples ``handed`` (T, n, 7) as the sensor hands them over (``mpc_sensed_common.measured`` of a
    returned X_hist: with the latency shift), with the returned U_hist (T, n, 3) and the rows of the batch's clock advanced by one
    rounded addition per step, the closing predict included: (Y (T, n, 7), filt_state (T, 58), filt_final (T, 12)). No solve, no
    plant."""
    T, n = handed.shape[:2]
    Y, S, F = np.zeros((T, n, 7)), np.zeros((T, STATE_W)), np.zeros((T, FINAL_W))
    make = estimator(ol, batch, float(us), filt, None, filt_init)
    ests = [make(t) for t in range(T)]
    tau = batch.tau0.copy()
    rows_prev = [None] * T
    for s in range(n):
        clock = types.SimpleNamespace(dtau=batch.dtau, tau0=tau, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
        for t in range(T):
            rows = rr.rows_of(clock, t, 0)
            Y[t, s] = np.r_[ests[t].sample(s, latency, handed[t, s, :3], handed[t, s, 3:7], None, None, rows, rows_prev[t],
                                           U_hist[t, s - 1] if s else None)]
            rows_prev[t] = rows
        tau = tau + batch.dtau
    for t in range(T):
        ests[t].flown(U_hist[t, n - 1], rows_prev[t])
        S[t], F[t] = ests[t].record(), ests[t].final()
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
        fo = None if filt is None else mm.filter_options(self.abi, filt)
        return mf6.filtered_run(self.lib.emu_mpc_held_model_filtered_batch, self.abi, fo, (STATE_W, FINAL_W), filt_init, batch, opts, po,
                                n_steps, replan_every, feedback, sens, bias, latency, plant, sat, noise_id, step0, Rtab, gm)

    def check(self, fo, filt_init, T, filt_state=None, filt_final=None):
        """check_mpc_model_filtered on the arguments tsat_mpc_run_held_model_filtered adds"""
        text = C.create_string_buffer(256)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rc = self.lib.emu_mpc_model_filtered_check(None if fo is None else C.byref(fo), self.abi.as_dp(c(filt_init)),
                                                   self.abi.as_dp(c(filt_state)), self.abi.as_dp(c(filt_final)), C.c_int64(T), text,
                                                   C.c_int32(256))
        return rc, text.value.decode()
