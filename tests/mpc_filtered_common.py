"""Shared pieces of tests/test_mpc_filtered.py (CPU tier) and tests/test_gpu_mpc_filtered.py (GPU tier): the held re-planning loop
BEHIND THE FILTER (tsat_mpc_run_held_filtered).

THE REFERENCE (``reference_loop``) is ``reference_rollout.held_loop`` with ``filtered_common.Ekf`` — the recursion of
include/tortoise_hip.h, line for line — between ``measure`` and solver / gains: numpy and the oracle's primitives only. Per control
step s, counted FROM THE CALL (``reference_rollout.SixState``): the raw sample the sensor hands over (m_s, or m_max(s-1, 0) at latency
1) makes ``first`` at s = 0 (a ``step`` when a record ``filt_init`` is given), no step at s = 1 of latency 1 (m_0 handed over a second
time), a ``step`` otherwise; the solver's x0, the gains' state and Y_hist read (w^, q^), with q^ predicted across the delay for s >= 1
at latency 1. With
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

import numpy as np

import filtered_common as fc
import mpc_held_common as hc
import mpc_sensed_common as mc
import reference_rollout as rr
from conftest import ROOT

FILT = fc.FILT
STATE_W = 31
EST_BAR = 1e-9               # Y_hist, filt_state, filt_final: the state bar of the sensed and filtered tests


def estimator(ol, batch, filt, filt_init=None, predict=True):
    """t -> the estimator of trajectory t: ``filtered_common.Ekf`` behind ``reference_rollout.SixState``, resumed from the record
    filt_init[t] where one is given. ``filt`` None: no filter"""
    if filt is None:
        return None
    return lambda t: rr.SixState(fc.Ekf(ol, batch.dt[t], filt), predict, None if filt_init is None else filt_init[t])


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, filt=None, filt_init=None, predict=True):
    """arguments and result as ``mpc_sensed_common.reference_loop`` plus ``filt`` (the five levels, None: no filter — the sensed
    reference itself), ``filt_init`` (T, 31) or None, ``predict`` (False leaves the prediction across the delay out: a condition of
    the tests, not a mode of the product); and ``filt_state`` (T, 31), ``filt_final`` (T, 9)"""
    return mc.reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens, bias, latency, plant, sat, noise_id, step0, Rtab,
                             gm, nthreads, estimator(ol, batch, filt, filt_init, predict))


def estimates(ol, batch, filt, handed, latency, filt_init=None):
    """the ``Ekf`` run over the samples ``handed`` (T, n, 7) as the sensor hands them over (``mpc_sensed_common.measured``: with the
    latency shift): (Y (T, n, 7), filt_state (T, 31), filt_final (T, 9)). No solve, no plant."""
    T, n = handed.shape[:2]
    Y, S, F = np.zeros((T, n, 7)), np.zeros((T, STATE_W)), np.zeros((T, 9))
    for t in range(T):
        e = estimator(ol, batch, filt, filt_init)(t)
        for s in range(n):
            Y[t, s] = np.r_[e.sample(s, latency, handed[t, s, :3], handed[t, s, 3:7], None, None, None, None, None)]
        S[t], F[t] = e.record(), e.final()
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


def filtered_run(fn, abi, fo, widths, filt_init, batch, *a):
    """the emulated driver ``fn`` of a held loop behind a filter: ``mpc_sensed_common.sensed_call(abi, batch, *a)`` followed by the
    filter options ``fo`` (None: f = NULL), filt_init, filt_state (T, widths[0]), filt_final (T, widths[1]) and x0_after"""
    args, out = mc.sensed_call(abi, batch, *a)
    fs, ff = (None, None) if fo is None else (np.full((batch.T, widths[0]), np.nan), np.full((batch.T, widths[1]), np.nan))
    fi = None if filt_init is None else np.ascontiguousarray(filt_init, dtype=np.float64)
    rc = fn(*args, None if fo is None else C.byref(fo), abi.as_dp(fi), abi.as_dp(fs), abi.as_dp(ff), abi.as_dp(out["x0_after"]))
    if rc != 0:
        raise RuntimeError(f"{fn.__name__} rc={rc}")
    return dict(out, filt_state=fs, filt_final=ff)


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
        fo = None if filt is None else fc.filter_options(self.abi, filt)
        return filtered_run(self.lib.emu_mpc_held_filtered_batch, self.abi, fo, (STATE_W, 9), filt_init, batch, opts, po, n_steps, replan_every,
                            feedback, sens, bias, latency, plant, sat, noise_id, step0, Rtab, gm)

    def check(self, fo, filt_init, T, filt_state=None, filt_final=None):
        """check_mpc_filtered on the arguments tsat_mpc_run_held_filtered adds"""
        text = C.create_string_buffer(256)
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rc = self.lib.emu_mpc_filtered_check(None if fo is None else C.byref(fo), self.abi.as_dp(c(filt_init)), self.abi.as_dp(c(filt_state)),
                                             self.abi.as_dp(c(filt_final)), C.c_int64(T), text, C.c_int32(256))
        return rc, text.value.decode()
