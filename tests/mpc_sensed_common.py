"""Shared pieces of tests/test_mpc_sensed.py (CPU tier) and tests/test_gpu_mpc_sensed.py (GPU tier): the held re-planning loop FED
MEASUREMENTS (tsat_mpc_run_held_sensed).

THE REFERENCE is ``mpc_held_common.reference_loop`` with three things inserted, built from the oracle's primitives only:
``sensed_common.measure`` (its w_m and q_m; the field measurement it also returns is dropped: the loop has no law that reads it),
the latency rule (y_s = m_s, or m_max(s-1, 0) with s counted FROM THE CALL), and the separation of the true state — which the
plant advances, the statistic judges and X_hist records — from the state the solver is given: each block's solve starts from
y_{s_b} and the held steps' gain product is evaluated on y_s. With an orbit table every stage also gets ``gg_common.gg_increment``,
as ``gg_common.held_loop`` adds it. With the ideal sensor it has to equal its parents with max |d| = 0
(test_mpc_sensed.py::test_reference_with_the_ideal_sensor_is_the_held_reference).

Workloads, plants, limits, ids and bars are the held tests' own (mpc_held_common). The sensor levels start from
``sensed_common.SIGMAS`` / ``BIAS``. The sigmas were kept. The biases were DOUBLED, on the reference alone: under the limits +-0.6
every command of the workload clips, so the flown commands are bang-bang and a small change of the measurement moves the final
state either by a flipped component or by exactly nothing — at the ensembles' bias levels the attitude or the gyro bias left three of
the six GPU cases unmoved (0.0); at twice the level every case meets every condition (``conditions`` below; the measured figures
are in the docstrings of the two test modules).

Also: the ctypes binding of the emulated loop (tests/emu/tsat_emu_mpc_sensed.cpp, built on demand by its own make fragment)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import gg_common as gc
import mpc_held_common as hc
import reference_rollout as rr
import sensed_common as sc
from conftest import ROOT

SIGMAS, IDEAL = sc.SIGMAS, sc.IDEAL
BIAS = {k: 2.0 * v for k, v in sc.BIAS.items()}      # gyro 3e-3 rad/s, attitude 1.5 deg (magnetometer 3e-6: nothing reads it)


def biases(pkg, T, M=None):
    """(T, 9), or (T, M, 9) with M: ``tracking.disperse_sensor`` at BIAS"""
    b = pkg.tracking.disperse_sensor(T, M or 1, np.random.default_rng(11), **BIAS)
    return b if M else np.ascontiguousarray(b[:, 0])


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, sens=None, bias=None, latency=0, plant=None, sat=None,
                   noise_id=None, step0=0, Rtab=None, gm=0.0, nthreads=4, est=None):
    """arguments and result as ``mpc_held_common.reference_loop`` plus: ``sens`` the three sigmas (None = IDEAL), ``bias`` (T, 9) or
    None, ``latency``, the orbit table and gm of ``gg_common.held_loop`` (None: no term), ``est(t)`` the estimator between sample and
    solver / gains (None: none); and ``Y_hist`` (T, n_steps, 7)"""
    return rr.held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, IDEAL if sens is None else sens, bias, latency, plant, sat,
                        noise_id, step0, Rtab, gm, nthreads, est)


def measured(ol, batch, po, X_hist, sens, bias, latency, noise_id, step0=0):
    """``measure`` applied to the true states X_hist (T, n + 1, 7) with the latency shift: what Y_hist (T, n, 7) has to be"""
    T, n = X_hist.shape[0], X_hist.shape[1] - 1
    noisy = int(po.noise_mode) == 1
    clock = types.SimpleNamespace(dtau=batch.dtau, tau0=batch.tau0, Btab=batch.Btab, btab_idx=batch.btab_idx, n_tab=batch.n_tab)
    M = np.zeros((T, n, 7))
    for t in range(T):
        for s in range(n):
            w_m, q_m, _ = sc.measure(ol, clock, t, int(step0) + s, X_hist[t, s], po, noise_id[t], sens, None if bias is None else bias[t], noisy)
            M[t, s] = np.r_[w_m, q_m]
    return np.concatenate([M[:, :1], M[:, :-1]], axis=1) if latency else M


def moved(a, b, label):
    """a sensor effect has to show on the references before a kernel is looked at: final states differ by >= gg_common.MOVED"""
    d = float(np.max(np.abs(a["X_hist"][:, -1] - b["X_hist"][:, -1])))
    print(f"{label}: moves the reference's final state by {d:.2e}")
    assert d >= gc.MOVED, f"{label} does not show on this case"
    return d


def conditions(ref_of, bias, label, batch, po):
    """the conditions of a case on references alone. ``ref_of(**over)`` is the reference of the test's call with the named arguments
    (sens, bias, latency) replaced. The call itself meets ``mpc_held_common.condition``; sensor noise, gyro bias, attitude bias and
    latency 1 against 0 each move the final state by at least ``gg_common.MOVED``. Returns the reference of the call itself."""
    ref = ref_of()
    hc.condition(ref, batch, po, label)
    moved(ref, ref_of(sens=IDEAL), f"{label}: sensor noise on against off")
    for name, sl in (("gyro", slice(0, 3)), ("attitude", slice(3, 6))):
        z = bias.copy()
        z[..., sl] = 0.0
        moved(ref, ref_of(bias=z), f"{label}: {name} bias on against zero")
    moved(ref_of(latency=1), ref_of(latency=0), f"{label}: latency 1 against 0")
    return ref


def sensed_call(abi, batch, opts, po, n_steps, replan_every, feedback, sens, bias, latency, plant, sat, noise_id, step0, Rtab, gm):
    """``mpc_held_common.held_call`` followed by what the sensed drivers share after it: Rtab, gm, the sensor options, the biases and
    Y_hist. A driver's ``run`` appends its own arguments and then x0_after, which is in ``out`` already."""
    T = batch.T
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    args, out = hc.held_call(abi, batch, opts, po, n_steps, replan_every, feedback, plant, sat, noise_id, step0)
    out.update(Y_hist=np.full((T, n_steps, 7), np.nan), x0_after=np.zeros((T, 7)))
    so = sc.sensor_options(abi, IDEAL if sens is None else sens, latency)
    return args + [abi.as_dp(c(Rtab)), C.c_double(gm), C.byref(so), abi.as_dp(c(bias)), abi.as_dp(out["Y_hist"])], out


class EmuMpcSensed:
    """ctypes binding of tests/emu/libtsat_emu_mpc_sensed.so, built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_sensed.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_sensed.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, sens=None, bias=None, latency=0, plant=None, sat=None, noise_id=None,
            step0=0, Rtab=None, gm=0.0):
        """emu_mpc_held_sensed_batch; the result of ``mpc_held_common.EmuMpcHeld.run`` plus Y_hist and x0_after (T, 7), x0 of the
        parameter records as the call leaves them"""
        args, out = sensed_call(self.abi, batch, opts, po, n_steps, replan_every, feedback, sens, bias, latency, plant, sat, noise_id, step0,
                                Rtab, gm)
        rc = self.lib.emu_mpc_held_sensed_batch(*args, self.abi.as_dp(out["x0_after"]))
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_sensed_batch rc={rc}")
        return out

    def check(self, so, sensor, T, Rtab=None, gm=0.0):
        """check_mpc_sensed on the arguments tsat_mpc_run_held_sensed adds"""
        text = C.create_string_buffer(256)
        sensor = None if sensor is None else np.ascontiguousarray(sensor, dtype=np.float64)
        R = None if Rtab is None else np.ascontiguousarray(Rtab, dtype=np.float64)
        rc = self.lib.emu_mpc_sensed_check(None if so is None else C.byref(so), self.abi.as_dp(sensor), C.c_int64(T), self.abi.as_dp(R),
                                           C.c_double(gm), text, C.c_int32(256))
        return rc, text.value.decode()
