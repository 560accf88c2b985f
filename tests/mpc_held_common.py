"""Shared pieces of tests/test_mpc_held.py (CPU tier) and tests/test_gpu_mpc_held.py (GPU tier).

THE REFERENCE of the loop that re-plans every R control steps (tsat_mpc_run_held) is a Python loop over blocks
(``reference_rollout.held_loop``) built from the unchanged oracle's primitives only. To ``mpc_dispersed_common.reference_loop`` it adds: ``ol.solve_batch(..., want_K=True)`` once
per block; the command rule of include/tortoise_hip.h (U_0 at j = 0; U_j + K_j dx at j > 0 with ``feedback``, the sum started from
U_j with the columns ascending, dx = x - X_j or ``ol.quaternion_error(x, X_j)``; U_j without); ``tau += dtau`` once per step, the
rows of a step looked up at knot 0 of that clock; the plan shifted by the block's r knots inside the trajectory's own horizon. At
R = 1 it has to reproduce ``mpc_dispersed_common.reference_loop`` (test_mpc_held.py::test_reference_at_r1_is_the_every_step_reference).

The bars (``same``), the workload, the plants, the limits, the noise options and the margins are those of mpc_dispersed_common."""
import ctypes as C
import os
import subprocess

import numpy as np

import dispersed_common as dc  # noqa: F401  (the tests reach stats_of through this module)
from conftest import ROOT
from mpc_dispersed_common import CLIP_BAND, MARGIN, SAT, margins, mpc_batch, noise_options, plants, same, solve_options  # noqa: F401

# the statistic and the generator ids of the three cases of test_gpu_mpc_held.py (those of tests/test_gpu_mpc_dispersed.py)
W_TOL, ANGLE_TOL, MIN_STEPS = 1.25e-4, 3.0, 3
IDS = np.arange(8, dtype=np.int64) * 1000 + 2 ** 33
WIDE = (np.full(3, -25.0), np.full(3, 25.0))     # limits no command of the workload reaches (max |U_hist| 20.4)
RAGGED = np.array([20, 13, 6, 7, 20, 19, 6, 20], dtype=np.int32)
TSAT_MAX_OUTER = 1          # tsat_status: 0 converged, 1 outer budget exhausted; 2 REG_FAIL and 3 DIVERGED leave K undefined


def reference_loop(ol, batch, opts, n_steps, replan_every, feedback, po, plant=None, sat=None, noise_id=None, step0=0, nthreads=4):
    """the loop for the whole batch: ``reference_rollout.held_loop`` on the true state; arguments and result as
    ``mpc_dispersed_common.reference_loop`` plus ``n_solves``, ``statuses`` (n_solves, T), the status of every block solve, and
    ``tally`` (T, 4), the sums of tsat_mpc_tally over the solves"""
    import reference_rollout as rr          # here: that module is built on this one's parents
    return rr.held_loop(ol, batch, opts, n_steps, replan_every, feedback, po, plant=plant, sat=sat, noise_id=noise_id, step0=step0,
                        nthreads=nthreads)


def condition(ref, batch, po, label):
    """what a case has to show on the reference alone before a kernel result is looked at: every trajectory off the statistic's
    thresholds, arrivals and failures both present, no block solve ended in a failure status"""
    m = margins(ref, batch, po)
    failed = ref["tracking_stats"]["failed"]
    print(f"{label} reference: smallest margin {m.min():.2e}, failed {failed}, statuses up to {int(ref['statuses'].max())}")
    assert np.all(m > MARGIN), "a trajectory of the case sits on a threshold"
    assert 0 < np.count_nonzero(failed) < failed.size, "the reference must have both arrivals and failures"
    assert np.all(ref["statuses"] <= TSAT_MAX_OUTER), "a block solve ended REG_FAIL or DIVERGED: its gains are undefined"


def held_call(abi, batch, opts, po, n_steps, replan_every, feedback, plant=None, sat=None, noise_id=None, step0=0):
    """what the emu_mpc_held*_batch drivers share: (args, out) — the head of their argument list, options to n_knots in the order of
    emu_mpc_held_batch, and the result dict whose arrays it points into (the pointers keep their arrays alive). A driver's ``run``
    appends its own trailing arguments and results."""
    T, N = batch.T, batch.N
    o = opts.copy()
    o.n_knots, o.n_tab = N, batch.n_tab
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    lo, hi = (None, None) if sat is None else (c(np.broadcast_to(sat[0], (T, 3))), c(np.broadcast_to(sat[1], (T, 3))))
    ids = None if noise_id is None else np.ascontiguousarray(noise_id, dtype=np.int64)
    out = dict(X_hist=np.zeros((T, n_steps + 1, 7)), U_hist=np.zeros((T, n_steps, 3)), stats=np.zeros(T, dtype=abi.STATS_DTYPE),
               X=np.zeros((T, N, 7)), U=np.zeros((T, N - 1, 3)), tracking_stats=np.zeros(T, dtype=abi.TVLQR_STATS_DTYPE),
               n_clipped=np.full(T, -1, dtype=np.int32))
    d = abi.as_dp
    args = [C.byref(o), C.byref(po), C.c_int64(T), C.c_int64(batch.Btab.shape[0]), d(batch.x0), d(batch.xf), d(batch.Btab),
            abi.as_ip(batch.btab_idx), d(batch.tau0), d(batch.dtau), d(batch.dt), d(batch.Jmat), d(batch.Qd), d(batch.Qfd), d(batch.Rd),
            d(batch.ulo), d(batch.uhi), d(batch.U0), C.c_int32(n_steps), C.c_int64(step0), C.c_int32(replan_every), C.c_int32(feedback),
            d(c(plant)), d(lo), d(hi), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), d(out["X_hist"]), d(out["U_hist"]),
            out["stats"].ctypes.data_as(C.c_void_p), out["tracking_stats"].ctypes.data_as(C.c_void_p), abi.as_ip(out["n_clipped"]),
            d(out["X"]), d(out["U"]), None if batch.n_knots is None else abi.as_ip(np.ascontiguousarray(batch.n_knots, dtype=np.int32))]
    return args, out


class EmuMpcHeld:
    """ctypes binding of tests/emu/libtsat_emu_mpc_held.so, built here by its own make fragment"""

    def __init__(self, abi):
        d = os.path.join(ROOT, "tests", "emu")
        subprocess.check_call(["make", "-C", d, "libtsat_emu_mpc_held.so"], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, "libtsat_emu_mpc_held.so"))
        self.abi = abi

    def run(self, batch, opts, po, n_steps, replan_every, feedback, plant=None, sat=None, noise_id=None, step0=0):
        args, out = held_call(self.abi, batch, opts, po, n_steps, replan_every, feedback, plant, sat, noise_id, step0)
        rc = self.lib.emu_mpc_held_batch(*args)
        if rc != 0:
            raise RuntimeError(f"emu_mpc_held_batch rc={rc}")
        return out

    def check(self, replan_every, feedback, min_nk):
        text = C.create_string_buffer(256)
        rc = self.lib.emu_mpc_held_check(C.c_int32(replan_every), C.c_int32(feedback), C.c_int32(min_nk), text, C.c_int32(256))
        return rc, text.value.decode()
