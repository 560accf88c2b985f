"""Shared by the line-search keep-rule tests (CPU tier: test_line_search_policy.py, GPU tier: test_gpu_line_search.py): the
input, its oracle solve with the per-iteration trace (computed once per session), and the keep rule of solve_trajectory
(tsat_device.hpp) replayed on that trace — how many forward sweeps a one-trajectory build executes under a policy."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, Emu, oracle_options

T, N, SEED = 64, 200, 20190530      # N - 1 = 199: no multiple of the 32-knot forward chunk or of 64
MAX_LS = 20                          # tsat_default_options: candidates alpha = 2^-j, j < 20
FEW, HOLD_DEFAULT = 4, 8             # N_FEW, LS_HOLD of tsat_device.hpp (documented at tsat_set_store_policy)
KEEP_ALL = (MAX_LS, 0)               # few >= max_linesearch: every roll-out is kept, always
NEVER_DEEP = 1 << 30

_case = None


class EmuLineSearch(Emu):
    """ctypes binding of tests/emu/libtsat_emu_line_search[_dense].so, built here by its own make fragment: the emulated solve
    launched as the library launches it (slabs as tsat_batch_reserve sizes them, the rule of emu_set_store_policy)"""

    def __init__(self, abi, dense=False):
        d = os.path.join(ROOT, "tests", "emu")
        name = "libtsat_emu_line_search_dense.so" if dense else "libtsat_emu_line_search.so"
        subprocess.check_call(["make", "-C", d, name], stdout=subprocess.DEVNULL)
        self.lib = C.CDLL(os.path.join(d, name))
        self.lib.emu_solve_batch = self.lib.emu_ls_solve_batch      # Emu.solve: same arguments, this driver's launch
        self.abi = abi


_emus = {}


def emulator(pkg, dense):
    if dense not in _emus:
        _emus[dense] = EmuLineSearch(pkg._abi, dense)
    return _emus[dense]


def case(pkg, ol):
    """(batch, oracle options, oracle result with trace): 64 slews x 200 knots on their own dipole tables, budget 5 x 10"""
    global _case
    if _case is None:
        b = pkg.slew_setup.workload_monte_carlo(T=T, N=N, seed=SEED)
        o = oracle_options(ol, max_outer=5, max_inner=10, dj_counter_limit=1, error_state=1)
        assert o.max_linesearch == MAX_LS
        ref = ol.solve_batch(b, o, nthreads=min(16, ol.num_procs()), trace_rows=64)
        for a in (ref["X"], ref["U"], ref["K"], ref["stats"], ref["trace"]):
            a.setflags(write=False)
        _case = (b, o, ref)
    return _case


def accepted_indices(ref, t):
    """accepted line-search index of every inner iteration of trajectory t, in order (-1: no candidate was accepted)"""
    n = int(ref["stats"]["inner_iters"][t])
    return ref["trace"][t, :n, 4].astype(int)


def deep_trajectories(ref):
    """trajectories with a search that went to index >= 12 (past what a sweep used to keep) or found nothing"""
    return [t for t in range(ref["X"].shape[0]) if np.any((accepted_indices(ref, t) >= 12) | (accepted_indices(ref, t) < 0))]


def expected_sweeps(jws, few, hold, slots, max_ls=MAX_LS):
    """forward sweeps of a solve whose line searches accept the indices `jws`: the open-loop roll-out, one sweep per search,
    and one more whenever the sweep before had not kept the candidate that is accepted (or none is)"""
    n, since = 1, NEVER_DEEP
    n_slots = min(max_ls, slots)
    for jw in jws:
        keep_all = since < NEVER_DEEP if hold < 0 else since <= hold
        n_store = n_slots if (keep_all or n_slots < few) else few
        shift = 0
        while shift < max_ls:
            n += 1
            if 0 <= jw < shift + min(max_ls - shift, n_store):
                break
            shift, n_store = shift + n_store, n_slots
        if jw < 0 or jw >= few - 1:
            since = 0
        elif since < NEVER_DEEP:
            since += 1
    return n


def expected_n_forward(ref, few, hold, slots, which=None):
    ts = range(ref["X"].shape[0]) if which is None else which
    return np.array([expected_sweeps(accepted_indices(ref, t), few, hold, slots) for t in ts], dtype=np.int32)


def pick(pkg, b, idx):
    """the trajectories `idx` of the batch as a batch of their own (tables kept whole)"""
    c = lambda a: np.ascontiguousarray(a[idx])
    return pkg.slew_setup.SlewBatch(b.N, b.n_tab, c(b.x0), c(b.xf), b.Btab, c(b.btab_idx), c(b.tau0), c(b.dtau), c(b.dt), c(b.Jmat),
                                    c(b.Qd), c(b.Qfd), c(b.Rd), c(b.ulo), c(b.uhi), c(b.U0), dict(b.meta), None)


def assert_same_bits(a, b, what):
    """X, U, K and every statistic except n_forward, bit for bit"""
    for k in ("X", "U", "K"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for f in a["stats"].dtype.names:
        assert f == "n_forward" or np.array_equal(a["stats"][f], b["stats"][f]), (what, f)
