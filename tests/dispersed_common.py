"""Shared pieces of tests/test_dispersed.py (CPU tier) and tests/test_gpu_dispersed.py (GPU tier).

THE REFERENCE of the dispersed ensemble (tsat_tvlqr_ensemble_dispersed) is a closed loop built knot by knot
(``reference_rollout.ensemble_loop``) from the unchanged oracle's primitives only: ``ol.tvlqr_batch`` for the gains K (model
inertia), then per knot ``ol.qmult`` on the conjugate reference attitude for dX, the three rules of the entry point (u_cmd =
U - K dX; u_sat = clip(u_cmd); the plant of all four RK4 stages sees G u_sat + m_res / u_scale and has inertia Jp),
``ol.plant_noise`` for the draws, the noise injection of src/simulator.jl:5-23 (``_noisy`` here), ``ol.dyn7`` on Jp per stage,
table rows floor((k + c) dtau + tau0) clamped (``_row`` here). With the model's plant and no limits it has to reproduce
``ol.tvlqr_batch`` (test_dispersed.py::test_reference_is_pinned_to_the_oracle).

Also: the bracket on the clipped-knot counter, the sampled (t, m) pairs with their replacement cap and the cases of
tests/ensemble_common.py, which also holds the ctypes binding of the emulated kernel (``EmuEnsemble.run(..., plant=...)``)."""
import math

import numpy as np

import ensemble_common as ec

MARGIN = 1e-7            # as the ensemble tests: index equality only where the reference is not on a threshold
CLIP_BAND = 1e-7         # relative width of the band around a limit inside which the clip decision is a matter of the last bit
N_DRAWN, N_KEPT = 34, 32  # sampled realisations: at most 2 of 34 may be replaced (the cap of test_gpu_ensemble_at_size)
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)

_fma = getattr(math, "fma", None)


def _row(batch, t, k, c):
    v = _fma(k + c, float(batch.dtau[t]), float(batch.tau0[t])) if _fma else (k + c) * float(batch.dtau[t]) + float(batch.tau0[t])
    r = math.floor(v)
    i = 0 if not r >= 0 else min(int(r), batch.n_tab - 1)
    return batch.Btab[batch.btab_idx[t], i]


def _noisy(ol, x, b, nz):
    """the state and the field row a stage evaluates the dynamics at (src/simulator.jl:5-23)"""
    if nz is None:
        return x, b
    q = x[3:7] / math.sqrt(float(x[3:7] @ x[3:7]))
    th = math.sqrt(float(nz[3:6] @ nz[3:6]))
    dq = np.r_[math.cos(th / 2), nz[3:6] * (0.5 if th == 0.0 else math.sin(th / 2) / th)]
    return np.r_[x[:3] + nz[:3], ol.qmult(q, dq)], b + nz[6:9]


def reference_loop(ol, batch, t, Xr, Ur, K, x0, opts, gid, plant=None, lo=None, hi=None, noisy=True):
    """one closed loop of slew t: ``reference_rollout.ensemble_loop`` under the TVLQR law on the true state, no gravity-gradient
    term. Xr (N,7), Ur (N-1,3) the plan, K (N-1,6,3) the oracle's gains of it, plant (21,) or None for the model's, lo / hi (3,) or
    None, gid the generator id. Returns X_sim (N,7) zero-filled beyond the slew's horizon, (n_sure, n_maybe)."""
    import reference_rollout as rr          # here: that module is built on this one
    return rr.ensemble_loop(ol, "tv", batch, t, Xr, Ur, K, x0, opts, gid, None, 0.0, plant, lo, hi, noisy=noisy)[:2]


def stats_of(abi, X_sim, xf, n_knots, dt, min_steps=10, w_tol=0.05, angle_tol=0.08727):
    """the slew-time statistic (src/monte_carlo.jl:242-262) of trajectories X_sim (n, N, 7)"""
    n = X_sim.shape[0]
    st = np.zeros(n, dtype=abi.TVLQR_STATS_DTYPE)
    for i in range(n):
        N = int(n_knots[i])
        X = X_sim[i, :N]
        w = np.linalg.norm(X[:, :3], axis=1)
        e0 = X[:, 3:7] @ xf[i, 3:7]
        ang = 2.0 * np.arccos(np.minimum(e0, 1.0))
        j = np.arange(1, N + 1)
        hit = np.flatnonzero((j > min_steps) & (w < w_tol) & (ang < angle_tol))
        first = int(j[hit[0]]) if hit.size else 0
        st[i] = (first, 0 if first else 1, dt[i] * (first if first else N), w[-1], ang[-1])
    return st


def reference_pairs(ol, abi, batch, X, U, K, x0_sim, opts, pairs, plant=None, sat=None, noise_id0=None):
    """the reference on the (t, m) pairs (n, 2); m = -1 is the noise-free MODEL plant from X[t, 0] (stats_nominal).
    Returns the dict of ``reference_rollout.pairs_of``."""
    import reference_rollout as rr
    return rr.pairs_of(ol, abi, "tv", batch, x0_sim, K, opts, pairs, X=X, U=U, plant=plant, sat=sat, noise_id0=noise_id0)


def all_pairs(T, M):
    return np.stack(np.meshgrid(np.arange(T), np.arange(M), indexing="ij"), axis=-1).reshape(-1, 2)


def sampled_pairs(T, M, seed=32):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, T, N_DRAWN), rng.integers(0, M, N_DRAWN)], axis=1)


def kept(ref):
    """indices of the first N_KEPT sampled realisations whose reference run meets the margin; asserts the replacement cap"""
    ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1]) > MARGIN for i in range(len(ref["stats"]))])
    keep = np.flatnonzero(ok)[:N_KEPT]
    print(f"sampled pairs that fail the margin: {int(np.count_nonzero(~ok))} of {len(ok)}; arrivals among the kept: "
          f"{int(np.count_nonzero(ref['stats']['failed'][keep] == 0))}")
    assert keep.size == N_KEPT, "more than 2 of 34 sampled realisations sit on a threshold"
    return keep


def compare(ref, got, pairs, idx=None, clipped=True):
    """the bars: |dX_sim| < 1e-9, same_stats, n_sure <= n_clipped <= n_maybe — on the realisations `idx` of `pairs`"""
    idx = np.arange(len(pairs)) if idx is None else idx
    t, m = pairs[idx, 0], pairs[idx, 1]
    if got.get("X_sim") is not None:
        dX = float(np.max(np.abs(ref["X_sim"][idx] - got["X_sim"][t, m])))
        print(f"max|dX_sim| against the reference {dX:.2e}")
        assert dX < 1e-9
    ec.same_stats(ref["stats"][idx], got["stats"][t, m])
    assert np.array_equal(ref["stats"]["slew_time"][idx], got["stats"]["slew_time"][t, m])
    if clipped:
        n = got["n_clipped"][t, m]
        print(f"clipped knots: sure {ref['n_sure'][idx].min()} .. {ref['n_sure'][idx].max()}, got {n.min()} .. {n.max()}, "
              f"undecided knots up to {int((ref['n_maybe'][idx] - ref['n_sure'][idx]).max())}")
        assert np.all(ref["n_sure"][idx] <= n) and np.all(n <= ref["n_maybe"][idx])


def all_five_plants(pkg, batch, M):
    """the plants of the parity tests: all five dispersions at LEVELS, default_rng(7)"""
    return pkg.tracking.disperse_plant(batch.Jmat, M, np.random.default_rng(7), **LEVELS)

