#!/usr/bin/env python3
"""The slew of examples/gravity_gradient_slew.py — same 256 dispersed plants, same generator ids, same limits, same gravity field —
flown by the feedback law every magnetorquer CubeSat already carries: does the plan and its gains buy anything over a PD law?

    python examples/baseline_slew.py [--out profiles/ensemble/pd_failures.txt]       (needs an MI355X; a few seconds)

The baseline is the projection PD law of the reference's comparison scripts (src/comparison/psiaki_dynamics.jl:1-26), as
include/tortoise_hip.h defines it: T_req = -(kd dw + kp s e), m = (b x T_req) / |b|^2 (tracking.attitude_ensemble_pd ->
tsat_pd_ensemble). It needs no plan, no gains and no Riccati pass, so one entry point serves three uses, all shown here:
  1. failures of 256 under TVLQR tracking of the plan (tracking.attitude_ensemble_gg), next to PD tracking of the same plan with and
     without its feed-forward;
  2. PD regulation to the goal over one orbit (X = None: 27 000 knots of 0.2 s, nothing of that size goes to the device);
  3. a 16 x 16 grid of (wn, zeta) as 256 "slews" x 64 plants in ONE call of the same regulation, the best pair printed."""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import magnetic, slew_setup as ss, tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from gravity_gradient_slew import tables  # noqa: E402
from replanned_slew import spread  # noqa: E402

WN, ZETA = 0.01, 1.0               # the pair of parts 1 and 2: rad/s, -
N_ORBIT = 27000                    # one orbit at 0.2 s
GRID_WN, GRID_ZETA = np.geomspace(1e-3, 3e-2, 16), np.linspace(0.3, 3.0, 16)
GM = tracking.GM_EARTH


def orbit_batch(solver, b, T, n=N_ORBIT):
    """the slew of `b` T times over n knots (default one orbit, N_ORBIT) on the orbit's own table (2 n rows, two per knot, the last one
    zero — the law commands no dipole there), field and position; no plan"""
    kep = np.array([[0.0, 400.0 + 6371.0, 51.6, 0.0, 0.0, 90.0]])
    B, pos = magnetic.magnetic_simulation(solver, kep, 0.0, n * float(b.dt[0]), n)
    rows = B.shape[1]
    rep = lambda a: np.ascontiguousarray(np.repeat(a[:1], T, axis=0))
    ob = dataclasses.replace(b, N=n, n_tab=rows, Btab=np.ascontiguousarray(B), btab_idx=np.zeros(T, dtype=np.int32),
                             tau0=np.zeros(T), dtau=np.full(T, rows / float(n)), U0=np.zeros((T, 1, 3)), n_knots=None,
                             **{k: rep(getattr(b, k)) for k in ("x0", "xf", "dt", "Jmat", "Qd", "Qfd", "Rd", "ulo", "uhi")})
    return ob, magnetic.orbit_rows(pos, rows)


def main(M=256, verbose=True, out=None):
    lines = []

    def say(line):
        if verbose:
            print(line, flush=True)
        lines.append(line)

    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say, J=ss.INERTIA["3U"])
    b = batch.arrays
    pos, _, _ = tables(solver, N)
    R1 = magnetic.orbit_rows(pos, b.n_tab)
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    sat = (b.ulo, b.uhi)
    kd, kp = tracking.pd_gains(b.Jmat, WN, ZETA)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants around the 3U inertia under gravity gradient, {N} samples of {b.dt[0]} s each; PD gains wn = {WN} rad/s, zeta = {ZETA}:")
    tv = tracking.attitude_ensemble_gg(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant, R1, GM, sat=sat)
    pf = tracking.attitude_ensemble_pd(solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], plant=plant, Rtab=R1, gm=GM, sat=sat)
    pn = tracking.attitude_ensemble_pd(solver, b, x0_lqr, kd, kp, 1, X=res["X"], plant=plant, Rtab=R1, gm=GM, sat=sat)
    for label, r in (("TVLQR tracking of the plan:    ", tv), ("PD tracking + feed-forward:    ", pf), ("PD tracking, no feed-forward:  ", pn)):
        st = r["stats"][0]
        say(f"  {label} {fails(st)} of {M} fail; {spread(st)}; median final error angle {np.median(st['final_angle']):.4f} rad")
    out_d = dict(N=N, tvlqr=tv["stats"][0], pd_ff=pf["stats"][0], pd=pn["stats"][0])
    # regulation over one orbit: no plan at all
    ob, Rorb = orbit_batch(solver, b, 1)
    rg = tracking.attitude_ensemble_pd(solver, ob, x0_lqr, kd, kp, 1, plant=plant, Rtab=Rorb, gm=GM, sat=sat, limit_mode=1)
    st = rg["stats"][0]
    say(f"  PD regulation over one orbit ({N_ORBIT} samples, direction-preserving limit): {fails(st)} of {M} fail; {spread(st)}; "
        f"median final error angle {np.median(st['final_angle']):.4f} rad")
    out_d["regulation"] = st
    # the gain grid: one "slew" per (wn, zeta), the first 64 plants, starts and generator ids for every pair
    Mg, T = min(64, M), GRID_WN.size * GRID_ZETA.size
    gb, Rg = orbit_batch(solver, b, T)
    wn, zeta = (g.ravel() for g in np.meshgrid(GRID_WN, GRID_ZETA, indexing="ij"))
    gkd, gkp = tracking.pd_gains(gb.Jmat, wn, zeta)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a[:1, :Mg], (T,) + a[:1, :Mg].shape[1:]))
    gr = tracking.attitude_ensemble_pd(solver, gb, tile(x0_lqr), gkd, gkp, 1, plant=tile(plant), Rtab=Rg, gm=GM, sat=sat, limit_mode=1,
                                       noise_id0=np.zeros(T, dtype=np.int64))
    nf, mean_all = gr["summary"][:, 1], gr["summary"][:, 5]
    best = int(np.lexsort((mean_all, nf))[0])
    say(f"  {GRID_WN.size} x {GRID_ZETA.size} gain grid, {Mg} plants per pair, one call of {T * Mg} closed loops: best pair wn = {wn[best]:.4g} rad/s, "
        f"zeta = {zeta[best]:.3g} with {int(nf[best])} of {Mg} failing (mean slew time {mean_all[best]:.0f} s); "
        f"pairs without a failure: {int(np.count_nonzero(nf == 0))} of {T}")
    out_d["grid"] = dict(wn=wn, zeta=zeta, failures=nf, best=best)
    solver.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out_d


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(out=ap.parse_args().out)
