#!/usr/bin/env python3
"""The slew of examples/baseline_slew.py — same 256 dispersed plants, same generator ids, same limits, same gravity field — flown by
the model-based regulator of the reference's comparison figure, the asymptotic periodic LQR: both laws this library could fly so far
fail on most of the dispersed plants; is that the law's fault or the plant's?

    python examples/aplqr_slew.py [--out profiles/ensemble/aplqr_failures.txt] [--orbits 2]       (needs an MI355X; a few seconds)

The law is that of src/comparison/psiaki2001_Period_LQR.jl as include/tortoise_hip.h defines it: a constant P from the 6 x 6 Riccati
equation of the orbit-averaged control-effectiveness Gramian (tracking.aplqr_gains -> tsat_aplqr_gains, on the device), then
m = -diag(1/rd) (b x Kg [theta; dw]) (tracking.attitude_ensemble_aplqr -> tsat_aplqr_ensemble). Shown here, failures of 256 each:
  1. regulation to the goal over `--orbits` orbits (X = None) by the PD law and by this law, gains averaged over the orbit's table;
  2. the plan tracked with its feed-forward by PD and by this law, gains averaged over the plan's own table."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import magnetic, slew_setup as ss, tracking, trajopt as to  # noqa: E402
import baseline_slew as base  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from gravity_gradient_slew import tables  # noqa: E402
from replanned_slew import spread  # noqa: E402

QD = np.array([1.5e-4] * 3 + [1e4] * 3)      # the reference's Q on [theta; dw] ...
RD = np.full(3, 8e6)                          # ... and R on the dipole (src/comparison/psiaki2001_Period_LQR.jl)
GM = tracking.GM_EARTH


def main(M=256, orbits=2, verbose=True, out=None):
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
    x0 = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    sat = (b.ulo, b.uhi)
    kd, kp = tracking.pd_gains(b.Jmat, base.WN, base.ZETA)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    line = lambda label, st: say(f"  {label} {fails(st)} of {M} fail; {spread(st)}; median final error angle {np.median(st['final_angle']):.4f} rad")
    say(f"{M} dispersed plants around the 3U inertia under gravity gradient; PD gains wn = {base.WN} rad/s, zeta = {base.ZETA}; APLQR weights "
        f"qd = {QD.tolist()}, rd = {RD.tolist()}, alpha = 1")
    out_d = {}
    # 1. regulation over whole orbits: the gains from the orbit's own table
    ob, Rorb = base.orbit_batch(solver, b, 1, base.N_ORBIT * int(orbits))
    Kg, info = tracking.aplqr_gains(solver, ob, QD, RD)
    say(f"gains over the orbit's table ({ob.n_tab} rows): {int(info['iterations'][0])} iterations of the sign function, residual "
        f"{float(info['residual'][0]):.2e}, smallest pivot {float(info['pivot_min'][0]):.2e}; |Kg| up to {np.abs(Kg).max():.3g}")
    say(f"regulation to the goal over {orbits} orbit(s), {ob.N} samples of {b.dt[0]} s, direction-preserving limit:")
    pr = tracking.attitude_ensemble_pd(solver, ob, x0, kd, kp, 1, plant=plant, Rtab=Rorb, gm=GM, sat=sat, limit_mode=1)
    ar = tracking.attitude_ensemble_aplqr(solver, ob, x0, Kg, RD, 1, plant=plant, Rtab=Rorb, gm=GM, sat=sat, limit_mode=1)
    line("PD regulation:                 ", pr["stats"][0])
    line("APLQR regulation:              ", ar["stats"][0])
    out_d.update(pd_regulation=pr["stats"][0], aplqr_regulation=ar["stats"][0], Kg_orbit=Kg)
    # 2. the plan tracked with its feed-forward: the gains from the plan's own table
    Kt, it = tracking.aplqr_gains(solver, b, QD, RD, allow_failed=True)
    say(f"the plan, {N} samples of {b.dt[0]} s, tracked with its feed-forward (gains over the plan's {b.n_tab}-row table: status "
        f"{int(it['status'][0])}, residual {float(it['residual'][0]):.2e}):")
    pf = tracking.attitude_ensemble_pd(solver, b, x0, kd, kp, 1, X=res["X"], U=res["U"], plant=plant, Rtab=R1, gm=GM, sat=sat)
    af = tracking.attitude_ensemble_aplqr(solver, b, x0, Kt, RD, 1, X=res["X"], U=res["U"], plant=plant, Rtab=R1, gm=GM, sat=sat)
    line("PD tracking + feed-forward:    ", pf["stats"][0])
    line("APLQR tracking + feed-forward: ", af["stats"][0])
    out_d.update(pd_ff=pf["stats"][0], aplqr_ff=af["stats"][0], Kg_plan=Kt)
    solver.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out_d


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--orbits", type=int, default=2)
    a = ap.parse_args()
    main(orbits=a.orbits, out=a.out)
