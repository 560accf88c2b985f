#!/usr/bin/env python3
"""The slew of examples/dispersed_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits — with the
feedback reading MEASUREMENTS instead of the true state: how many slews still arrive, and does the plan-tracking law lose more than
the PD law that needs no plan?

    python examples/sensed_slew.py [--out profiles/ensemble/sensed_failures.txt]       (needs an MI355X; a few seconds)

Every other closed loop of the library commands from a perfect attitude solution and a perfect gyro. The reference's noise figures
are sensor figures — a 0.38 deg gyro figure and a 1 deg attitude figure (src/simulator.jl:5,10), which it squares and injects into
the dynamics. Here they are read UN-SQUARED and put where a sensor sits: sigma_gyro = 0.38 pi / 180 rad/s on the measured rate,
sigma_att = pi / 180 rad on the measured attitude (tracking.attitude_ensemble_sensed -> tsat_tvlqr_ensemble_sensed,
tracking.attitude_ensemble_pd_sensed -> tsat_pd_ensemble_sensed; no biases, no magnetometer error). Printed: failures of 256 for
the TVLQR law and for the PD law with the plan's feed-forward, each with ideal sensors, with those levels, and with those levels
one sample late (latency = 1)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from replanned_slew import spread  # noqa: E402

WN, ZETA = 0.01, 1.0               # PD gains, as examples/baseline_slew.py: rad/s, -
SETTINGS = (("ideal sensors", dict()),
            ("0.38 deg/s gyro, 1 deg attitude noise", dict(sigma_gyro=tracking.SENSOR_SIGMA_GYRO, sigma_att=tracking.SENSOR_SIGMA_ATT)),
            ("the same, one sample late", dict(sigma_gyro=tracking.SENSOR_SIGMA_GYRO, sigma_att=tracking.SENSOR_SIGMA_ATT, latency=1)))


def main(M=256, verbose=True, out=None):
    lines = []

    def say(line):
        if verbose:
            print(line, flush=True)
        lines.append(line)

    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    Ql, Qfl, Rl = tracking.tvlqr_weights(1)
    x0_lqr = tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tracking.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    sat = (b.ulo, b.uhi)
    kd, kp = tracking.pd_gains(b.Jmat, WN, ZETA)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; PD gains wn = {WN} rad/s, zeta = {ZETA}; failures of {M}:")
    out_d = dict(N=N)
    for law in ("TVLQR tracking of the plan", "PD tracking + feed-forward"):
        for label, kw in SETTINGS:
            if law.startswith("TVLQR"):
                r = tracking.attitude_ensemble_sensed(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant=plant, sat=sat, **kw)
            else:
                r = tracking.attitude_ensemble_pd_sensed(solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], plant=plant, sat=sat, **kw)
            st = r["stats"][0]
            say(f"  {law}, {label}: {fails(st)} of {M} fail; {spread(st)}; median final error angle {np.median(st['final_angle']):.4f} rad")
            out_d[(law, label)] = st
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
