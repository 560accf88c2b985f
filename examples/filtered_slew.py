#!/usr/bin/env python3
"""The slew of examples/sensed_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same sensor
levels — with a multiplicative EKF between the measurement and the law: of the loops that fail on raw 1 deg / 0.38 deg/s
measurements, how many still fail behind the filter every spacecraft carries?

    python examples/filtered_slew.py [--out profiles/ensemble/filtered_failures.txt]       (needs an MI355X; a few seconds)

The filter is the standard six-state one — attitude error and gyro bias, propagated by the gyro, updated by the attitude
measurement (include/tortoise_hip.h; tracking.attitude_ensemble_filtered -> tsat_tvlqr_ensemble_filtered,
tracking.attitude_ensemble_pd_filtered -> tsat_pd_ensemble_filtered) — at the sensor's own figures: sigma_v = 0.38 pi / 180 rad/s,
sigma_a = p0_att = pi / 180 rad, no bias state (the sensors of this example carry no bias). It removes attitude-sensor noise; it
does NOT smooth white gyro noise: the rate the law sees is still one gyro sample. Printed: failures of 256 for the TVLQR law and
for the PD law with the plan's feed-forward, each raw and filtered, at latency 0 and 1."""
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
from sensed_slew import WN, ZETA  # noqa: E402

SENSOR = dict(sigma_gyro=tracking.SENSOR_SIGMA_GYRO, sigma_att=tracking.SENSOR_SIGMA_ATT)


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
    filt = tracking.filter_options(tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; 0.38 deg/s gyro and 1 deg attitude noise; PD gains wn = {WN} rad/s, "
        f"zeta = {ZETA}; failures of {M}:")
    out_d = dict(N=N)
    for law in ("TVLQR tracking of the plan", "PD tracking + feed-forward"):
        for latency in (0, 1):
            for label, f in (("raw measurements", None), ("behind the filter", filt)):
                kw = dict(plant=plant, sat=sat, latency=latency, **SENSOR)
                if law.startswith("TVLQR"):
                    fn = tracking.attitude_ensemble_sensed if f is None else tracking.attitude_ensemble_filtered
                    r = fn(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, **kw, **({} if f is None else dict(filter=f)))
                else:
                    fn = tracking.attitude_ensemble_pd_sensed if f is None else tracking.attitude_ensemble_pd_filtered
                    r = fn(solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], **kw, **({} if f is None else dict(filter=f)))
                st = r["stats"][0]
                tail = "" if f is None else f"; median sqrt(diag A) at the end {np.degrees(np.median(r['filt_final'][0, :, 3:6])):.3f} deg"
                say(f"  {law}, latency {latency}, {label}: {fails(st)} of {M} fail; {spread(st)}; median final error angle "
                    f"{np.median(st['final_angle']):.4f} rad{tail}")
                out_d[(law, latency, label)] = st
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
