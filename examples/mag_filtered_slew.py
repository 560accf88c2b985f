#!/usr/bin/env python3
"""The slew of examples/filtered_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same gyro figure
— flown with the sensors the reference's satellite has: a gyro and a magnetometer, and ONE coarse attitude fix at acquisition. Of the
loops that arrive behind the six-state filter with a 1 deg attitude sensor, how many still arrive when the attitude sensor is gone
after knot 0 and the magnetometer takes its place?

    python examples/mag_filtered_slew.py [--out profiles/ensemble/mag_filtered_failures.txt]       (needs an MI355X; well under a minute)

Five configurations, each under the TVLQR law and under the PD law with the plan's feed-forward, at latency 0 and 1:
  raw measurements                                       tracking.attitude_ensemble_sensed / attitude_ensemble_pd_sensed
  behind the six-state filter                            tracking.attitude_ensemble_filtered / attitude_ensemble_pd_filtered
  behind the magnetometer-updated filter, sigma_mag 5e-7 tracking.attitude_ensemble_mag_filtered / attitude_ensemble_pd_mag_filtered
  ... at sigma_mag 1e-7 T
  ... at sigma_mag 5e-7 T with a 1.5e-6 T magnetometer bias (tracking.disperse_sensor), which the filter does not estimate
The magnetometer-updated filter (include/tortoise_hip.h) uses the attitude measurement of knot 0 only (p0_att = 1 deg, the sensor's
figure), assumes the gyro's own noise (sigma_v = 0.38 pi / 180 rad/s) and the magnetometer's own (sigma_m = sigma_mag), and carries no
bias state (the gyros of this example carry no bias). The first two configurations read the magnetometer at 5e-7 T too — the PD law
projects on it. Printed per run: failures of 256 and, behind a filter, the rms over the realisations and the last half of the
horizon of the angle between what the law saw (X_hat) and the true attitude."""
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
from filtered_slew import SENSOR  # noqa: E402
from replanned_slew import spread  # noqa: E402
from sensed_slew import WN, ZETA  # noqa: E402

SIGMA_MAG, SIGMA_MAG_FINE, MAG_BIAS = 5e-7, 1e-7, 1.5e-6      # T, on a field of about 2.5e-5 T


def rms_attitude_error_deg(X_hat, X_sim, N):
    """rms over realisations and knots N // 2 .. N - 2 of the angle between the estimate and the truth"""
    a, c = X_hat[0, :, N // 2:N - 1, 3:7], X_sim[0, :, N // 2:N - 1, 3:7]
    dot = np.abs(np.sum(a * c, axis=-1)) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(c, axis=-1))
    return float(np.degrees(np.sqrt(np.mean((2.0 * np.arccos(np.minimum(dot, 1.0))) ** 2))))


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
    six = tracking.filter_options(tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
    mag = lambda sm: tracking.mag_filter_options(tracking.SENSOR_SIGMA_GYRO, sm, p0_att=tracking.SENSOR_SIGMA_ATT)
    biased = tracking.disperse_sensor(1, M, np.random.default_rng(11), mag_bias=MAG_BIAS)
    tv = dict(raw=tracking.attitude_ensemble_sensed, six=tracking.attitude_ensemble_filtered, mag=tracking.attitude_ensemble_mag_filtered)
    pd = dict(raw=tracking.attitude_ensemble_pd_sensed, six=tracking.attitude_ensemble_pd_filtered, mag=tracking.attitude_ensemble_pd_mag_filtered)
    configs = (("raw measurements", "raw", None, SIGMA_MAG, None),
               ("behind the six-state filter", "six", six, SIGMA_MAG, None),
               (f"behind the magnetometer-updated filter, sigma_mag {SIGMA_MAG:g} T", "mag", mag(SIGMA_MAG), SIGMA_MAG, None),
               (f"behind the magnetometer-updated filter, sigma_mag {SIGMA_MAG_FINE:g} T", "mag", mag(SIGMA_MAG_FINE), SIGMA_MAG_FINE, None),
               (f"behind the magnetometer-updated filter, sigma_mag {SIGMA_MAG:g} T, magnetometer bias {MAG_BIAS:g} T", "mag", mag(SIGMA_MAG),
                SIGMA_MAG, biased))
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; 0.38 deg/s gyro noise; 1 deg attitude noise (the magnetometer-updated "
        f"filter reads the attitude sensor at knot 0 only); PD gains wn = {WN} rad/s, zeta = {ZETA}; failures of {M}:")
    out_d = dict(N=N)
    for law in ("TVLQR tracking of the plan", "PD tracking + feed-forward"):
        for latency in (0, 1):
            for label, kind, f, smag, sensor in configs:
                kw = dict(plant=plant, sat=sat, latency=latency, sigma_mag=smag, sensor=sensor, want_trajectories=f is not None, **SENSOR)
                if f is not None:
                    kw.update(filter=f, want_estimates=True)
                if law.startswith("TVLQR"):
                    r = tv[kind](solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, **kw)
                else:
                    r = pd[kind](solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], **kw)
                st = r["stats"][0]
                tail = ""
                if f is not None:
                    tail = (f"; rms attitude error of X_hat over the last half {rms_attitude_error_deg(r['X_hat'], r['X_sim'], N):.2f} deg; "
                            f"median sqrt(diag A) at the end {np.degrees(np.median(r['filt_final'][0, :, 3:6])):.3f} deg")
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
