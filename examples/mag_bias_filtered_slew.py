#!/usr/bin/env python3
"""The slew of examples/mag_filtered_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same gyro
figure, a magnetometer at 5e-7 T noise — with the magnetometer carrying a 1.5e-6 T bias (tracking.disperse_sensor), the normal case
next to magnetorquers. How many loops arrive when the filter ESTIMATES that bias, and how far off is the attitude the law sees?

    python examples/mag_bias_filtered_slew.py [--out profiles/ensemble/mag_bias_filtered_failures.txt]   (needs an MI355X; well under a minute)

Four configurations, each under the TVLQR law and under the PD law with the plan's feed-forward, at latency 0 and 1, all on the
biased magnetometer:
  raw measurements                                   tracking.attitude_ensemble_sensed / attitude_ensemble_pd_sensed
  behind the six-state filter                        tracking.attitude_ensemble_filtered / attitude_ensemble_pd_filtered
  behind the magnetometer-updated filter             tracking.attitude_ensemble_mag_filtered / attitude_ensemble_pd_mag_filtered
  ... with the magnetometer bias as a state          tracking.attitude_ensemble_mag_bias_filtered / attitude_ensemble_pd_mag_bias_filtered
The first two read a 1 deg attitude sensor at every knot and the magnetometer only in the PD law's projection; the last two use the
attitude measurement of knot 0 only (p0_att = 1 deg), assume the gyro's own noise (sigma_v = 0.38 pi / 180 rad/s) and the
magnetometer's own (sigma_m = 5e-7 T), and carry no gyro-bias state (the gyros of this example carry no bias). The last one starts
its bias state at p0_mag = 1.5e-6 T with no random walk (the bias is constant). Printed per run: failures of 256 and, behind a
filter, the rms over the realisations and the last half of the horizon of the angle between what the law saw (X_hat) and the true
attitude; for the last one also the median of |c^ - c| / |c| at the end."""
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
from mag_filtered_slew import MAG_BIAS, SIGMA_MAG, rms_attitude_error_deg  # noqa: E402
from replanned_slew import spread  # noqa: E402
from sensed_slew import WN, ZETA  # noqa: E402


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
    mag = tracking.mag_filter_options(tracking.SENSOR_SIGMA_GYRO, SIGMA_MAG, p0_att=tracking.SENSOR_SIGMA_ATT)
    magb = tracking.mag_bias_filter_options(tracking.SENSOR_SIGMA_GYRO, SIGMA_MAG, p0_att=tracking.SENSOR_SIGMA_ATT, p0_mag=MAG_BIAS)
    biased = tracking.disperse_sensor(1, M, np.random.default_rng(11), mag_bias=MAG_BIAS)
    tv = dict(raw=tracking.attitude_ensemble_sensed, six=tracking.attitude_ensemble_filtered, mag=tracking.attitude_ensemble_mag_filtered,
              magb=tracking.attitude_ensemble_mag_bias_filtered)
    pd = dict(raw=tracking.attitude_ensemble_pd_sensed, six=tracking.attitude_ensemble_pd_filtered, mag=tracking.attitude_ensemble_pd_mag_filtered,
              magb=tracking.attitude_ensemble_pd_mag_bias_filtered)
    configs = (("raw measurements", "raw", None), ("behind the six-state filter", "six", six),
               ("behind the magnetometer-updated filter", "mag", mag),
               ("behind the magnetometer-updated filter that estimates the magnetometer bias", "magb", magb))
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    say(f"{M} dispersed plants, {N} samples of {b.dt[0]} s each; 0.38 deg/s gyro noise; 1 deg attitude noise (the magnetometer-updated "
        f"filters read the attitude sensor at knot 0 only); magnetometer noise {SIGMA_MAG:g} T, magnetometer bias {MAG_BIAS:g} T per axis; "
        f"PD gains wn = {WN} rad/s, zeta = {ZETA}; failures of {M}:")
    out_d = dict(N=N)
    for law in ("TVLQR tracking of the plan", "PD tracking + feed-forward"):
        for latency in (0, 1):
            for label, kind, f in configs:
                kw = dict(plant=plant, sat=sat, latency=latency, sigma_mag=SIGMA_MAG, sensor=biased, want_trajectories=f is not None, **SENSOR)
                if f is not None:
                    kw.update(filter=f, want_estimates=True)
                if law.startswith("TVLQR"):
                    r = tv[kind](solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, **kw)
                else:
                    r = pd[kind](solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], **kw)
                st = r["stats"][0]
                tail = ""
                if f is not None:
                    tail = f"; rms attitude error of X_hat over the last half {rms_attitude_error_deg(r['X_hat'], r['X_sim'], N):.2f} deg"
                if kind == "magb":
                    c = biased[0, :, 6:9]
                    rel = np.linalg.norm(r["filt_final"][0, :, 9:12] - c, axis=1) / np.linalg.norm(c, axis=1)
                    tail += f"; median |c^ - c| / |c| at the end {np.median(rel):.2f}"
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
