#!/usr/bin/env python3
"""The slew of examples/filtered_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same gyro figure
— behind the filter a magnetorquer-only satellite could fly: the MODEL-BASED rate filter UPDATED BY THE MAGNETOMETER. It reads a gyro,
a magnetometer and ONE attitude fix at acquisition, like the mag filter, and hands the law a rate that was propagated on the model,
like the model filter. What does the law then see, and do the loops arrive?

    python examples/model_mag_filtered_slew.py [--out profiles/ensemble/model_mag_filtered_failures.txt]     (needs an MI355X; under a minute)

Six configurations, each under the TVLQR law and under the PD law with the plan's feed-forward, at latency 0 and 1:
  raw measurements                                  tracking.attitude_ensemble_sensed / attitude_ensemble_pd_sensed
  behind the six-state filter                       tracking.attitude_ensemble_filtered / attitude_ensemble_pd_filtered
  behind the model filter (attitude sensor)         tracking.attitude_ensemble_model_filtered / attitude_ensemble_pd_model_filtered
  behind the mag filter                             tracking.attitude_ensemble_mag_filtered / attitude_ensemble_pd_mag_filtered
  behind this filter at the example's sigma_w       tracking.attitude_ensemble_model_mag_filtered / attitude_ensemble_pd_model_mag_filtered
  ... at 10 x that sigma_w
All read the sensors at their own figures: 0.38 deg/s gyro noise, 1 deg attitude noise, 5e-7 T magnetometer noise on a field of
about 2.5e-5 T, no biases. The filters assume those figures (sigma_g = sigma_v = 0.38 pi / 180, sigma_a = p0_att = pi / 180, sigma_m =
5e-7) and carry no bias state. sigma_w, the un-modelled angular acceleration the two model filters assume, is measured on the
example's own dispersed plants as examples/model_filtered_slew.py measures it: one model-filtered run with the ideal sensor at
latency 1 and a filter that trusts its measurements entirely, so that (X_hat - X_sim)[k, 0:3] / h is what the model does not know; its
rms per axis over both laws is the example's sigma_w. That example found the estimate best at 10 x of it, hence the last row.

Printed per run: failures of 256 and, behind a filter, the rms over the realisations and the last half of the horizon of the rate
error (rad/s) and of the angle (deg) between what the law saw (X_hat) and the true state."""
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
from mag_filtered_slew import SIGMA_MAG  # noqa: E402
from model_filtered_slew import _errors  # noqa: E402
from sensed_slew import WN, ZETA  # noqa: E402

LAWS = ("TVLQR tracking of the plan", "PD tracking + feed-forward")


def main(M=256, verbose=True, out=None):
    lines = []

    def say(line):
        if verbose:
            print(line, flush=True)
        lines.append(line)

    tr = tracking
    solver = to.AugmentedLagrangianSolver(None, None)
    batch, res, N = plan(solver, say)
    b = batch.arrays
    Ql, Qfl, Rl = tr.tvlqr_weights(1)
    x0_lqr = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(0))
    plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
    sat = (b.ulo, b.uhi)
    kd, kp = tr.pd_gains(b.Jmat, WN, ZETA)
    h = float(b.dt[0])
    fails = lambda st: int(np.count_nonzero(st["failed"]))
    tv = dict(raw=tr.attitude_ensemble_sensed, six=tr.attitude_ensemble_filtered, model=tr.attitude_ensemble_model_filtered,
              mag=tr.attitude_ensemble_mag_filtered, this=tr.attitude_ensemble_model_mag_filtered)
    pd = dict(raw=tr.attitude_ensemble_pd_sensed, six=tr.attitude_ensemble_pd_filtered, model=tr.attitude_ensemble_pd_model_filtered,
              mag=tr.attitude_ensemble_pd_mag_filtered, this=tr.attitude_ensemble_pd_model_mag_filtered)

    def fly(law, kind, **kw):
        if law.startswith("TVLQR"):
            return tv[kind](solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant=plant, sat=sat, **kw)
        return pd[kind](solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], plant=plant, sat=sat, **kw)

    # sigma_w from the plants themselves: the model's one-step prediction from the truth against the truth
    probe = tr.model_filter_options(1.0, 1e-9, 1e-9, sigma_v=1.0, p0_att=0.0)
    acc = []
    for law in LAWS:
        r = fly(law, "model", latency=1, filter=probe, want_trajectories=True, want_estimates=True)
        d = (r["X_hat"][0][:, 1:N - 1, 0:3] - r["X_sim"][0][:, 1:N - 1, 0:3]) / h
        acc.append(float(np.sqrt(np.mean(d ** 2))))
    sigma_w = float(np.sqrt(np.mean(np.square(acc))))
    say(f"sigma_w of the example: {sigma_w:.3e} rad/s^2 (rms per axis of the un-modelled angular acceleration of the {M} plants, both laws)")
    sg, sa = tr.SENSOR_SIGMA_GYRO, tr.SENSOR_SIGMA_ATT
    configs = (("raw measurements", "raw", None),
               ("behind the six-state filter", "six", tr.filter_options(sg, sa)),
               ("behind the model filter (attitude sensor)", "model", tr.model_filter_options(sigma_w, sg, sa)),
               ("behind the mag filter", "mag", tr.mag_filter_options(sg, SIGMA_MAG, p0_att=sa)),
               ("behind this filter at sigma_w", "this", tr.model_mag_filter_options(sigma_w, sg, SIGMA_MAG, p0_att=sa)),
               ("behind this filter at 10 x sigma_w", "this", tr.model_mag_filter_options(10.0 * sigma_w, sg, SIGMA_MAG, p0_att=sa)))
    say(f"{M} dispersed plants, {N} samples of {h} s each; 0.38 deg/s gyro, 1 deg attitude and {SIGMA_MAG:g} T magnetometer noise (the two "
        f"magnetometer filters read the attitude sensor at knot 0 only); PD gains wn = {WN} rad/s, zeta = {ZETA}; failures of {M}; rms errors "
        f"of what the law saw against the true state over the second half of the horizon (a raw sample's: {np.sqrt(3.0) * sg:.2e} rad/s, "
        f"{np.sqrt(3.0):.2f} deg):")
    out_d = dict(N=N, sigma_w=sigma_w)
    for law in LAWS:
        for latency in (0, 1):
            for label, kind, f in configs:
                kw = dict(latency=latency, sigma_mag=SIGMA_MAG, want_trajectories=f is not None, **SENSOR)
                if f is not None:
                    kw.update(filter=f, want_estimates=True)
                r = fly(law, kind, **kw)
                st = r["stats"][0]
                tail = ""
                if f is not None:
                    dw, da = _errors(r, N)
                    tail = f"; rate error {dw:.2e} rad/s, attitude error {da:.3f} deg"
                say(f"  {law}, latency {latency}, {label}: {fails(st)} of {M} fail{tail}")
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
