#!/usr/bin/env python3
"""The slew of examples/model_mag_filtered_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same
sensor figures — with a COARSE SUN SENSOR next to the magnetometer. The model-mag filter of that example reads one field vector, which
does not observe the rotation about itself: at the measured sigma_w its attitude estimate drifts. A second body vector closes that
gap while the satellite is lit, and hands over nothing in the Earth's shadow. What does the law then see, and do the loops arrive?

    python examples/model_mag_sun_filtered_slew.py [--out profiles/ensemble/model_mag_sun_filtered_failures.txt]     (needs an MI355X; under a minute)

Four configurations, each under the TVLQR law and under the PD law with the plan's feed-forward, at latency 0 and 1, at the
measured sigma_w and at 10 x it:
  raw measurements                                  tracking.attitude_ensemble_sensed / attitude_ensemble_pd_sensed
  behind the model-mag filter                       tracking.attitude_ensemble_model_mag_filtered / attitude_ensemble_pd_model_mag_filtered
  behind this filter, lit throughout                tracking.attitude_ensemble_model_mag_sun_filtered / attitude_ensemble_pd_model_mag_sun_filtered
  behind this filter, in eclipse from mid-horizon   the same calls, the sun table zero from the row of knot N / 2 on
The sensors are that example's (0.38 deg/s gyro noise, 5e-7 T magnetometer noise, one attitude fix of 1 deg, no biases) and a sun
sensor of 0.5 deg (sigma_sun = sigma_s = 0.5 pi / 180). The sun direction is ``magnetic.sun_direction`` at the default date of the
field tables; its angle to the field rows of the slew is printed. sigma_w is measured as in that example.

Printed per run: failures of 256 and, behind a filter, the rms over the realisations and the last half of the horizon of the rate
error (rad/s) and of the angle (deg) between what the law saw (X_hat) and the true state."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
from tsat_loader import load_package  # noqa: E402

load_package()
from tortoisesat_jl_amd import magnetic, tracking, trajopt as to  # noqa: E402
from dispersed_slew import LEVELS  # noqa: E402
from ensemble_slew import plan  # noqa: E402
from filtered_slew import SENSOR  # noqa: E402
from mag_filtered_slew import SIGMA_MAG  # noqa: E402
from model_filtered_slew import _errors  # noqa: E402
from sensed_slew import WN, ZETA  # noqa: E402

LAWS = ("TVLQR tracking of the plan", "PD tracking + feed-forward")
SIGMA_SUN = math.radians(0.5)
MJD = 58155.0


def sun_tables(b, N):
    """(Stab lit throughout, Stab dark from the row of knot N // 2 on, the smallest angle in degrees between the sun direction and
    a field row the slew reads)"""
    s = magnetic.sun_direction(MJD)
    rows = b.Btab[:, :b.n_tab]
    live = np.linalg.norm(rows, axis=2) > 0
    c = np.abs(rows @ s) / np.where(live, np.linalg.norm(rows, axis=2), 1.0)
    angle = float(np.degrees(np.arccos(np.minimum(c[live], 1.0)).min()))
    lit = np.ascontiguousarray(np.broadcast_to(s, (b.Btab.shape[0], b.n_tab, 3)))
    dark = lit.copy()
    first = min(max(int(math.floor(float(b.tau0[0]) + (N // 2) * float(b.dtau[0]))), 0), b.n_tab - 1)
    dark[:, first:] = 0.0
    return lit, dark, angle


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
    tv = dict(raw=tr.attitude_ensemble_sensed, model=tr.attitude_ensemble_model_filtered, mag=tr.attitude_ensemble_model_mag_filtered,
              sun=tr.attitude_ensemble_model_mag_sun_filtered)
    pd = dict(raw=tr.attitude_ensemble_pd_sensed, model=tr.attitude_ensemble_pd_model_filtered, mag=tr.attitude_ensemble_pd_model_mag_filtered,
              sun=tr.attitude_ensemble_pd_model_mag_sun_filtered)

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
    lit, dark, angle = sun_tables(b, N)
    n_dark = int(np.count_nonzero(~np.any(dark[0] != 0, axis=1)))
    say(f"sun direction of MJD {MJD:g}, {angle:.1f} deg from the nearest field row of the slew; sun sensor 0.5 deg; the eclipse table is "
        f"zero on its last {n_dark} of {b.n_tab} rows (from the row of knot {N // 2} on)")
    sg, sa = tr.SENSOR_SIGMA_GYRO, tr.SENSOR_SIGMA_ATT
    say(f"{M} dispersed plants, {N} samples of {h} s each; 0.38 deg/s gyro and {SIGMA_MAG:g} T magnetometer noise, one attitude fix of 1 deg "
        f"at knot 0; PD gains wn = {WN} rad/s, zeta = {ZETA}; failures of {M}; rms errors of what the law saw against the true state over "
        f"the second half of the horizon (a raw sample's: {np.sqrt(3.0) * sg:.2e} rad/s, {np.sqrt(3.0):.2f} deg):")
    out_d = dict(N=N, sigma_w=sigma_w)
    for scale in (1.0, 10.0):
        sw = scale * sigma_w
        mag_f = tr.model_mag_filter_options(sw, sg, SIGMA_MAG, p0_att=sa)
        sun_f = tr.model_mag_sun_filter_options(sw, sg, SIGMA_MAG, SIGMA_SUN, p0_att=sa)
        configs = (("raw measurements", "raw", None, {}),
                   ("behind the model-mag filter", "mag", mag_f, {}),
                   ("behind this filter, lit throughout", "sun", sun_f, dict(Stab=lit, sigma_sun=SIGMA_SUN)),
                   ("behind this filter, in eclipse from mid-horizon", "sun", sun_f, dict(Stab=dark, sigma_sun=SIGMA_SUN)))
        say(f" at {scale:g} x the measured sigma_w ({sw:.3e} rad/s^2):")
        for law in LAWS:
            for latency in (0, 1):
                for label, kind, f, more in configs:
                    if f is None and scale != 1.0:
                        continue                          # the raw run does not depend on sigma_w
                    kw = dict(latency=latency, sigma_mag=SIGMA_MAG, want_trajectories=f is not None, **SENSOR, **more)
                    if f is not None:
                        kw.update(filter=f, want_estimates=True)
                    r = fly(law, kind, **kw)
                    st = r["stats"][0]
                    tail = ""
                    if f is not None:
                        dw, da = _errors(r, N)
                        tail = f"; rate error {dw:.2e} rad/s, attitude error {da:.3f} deg"
                    say(f"  {law}, latency {latency}, {label}: {fails(st)} of {M} fail{tail}")
                    out_d[(scale, law, latency, label)] = st
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
