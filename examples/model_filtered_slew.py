#!/usr/bin/env python3
"""The slew of examples/filtered_slew.py — same 256 dispersed plants, same starts, same generator ids, same limits, same sensor
levels — behind the MODEL-BASED rate filter: is the white gyro noise, which the six-state filter cannot smooth, what makes these
loops fail?

    python examples/model_filtered_slew.py [--out profiles/ensemble/model_filtered_failures.txt]     (needs an MI355X; a few seconds)

The filter is the nine-state one of include/tortoise_hip.h (tracking.attitude_ensemble_model_filtered ->
tsat_tvlqr_ensemble_model_filtered, tracking.attitude_ensemble_pd_model_filtered -> tsat_pd_ensemble_model_filtered): the body rate
is a state, propagated by the model's plant under the command just issued; the gyro and the attitude sensor are measurements, at the
sensor's own figures (sigma_g = 0.38 pi / 180 rad/s, sigma_a = p0_att = pi / 180 rad), no bias state.

sigma_w, the un-modelled angular acceleration the filter assumes, is measured on the example's own dispersed plants first: one run
with the ideal sensor at latency 1 and a filter that trusts its measurements entirely (sigma_g = sigma_a = 1e-9, sigma_w = sigma_v =
1), so that X_hat[k] is the model's one-step prediction from the true state of knot k - 1 under the command flown there, and
(X_hat - X_sim)[k, 0:3] / h is what the model does not know: inertia and actuator mismatch, residual dipole, plant noise. Its rms
per axis is the example's sigma_w; the counts are shown at that value, at 10 x and at 0.1 x of it.

Printed, for the TVLQR law and for the PD law with the plan's feed-forward, at latency 0 and 1: failures of 256 under raw
measurements, behind the six-state filter, behind this filter, and under raw measurements with sigma_gyro = 0 in the sensor — the run
that says whether the gyro noise is the cause; and the rms rate and attitude error of X_hat against X_sim next to the raw sample's.

What it showed on an MI355X (profiles/ensemble/model_filtered_failures.txt): the counts do not move, with the filter or without any
gyro noise, so the gyro noise is not the cause; and the measured rms is too small a sigma_w, because the un-modelled acceleration of
these plants is a slowly varying torque and not white — the estimate is best at 10 x of it."""
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
from sensed_slew import WN, ZETA  # noqa: E402

SENSOR = dict(sigma_gyro=tracking.SENSOR_SIGMA_GYRO, sigma_att=tracking.SENSOR_SIGMA_ATT)
LAWS = ("TVLQR tracking of the plan", "PD tracking + feed-forward")


def _errors(r, N):
    """rms over realisations and the knots of the second half of |w^ - w| (rad/s) and of the angle between q^ and q (deg)"""
    half = slice(N // 2, N - 1)
    xh, xs = r["X_hat"][0][:, half], r["X_sim"][0][:, half]
    dw = np.sqrt(np.mean(np.sum((xh[..., 0:3] - xs[..., 0:3]) ** 2, axis=-1)))
    c = np.abs(np.sum(xh[..., 3:7] * xs[..., 3:7], axis=-1)) / (np.linalg.norm(xh[..., 3:7], axis=-1) * np.linalg.norm(xs[..., 3:7], axis=-1))
    ang = np.sqrt(np.mean((2.0 * np.arccos(np.minimum(c, 1.0))) ** 2))
    return float(dw), float(np.degrees(ang))


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
    h = float(b.dt[0])
    fails = lambda st: int(np.count_nonzero(st["failed"]))

    def fly(law, fn_tv, fn_pd, **kw):
        if law.startswith("TVLQR"):
            return fn_tv(solver, b, res["X"], res["U"], x0_lqr, Ql, Qfl, Rl, 1, plant=plant, sat=sat, **kw)
        return fn_pd(solver, b, x0_lqr, kd, kp, 1, X=res["X"], U=res["U"], plant=plant, sat=sat, **kw)

    model = lambda law, **kw: fly(law, tracking.attitude_ensemble_model_filtered, tracking.attitude_ensemble_pd_model_filtered, **kw)
    six = lambda law, **kw: fly(law, tracking.attitude_ensemble_filtered, tracking.attitude_ensemble_pd_filtered, **kw)
    raw = lambda law, **kw: fly(law, tracking.attitude_ensemble_sensed, tracking.attitude_ensemble_pd_sensed, **kw)

    # sigma_w from the plants themselves: the model's one-step prediction from the truth against the truth
    probe = tracking.model_filter_options(1.0, 1e-9, 1e-9, sigma_v=1.0, p0_att=0.0)
    acc = []
    for law in LAWS:
        r = model(law, latency=1, filter=probe, want_trajectories=True, want_estimates=True)
        d = (r["X_hat"][0][:, 1:N - 1, 0:3] - r["X_sim"][0][:, 1:N - 1, 0:3]) / h
        acc.append(float(np.sqrt(np.mean(d ** 2))))
        say(f"un-modelled angular acceleration of the {M} plants under {law}: rms per axis {acc[-1]:.3e} rad/s^2")
    sigma_w = float(np.sqrt(np.mean(np.square(acc))))
    say(f"sigma_w of the example: {sigma_w:.3e} rad/s^2 (rms of the two)")
    say(f"{M} dispersed plants, {N} samples of {h} s each; 0.38 deg/s gyro and 1 deg attitude noise; PD gains wn = {WN} rad/s, "
        f"zeta = {ZETA}; failures of {M}; rms errors of what the law saw against the true state over the second half of the horizon "
        f"(a raw sample's: {np.sqrt(3.0) * tracking.SENSOR_SIGMA_GYRO:.2e} rad/s, {np.sqrt(3.0):.2f} deg):")
    f6 = tracking.filter_options(tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
    out_d = dict(N=N, sigma_w=sigma_w)
    for law in LAWS:
        for latency in (0, 1):
            kw = dict(latency=latency, **SENSOR)
            st = raw(law, **kw)["stats"][0]
            say(f"  {law}, latency {latency}, raw measurements: {fails(st)} of {M} fail")
            out_d[(law, latency, "raw")] = st
            r = six(law, filter=f6, want_trajectories=True, want_estimates=True, **kw)
            dw, da = _errors(r, N)
            say(f"  {law}, latency {latency}, six-state filter: {fails(r['stats'][0])} of {M} fail; rate error {dw:.2e} rad/s (its rate is the "
                f"raw gyro sample), attitude error {da:.3f} deg")
            out_d[(law, latency, "six-state")] = r["stats"][0]
            for scale in (1.0, 10.0, 0.1):
                fo = tracking.model_filter_options(scale * sigma_w, tracking.SENSOR_SIGMA_GYRO, tracking.SENSOR_SIGMA_ATT)
                r = model(law, filter=fo, want_trajectories=True, want_estimates=True, **kw)
                dw, da = _errors(r, N)
                ff = r["filt_final"][0]
                say(f"  {law}, latency {latency}, model-based filter at {scale:g} x sigma_w: {fails(r['stats'][0])} of {M} fail; rate error "
                    f"{dw:.2e} rad/s, attitude error {da:.3f} deg; median sqrt(diag P_ww) at the end {np.median(ff[:, 6:9]):.2e} rad/s, "
                    f"sqrt(diag P_tt) {np.degrees(np.median(ff[:, 3:6])):.3f} deg")
                out_d[(law, latency, f"model x{scale:g}")] = r["stats"][0]
            st = raw(law, latency=latency, sigma_gyro=0.0, sigma_att=tracking.SENSOR_SIGMA_ATT)["stats"][0]
            say(f"  {law}, latency {latency}, raw measurements with sigma_gyro = 0 in the sensor: {fails(st)} of {M} fail")
            out_d[(law, latency, "raw, no gyro noise")] = st
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
