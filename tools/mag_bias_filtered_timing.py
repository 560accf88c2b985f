"""Developer tool: what the magnetometer-bias state costs — each of the four mag-bias-filtered roll-out kernels next to its
mag-filtered parent kernel in the same run, on the workload of tools/mag_filtered_timing.py (1024 slews x 1000 knots, solved once,
x 64 realisations, all five dispersions, the plan's box, the same sensor levels and biases):
  tsat_mag_bias_filtered_tv_kernel     against tsat_mag_filtered_tv_kernel     (tsat_tvlqr_ensemble_mag_bias_filtered / _mag_filtered, Rtab = None)
  tsat_mag_bias_filtered_tv_gg_kernel  against tsat_mag_filtered_tv_gg_kernel  (... with the orbit table)
  tsat_mag_bias_filtered_pd_kernel     against tsat_mag_filtered_pd_kernel     (tsat_pd_ensemble_mag_bias_filtered / _mag_filtered, plan + feed-forward, Rtab = None)
  tsat_mag_bias_filtered_pd_gg_kernel  against tsat_mag_filtered_pd_gg_kernel  (... with the orbit table)
HIP-event times of the roll-out kernels (the library prints them when TSAT_ENSEMBLE_TIMING=1). One warm-up of every call, then
`--rounds` alternating rounds in one process; medians, min, max and each ratio next to the spread of the parent's own rounds, at
latency 0 and 1. No ratio is set in advance: against its parent the kernel carries 27 more values a lane, propagates one more 3 x 3
block and forms a third gain and three more blocks of K S K^T per knot; this file records what that costs. Both filters run with a
gyro-bias state (p0_bias, sigma_u > 0), this one with p0_mag and sigma_c > 0 besides, X_hat and filt_final not asked for.
Everything goes to `--out` and to stdout."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TSAT_ENSEMBLE_TIMING"] = "1"
import numpy as np
from tsat_loader import load_package

load_package()
from tortoisesat_jl_amd import slew_setup as ss, tracking as tr, trajopt as to

ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=1024)
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--wn", type=float, default=0.02)
ap.add_argument("--zeta", type=float, default=1.0)
ap.add_argument("--sigma-mag", dest="sigma_mag", type=float, default=5e-7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "mag_bias_filtered_timing.txt"))
args = ap.parse_args()
LEVELS = dict(inertia_rel=0.01, axes_deg=0.2, gain_rel=0.01, misalign_deg=0.5, residual_dipole=2e-4)
SEED, A_KM, INC = 2019, ss.R_EARTH_KM + 400.0, 96.6
GM = tr.GM_EARTH
text = []


def say(line):
    print(line, flush=True)
    text.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


def timed(call):
    """(roll-out kernel ms, result) of one synchronous ensemble call, with what the library wrote to stderr parsed"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        words = f.read().decode().split()
    ms = [float(words[words.index(k) + 1]) for k in ("ensemble_kernel_ms", "pd_kernel_ms") if k in words]
    assert len(ms) == 1, words
    return ms[0], out


fmt = lambda v: f"median {np.median(v):.4f} ms (min {v.min():.4f}, max {v.max():.4f})"
opts = to.AugmentedLagrangianSolverOptions()
opts.iterations, opts.opts_uncon.iterations, opts.opts_uncon.dJ_counter_limit = 5, 10, 1
s = to.AugmentedLagrangianSolver(None, opts)
T, N, M = args.T, args.N, args.M
b = ss.workload_monte_carlo(T=T, N=N)
Rtab = ss.circular_orbit_rows(b.n_tab, 0.2, A_KM, INC)[None]
res = to.solve_(to.BatchProblem.from_arrays(b), s, want_K=False)
W = tr.tvlqr_weights(T, r=0.5e3)
x0s = tr.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
plant = tr.disperse_plant(b.Jmat, M, np.random.default_rng(7), **LEVELS)
sensor = tr.disperse_sensor(T, M, np.random.default_rng(11), gyro_bias=1e-3, att_bias_deg=0.5, mag_bias=1e-6)
kd, kp = tr.pd_gains(b.Jmat, args.wn, args.zeta)
sat = (b.ulo, b.uhi)
X, U = res["X"], res["U"]
gfilt = tr.mag_filter_options(tr.SENSOR_SIGMA_GYRO, args.sigma_mag, sigma_u=1e-5, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=1e-3)
bfilt = tr.mag_bias_filter_options(tr.SENSOR_SIGMA_GYRO, args.sigma_mag, sigma_u=1e-5, sigma_c=1e-8, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=1e-3,
                                   p0_mag=1e-6)
sens = lambda lat: dict(sensor=sensor, sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=args.sigma_mag, latency=lat)
PAIRS = [
    ("tsat_mag_bias_filtered_tv_kernel", "tsat_mag_filtered_tv_kernel",
     lambda lat: tr.attitude_ensemble_mag_filtered(s, b, X, U, x0s, *W, SEED, plant=plant, sat=sat, filter=gfilt, **sens(lat)),
     lambda lat: tr.attitude_ensemble_mag_bias_filtered(s, b, X, U, x0s, *W, SEED, plant=plant, sat=sat, filter=bfilt, **sens(lat))),
    ("tsat_mag_bias_filtered_tv_gg_kernel", "tsat_mag_filtered_tv_gg_kernel",
     lambda lat: tr.attitude_ensemble_mag_filtered(s, b, X, U, x0s, *W, SEED, plant=plant, Rtab=Rtab, gm=GM, sat=sat, filter=gfilt, **sens(lat)),
     lambda lat: tr.attitude_ensemble_mag_bias_filtered(s, b, X, U, x0s, *W, SEED, plant=plant, Rtab=Rtab, gm=GM, sat=sat, filter=bfilt,
                                                        **sens(lat))),
    ("tsat_mag_bias_filtered_pd_kernel", "tsat_mag_filtered_pd_kernel",
     lambda lat: tr.attitude_ensemble_pd_mag_filtered(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, sat=sat, filter=gfilt, **sens(lat)),
     lambda lat: tr.attitude_ensemble_pd_mag_bias_filtered(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, sat=sat, filter=bfilt, **sens(lat))),
    ("tsat_mag_bias_filtered_pd_gg_kernel", "tsat_mag_filtered_pd_gg_kernel",
     lambda lat: tr.attitude_ensemble_pd_mag_filtered(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, Rtab=Rtab, gm=GM, sat=sat, filter=gfilt,
                                                      **sens(lat)),
     lambda lat: tr.attitude_ensemble_pd_mag_bias_filtered(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, Rtab=Rtab, gm=GM, sat=sat,
                                                           filter=bfilt, **sens(lat))),
]
say(f"mag-bias-filtered timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, all five dispersions, noise, the plan's box; "
    f"sensor at sigma_gyro {tr.SENSOR_SIGMA_GYRO:.4g} rad/s, sigma_att {tr.SENSOR_SIGMA_ATT:.4g} rad, sigma_mag {args.sigma_mag:g}, biases on "
    f"(magnetometer 1e-6); both filters with sigma_u 1e-5, p0_bias 1e-3, sigma_m {args.sigma_mag:g}, this one with p0_mag 1e-6, sigma_c 1e-8; "
    f"{args.rounds} alternating rounds after a warm-up; HIP-event times of the roll-out kernels")
for new, old, parent, child in PAIRS:
    for lat in (0, 1):
        parent(lat); child(lat)                   # warm-up
        A, B = [], []
        for _ in range(args.rounds):
            A.append(timed(lambda: parent(lat)))
            B.append(timed(lambda: child(lat)))
        a, c = (np.array([r[0] for r in v]) for v in (A, B))
        fails = lambda v: int(v[-1][1]["summary"][:, 1].sum())
        say(f"{old}, latency {lat}:  {fmt(a)}; failures of {T * M}: {fails(A)}")
        say(f"{new}, latency {lat}:  {fmt(c)}; failures {fails(B)}")
        say(f"    ratio to the parent, medians: {np.median(c) / np.median(a):.3f} x; spread of the parent's own rounds (max / min) "
            f"{a.max() / a.min():.3f} x; of this kernel's {c.max() / c.min():.3f} x")
s.close()
