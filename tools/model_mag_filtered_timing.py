"""Developer tool: what the model-based rate filter costs when its attitude update is the magnetometer's — each of the four
model-mag-filtered roll-out kernels next to the model-filtered and the mag-filtered kernel of the same run, on the workload of
tools/mag_filtered_timing.py (1024 slews x 1000 knots, solved once, x 64 realisations, all five dispersions, the plan's box, the same
sensor levels and biases):
  tsat_model_mag_filtered_tv_kernel     against tsat_model_filtered_tv_kernel     and tsat_mag_filtered_tv_kernel     (Rtab = None)
  tsat_model_mag_filtered_tv_gg_kernel  against tsat_model_filtered_tv_gg_kernel  and tsat_mag_filtered_tv_gg_kernel  (with the orbit table)
  tsat_model_mag_filtered_pd_kernel     against tsat_model_filtered_pd_kernel     and tsat_mag_filtered_pd_kernel     (plan + feed-forward, Rtab = None)
  tsat_model_mag_filtered_pd_gg_kernel  against tsat_model_filtered_pd_gg_kernel  and tsat_mag_filtered_pd_gg_kernel  (with the orbit table)
HIP-event times of the roll-out kernels (the library prints them when TSAT_ENSEMBLE_TIMING=1). One warm-up of every call, then
`--rounds` alternating rounds in one process; medians, min, max and each ratio next to the run-to-run spread of the kernels' own
rounds, at latency 0 and 1. No ratio is set in advance. The figure to read this kernel against is the model-filtered kernel's time in
the same run: against it the kernel draws the magnetometer noise in every knot (under the TVLQR law too), forms C(n), Hm and three
3 x 3 products where the attitude block formed none, and carries 96 .. 144 B more scratch a lane
(profiles/ensemble/model_mag_filtered_resource_usage.txt). All three filters run with a gyro-bias state (p0_bias, sigma_u > 0), X_hat
and filt_final not asked for. Everything goes to `--out` and to stdout."""
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
ap.add_argument("--sigma-w", dest="sigma_w", type=float, default=3e-4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "model_mag_filtered_timing.txt"))
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
mfilt = tr.model_filter_options(args.sigma_w, tr.SENSOR_SIGMA_GYRO, tr.SENSOR_SIGMA_ATT, sigma_u=1e-5, p0_bias=1e-3)
nfilt = tr.model_mag_filter_options(args.sigma_w, tr.SENSOR_SIGMA_GYRO, args.sigma_mag, sigma_u=1e-5, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=1e-3)
sens = lambda lat: dict(sensor=sensor, sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=args.sigma_mag, latency=lat)
FILTERS = (("model_mag_filtered", tr.attitude_ensemble_model_mag_filtered, tr.attitude_ensemble_pd_model_mag_filtered, nfilt),
           ("model_filtered", tr.attitude_ensemble_model_filtered, tr.attitude_ensemble_pd_model_filtered, mfilt),
           ("mag_filtered", tr.attitude_ensemble_mag_filtered, tr.attitude_ensemble_pd_mag_filtered, gfilt))


def calls(law, gg):
    """name -> lat -> the call of each of the three filters' kernels of this law, with or without the orbit table"""
    orbit = dict(Rtab=Rtab, gm=GM) if gg else {}
    out = []
    for name, tv, pd, f in FILTERS:
        kern = f"tsat_{name}_{law}{'_gg' if gg else ''}_kernel"
        if law == "tv":
            out.append((kern, lambda lat, tv=tv, f=f: tv(s, b, X, U, x0s, *W, SEED, plant=plant, sat=sat, filter=f, **orbit, **sens(lat))))
        else:
            out.append((kern, lambda lat, pd=pd, f=f: pd(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, sat=sat, filter=f, **orbit, **sens(lat))))
    return out


say(f"model-mag-filtered timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, all five dispersions, noise, the plan's box; "
    f"sensor at sigma_gyro {tr.SENSOR_SIGMA_GYRO:.4g} rad/s, sigma_att {tr.SENSOR_SIGMA_ATT:.4g} rad, sigma_mag {args.sigma_mag:g}, biases on "
    f"(magnetometer 1e-6); the three filters with sigma_u 1e-5, p0_bias 1e-3, the model filters with sigma_w {args.sigma_w:g}, the magnetometer "
    f"filters with sigma_m {args.sigma_mag:g}; {args.rounds} alternating rounds after a warm-up; HIP-event times of the roll-out kernels")
for law, gg in (("tv", False), ("tv", True), ("pd", False), ("pd", True)):
    trio = calls(law, gg)
    for lat in (0, 1):
        for _, call in trio:
            call(lat)                             # warm-up
        runs = [[] for _ in trio]
        for _ in range(args.rounds):
            for v, (_, call) in zip(runs, trio):
                v.append(timed(lambda: call(lat)))
        ms = [np.array([r[0] for r in v]) for v in runs]
        fails = lambda v: int(v[-1][1]["summary"][:, 1].sum())
        for (kern, _), a, v in zip(trio, ms, runs):
            say(f"{kern}, latency {lat}:  {fmt(a)}; failures of {T * M}: {fails(v)}")
        say(f"    this kernel against the model-filtered one, medians: {np.median(ms[0]) / np.median(ms[1]):.3f} x; against the mag-filtered "
            f"one {np.median(ms[0]) / np.median(ms[2]):.3f} x; run-to-run spread (max / min) of this kernel's rounds {ms[0].max() / ms[0].min():.3f} x, "
            f"the model-filtered one's {ms[1].max() / ms[1].min():.3f} x, the mag-filtered one's {ms[2].max() / ms[2].min():.3f} x")
s.close()
