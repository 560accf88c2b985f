"""Developer tool: what the sun-vector update costs inside the magnetometer-updated model filter — each of the four
model-mag-sun-filtered roll-out kernels next to the model-mag-filtered kernel of the same run, on the workload of
tools/model_mag_filtered_timing.py (1024 slews x 1000 knots, solved once, x 64 realisations, all five dispersions, the plan's box, the
same sensor levels and biases), with the sun table LIT THROUGHOUT and HALF DARK (zero from the middle row on):
  tsat_model_mag_sun_filtered_tv_kernel     against tsat_model_mag_filtered_tv_kernel     (Rtab = None)
  tsat_model_mag_sun_filtered_tv_gg_kernel  against tsat_model_mag_filtered_tv_gg_kernel  (with the orbit table)
  tsat_model_mag_sun_filtered_pd_kernel     against tsat_model_mag_filtered_pd_kernel     (plan + feed-forward, Rtab = None)
  tsat_model_mag_sun_filtered_pd_gg_kernel  against tsat_model_mag_filtered_pd_gg_kernel  (with the orbit table)
HIP-event times of the roll-out kernels (the library prints them when TSAT_ENSEMBLE_TIMING=1). One warm-up of every call, then
`--rounds` alternating rounds in one process; medians, min, max and each ratio next to the run-to-run spread of the kernels' own
rounds, at latency 0 and 1. No ratio is set in advance: the file records the cost. Against its parent the kernel draws one more
Philox block per lit knot, forms C(n), Hs and three 3 x 3 products and makes a third `correct`; a dark knot pays the row fetch and a
uniform branch. Both filters run with a gyro-bias state (p0_bias, sigma_u > 0), X_hat and filt_final not asked for. Everything goes
to `--out` and to stdout."""
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
ap.add_argument("--sigma-sun", dest="sigma_sun", type=float, default=0.5 * np.pi / 180.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "model_mag_sun_filtered_timing.txt"))
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
nfilt = tr.model_mag_filter_options(args.sigma_w, tr.SENSOR_SIGMA_GYRO, args.sigma_mag, sigma_u=1e-5, p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=1e-3)
sfilt = tr.model_mag_sun_filter_options(args.sigma_w, tr.SENSOR_SIGMA_GYRO, args.sigma_mag, args.sigma_sun, sigma_u=1e-5,
                                        p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=1e-3)
sens = lambda lat: dict(sensor=sensor, sigma_gyro=tr.SENSOR_SIGMA_GYRO, sigma_att=tr.SENSOR_SIGMA_ATT, sigma_mag=args.sigma_mag, latency=lat)
sun_dir = np.array([0.6, -0.64, 0.48])
LIT = np.ascontiguousarray(np.broadcast_to(sun_dir, (b.Btab.shape[0], b.n_tab, 3)))
HALF = LIT.copy()
HALF[:, b.n_tab // 2:] = 0.0
FILTERS = (("model_mag_sun_filtered", "lit throughout", tr.attitude_ensemble_model_mag_sun_filtered, tr.attitude_ensemble_pd_model_mag_sun_filtered,
            sfilt, dict(Stab=LIT, sigma_sun=args.sigma_sun)),
           ("model_mag_sun_filtered", "half dark", tr.attitude_ensemble_model_mag_sun_filtered, tr.attitude_ensemble_pd_model_mag_sun_filtered,
            sfilt, dict(Stab=HALF, sigma_sun=args.sigma_sun)),
           ("model_mag_filtered", "the parent", tr.attitude_ensemble_model_mag_filtered, tr.attitude_ensemble_pd_model_mag_filtered, nfilt, {}))


def calls(law, gg):
    """(kernel, label, lat -> the call) of this family lit throughout, half dark, and of the parent, with or without the orbit table"""
    orbit = dict(Rtab=Rtab, gm=GM) if gg else {}
    out = []
    for name, label, tv, pd, f, sun in FILTERS:
        kern = f"tsat_{name}_{law}{'_gg' if gg else ''}_kernel"
        if law == "tv":
            out.append((kern, label, lambda lat, tv=tv, f=f, sun=sun: tv(s, b, X, U, x0s, *W, SEED, plant=plant, sat=sat, filter=f, **orbit,
                                                                          **sun, **sens(lat))))
        else:
            out.append((kern, label, lambda lat, pd=pd, f=f, sun=sun: pd(s, b, x0s, kd, kp, SEED, X=X, U=U, plant=plant, sat=sat, filter=f,
                                                                          **orbit, **sun, **sens(lat))))
    return out


say(f"model-mag-sun-filtered timing: {T} slews x {N} knots x {M} realisations = {T * M} closed loops, all five dispersions, noise, the plan's box; "
    f"sensor at sigma_gyro {tr.SENSOR_SIGMA_GYRO:.4g} rad/s, sigma_att {tr.SENSOR_SIGMA_ATT:.4g} rad, sigma_mag {args.sigma_mag:g}, sigma_sun "
    f"{args.sigma_sun:.4g}, biases on (magnetometer 1e-6); both filters with sigma_u 1e-5, p0_bias 1e-3, sigma_w {args.sigma_w:g}, sigma_m "
    f"{args.sigma_mag:g}, this one with sigma_s {args.sigma_sun:.4g}; the sun table lit throughout, or zero from row {b.n_tab // 2} of {b.n_tab} "
    f"on; {args.rounds} alternating rounds after a warm-up; HIP-event times of the roll-out kernels")
for law, gg in (("tv", False), ("tv", True), ("pd", False), ("pd", True)):
    trio = calls(law, gg)
    for lat in (0, 1):
        for _, _, call in trio:
            call(lat)                             # warm-up
        runs = [[] for _ in trio]
        for _ in range(args.rounds):
            for v, (_, _, call) in zip(runs, trio):
                v.append(timed(lambda: call(lat)))
        ms = [np.array([r[0] for r in v]) for v in runs]
        fails = lambda v: int(v[-1][1]["summary"][:, 1].sum())
        for (kern, label, _), a, v in zip(trio, ms, runs):
            say(f"{kern} ({label}), latency {lat}:  {fmt(a)}; failures of {T * M}: {fails(v)}")
        say(f"    against the model-mag-filtered kernel, medians: lit throughout {np.median(ms[0]) / np.median(ms[2]):.3f} x, half dark "
            f"{np.median(ms[1]) / np.median(ms[2]):.3f} x; run-to-run spread (max / min) of the rounds: lit {ms[0].max() / ms[0].min():.3f} x, "
            f"half dark {ms[1].max() / ms[1].min():.3f} x, the parent's {ms[2].max() / ms[2].min():.3f} x")
s.close()
