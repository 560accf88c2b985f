"""Shared pieces of tests/test_model_filtered.py (CPU tier) and tests/test_gpu_model_filtered.py (GPU tier): the ensemble controllers
behind the model-based rate filter (tsat_tvlqr_ensemble_model_filtered, tsat_pd_ensemble_model_filtered).

THE REFERENCE (``pairs_of``) is ``reference_rollout.ensemble_loop`` with the nine-state recursion of include/tortoise_hip.h
(``ModelEkf``, behind ``reference_rollout.ModelState``) between ``measure`` and the law — numpy and the oracle's primitives only
(``ol.qmult``, ``ol.inv3``, ``ol.dyn7``, ``ol.qrot``, ``ol.plant_noise``). With ``filt=None`` it has to equal
``sensed_common.pairs_of`` with max |d| = 0 (test_model_filtered.py::test_reference_with_the_filter_off_is_the_sensed_reference); it
also returns X_hat and filt_final.

The case of both tiers is ``sensed_common``'s; the filter's levels are FILT below. Every parity test first asserts its conditions on
references alone with the bar ``gg_common.MOVED`` (``conditions``): terms of the recursion are switched off through ``variant``, which
is a device of the tests, not a mode of the product.

Also: the filter as a ``filtered_common.Family``, which gives the argument lists of the two entry points (``TvCall``, ``PdCall``) and
the ctypes binding of the emulated kernels (``EmuModelFiltered``; tests/emu/tsat_emu_model_filtered.cpp)."""
import math

import numpy as np

import filtered_common as fc
import gg_common as gc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = 12
# the filter of the parity tests: the sensor's own attitude noise (sensed_common.SIGMAS), a gyro noise of 5e-3 rad/s as
# filtered_common.FILT assumes (at the sensor's own 3e-4 rad/s the gyro update is so sharp that sigma_w hardly acts), a bias random
# walk and an initial bias spread of the size of sensed_common.BIAS' gyro bias, an attitude process noise, and an un-modelled
# angular acceleration of the size the dispersed plants of the case produce against the model (1e-4 .. 1e-3 rad/s^2), so that every
# option acts
FILT = dict(sigma_v=1e-3, sigma_w=3e-4, sigma_u=1e-4, sigma_a=sc.SIGMAS["sigma_att"], sigma_g=5e-3, p0_att=math.radians(1.0),
            p0_bias=2e-3)
FAST = fc.FAST
# the sensor and filter on which the ORDER of the two updates shows. In a linear filter two updates with independent noises commute
# exactly; here the order acts only through the second-order term of the quaternion correction, (dtheta_a x dtheta_b) / 2, which at
# the parity levels (0.3 deg, 3e-4 rad/s) moves the final state by 1e-9 .. 4e-8 whatever the starts. At three times the reference's
# own sensor figures (3 deg, 2e-2 rad/s) it moves it by 2e-7 .. 2e-6 under both laws and latencies.
LOUD_SENS = dict(sigma_gyro=2e-2, sigma_att=math.radians(3.0), sigma_mag=5e-7)
LOUD_FILT = dict(sigma_v=1e-3, sigma_w=3e-4, sigma_u=1e-4, sigma_a=math.radians(3.0), sigma_g=2e-2, p0_att=math.radians(3.0), p0_bias=2e-3)
VARIANT = dict(command=True, gyroscopic=True, cross=True, order="ab", predict=True)


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _sym(P):
    """the matrix the upper triangle of P stands for"""
    return np.triu(P) + np.triu(P, 1).T


class ModelEkf:
    """the recursion of include/tortoise_hip.h, line for line; error state (dtheta, dw, db), P 9 x 9"""

    def __init__(self, ol, h, J, us, filt, variant=VARIANT):
        self.ol, self.h, self.J, self.us, self.f, self.v = ol, float(h), np.asarray(J, dtype=np.float64), float(us), filt, variant

    def first(self, w_m, q_m):
        f, I, Z = self.f, np.eye(3), np.zeros((3, 3))
        self.q = q_m / math.sqrt(float(q_m @ q_m))
        self.w = np.array(w_m, dtype=np.float64)
        self.b = np.zeros(3)
        a, d, g = f["p0_att"] ** 2, f["p0_bias"] ** 2, f["sigma_g"] ** 2
        c = -d if self.v["cross"] else 0.0
        self.P = np.block([[a * I, Z, Z], [Z, (g + d) * I, c * I], [Z, c * I, d * I]])

    def predict(self, u, rows):
        """``rows``: the field rows of the knot being crossed at c = 0, 1/2, 1"""
        ol, h, f, J, I, Z = self.ol, self.h, self.f, self.J, np.eye(3), np.zeros((3, 3))
        w = self.w
        d = fc.dq_of(h * w)
        V = _skew(d[1:4])
        F = (I + 2 * d[0] * V + 2 * V @ V).T                                           # C(h w^)^T
        G = I + h * ol.inv3(J) @ (_skew(J @ w) - _skew(w) @ J) if self.v["gyroscopic"] else I
        uu = np.asarray(u, dtype=np.float64) if self.v["command"] else np.zeros(3)
        x = np.r_[w, self.q]
        b0, b1, b2 = rows
        k1 = h * ol.dyn7(x, uu, b0, J, self.us)
        k2 = h * ol.dyn7(x + k1 / 2, uu, b1, J, self.us)
        k3 = h * ol.dyn7(x + k2 / 2, uu, b1, J, self.us)
        k4 = h * ol.dyn7(x + k3, uu, b2, J, self.us)
        x = x + (k1 + 2 * k2 + 2 * k3 + k4) / 6
        self.w, self.q = x[:3], x[3:7] / math.sqrt(float(x[3:7] @ x[3:7]))
        Phi = np.block([[F, h * I, Z], [Z, G, Z], [Z, Z, I]])
        Q = np.diag(np.r_[np.full(3, (f["sigma_v"] * h) ** 2), np.full(3, (f["sigma_w"] * h) ** 2), np.full(3, f["sigma_u"] ** 2)])
        self.P = _sym(Phi @ self.P @ Phi.T + Q)

    def _apply(self, PH, S, z):
        ol = self.ol
        K = PH @ ol.inv3(S)
        dl = K @ z
        qp = ol.qmult(self.q, np.r_[1.0, dl[0:3] / 2])
        self.q = qp / math.sqrt(float(qp @ qp))
        self.w = self.w + dl[3:6]
        self.b = self.b + dl[6:9]
        self.P = _sym(self.P - K @ S @ K.T)

    def _attitude(self, q_m):
        ol, f, P = self.ol, self.f, self.P
        e = ol.qmult(np.r_[self.q[0], -self.q[1:4]], q_m / math.sqrt(float(q_m @ q_m)))
        z = 2.0 * (-1.0 if e[0] < 0 else 1.0) * e[1:4]
        self._apply(P[:, 0:3], P[0:3, 0:3] + f["sigma_a"] ** 2 * np.eye(3), z)

    def _gyro(self, w_m):
        f, P = self.f, self.P
        z = w_m - (self.w + self.b)
        S = P[3:6, 3:6] + P[3:6, 6:9] + P[3:6, 6:9].T + P[6:9, 6:9] + f["sigma_g"] ** 2 * np.eye(3)
        self._apply(P[:, 3:6] + P[:, 6:9], S, z)

    def update(self, w_m, q_m):
        if self.v["order"] == "ab":
            self._attitude(q_m)
            self._gyro(w_m)
        else:
            self._gyro(w_m)
            self._attitude(q_m)

    def final(self):
        d = np.sqrt(np.diag(self.P))
        return np.r_[self.b, d]


def estimator(ol, batch, opts, filt, variant=VARIANT):
    """t -> the estimator of one loop of slew t: ``ModelEkf`` on the MODEL's inertia behind ``reference_rollout.ModelState``.
    ``filt`` None: the raw measurement. Of ``variant`` the filter takes its terms and the adapter ``predict``"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    return lambda t: rr.ModelState(ModelEkf(ol, float(batch.dt[t]), np.asarray(batch.Jmat[t]).reshape(3, 3).T, float(opts.u_scale), filt,
                                            variant), variant["predict"])


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, filt=None, variant=VARIANT, **kw):
    """``filtered_common.pairs_of`` behind this filter: its dict with filt_final (n, 12)"""
    return rr.pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, est=estimator(ol, batch, opts, filt, variant), **kw)


# the terms a parity test shows to act, as (label, what replaces in the call of ``ref_of``); the latency-1 one is added there
def terms_of(filt):
    return [
        ("sigma_w against three times it", dict(filt=dict(filt, sigma_w=3.0 * filt["sigma_w"]))),
        ("sigma_g against three times it", dict(filt=dict(filt, sigma_g=3.0 * filt["sigma_g"]))),
        ("sigma_u with p0_bias against three times them", dict(filt=dict(filt, sigma_u=3.0 * filt["sigma_u"], p0_bias=3.0 * filt["p0_bias"]))),
        (COMMAND, dict(variant=dict(VARIANT, command=False))),
        (GYROSCOPIC, dict(variant=dict(VARIANT, gyroscopic=False))),
        ("the -p0_bias^2 cross block of first against none", dict(variant=dict(VARIANT, cross=False))),
        (ORDER, dict(variant=dict(VARIANT, order="ba"))),
    ]


COMMAND = "the command in predict against u = 0"
GYROSCOPIC = "the gyroscopic term of Phi_ww against Phi_ww = I"
ORDER = "the update order a, b against b, a"
DELAY = ("the prediction across the delay against y_k = posterior", dict(latency=1, variant=dict(VARIANT, predict=False)))


def moved(ref, other):
    """max |d final state| between two references of the same pairs"""
    n = ref["n_knots"]
    i = np.arange(len(n))
    return float(np.max(np.abs(ref["X_sim"][i, n - 1] - other["X_sim"][i, n - 1])))


def conditions(ref_of, sensor, latency, skip=(), filt=FILT):
    """the conditions of a parity test on references alone (bar gg_common.MOVED on the final states). ``ref_of(**over)`` is the
    reference of the test's call with the named arguments replaced; the call flies sensor biases ``sensor`` with a gyro bias in them.
    Filtered against raw moves the final state, and so does each of ``terms_of(filt)``; at latency 1 also DELAY. ``skip`` names the
    labels that the test leaves to the one that flies the case on which they show (the FAST starts, the LOUD sensor): their figures
    are printed. Returns the reference of the call itself."""
    assert np.abs(sensor[..., 0:3]).min() > 0, "the conditions on sigma_u and p0_bias need a gyro bias"
    ref = ref_of()
    terms = [("filtered against raw", dict(filt=None))] + terms_of(filt) + ([DELAY] if latency else [])
    short = []
    for label, over in terms:
        d = moved(ref, ref_of(**over))
        print(f"  condition: {label}: max|d final state| {d:.2e}" + ("  (left to the case that shows it)" if label in skip else ""))
        if label not in skip and not d >= gc.MOVED:
            short.append(f"{label} moves the final state by {d:.2e} only")
    assert not short, short
    return ref


def compare_estimates(ref, got, pairs, idx=None):
    """X_hat and filt_final against the reference to 1e-9, the project's bar for these loops; X_hat zero from the last knot on"""
    assert got["filt_final"].shape[-1] == FILTER_W
    fc.compare_estimates(ref, got, pairs, idx)


def filter_options(abi, filt):
    return abi.ModelFilterOptions(sigma_v=filt["sigma_v"], sigma_w=filt["sigma_w"], sigma_u=filt["sigma_u"], sigma_a=filt["sigma_a"],
                                  sigma_g=filt["sigma_g"], p0_att=filt["p0_att"], p0_bias=filt["p0_bias"], reserved=0)


def first_record(filt):
    """filt_final when no update was made"""
    return np.r_[np.zeros(3), np.full(3, filt["p0_att"]), np.full(3, math.sqrt(filt["sigma_g"] ** 2 + filt["p0_bias"] ** 2)),
                 np.full(3, filt["p0_bias"])]


FAMILY = fc.Family(filter_options, FILTER_W, FILT, "model_filtered", "emu_model_filter_check")
TvCall, PdCall, EmuModelFiltered = fc.bindings(FAMILY)


def filter_rejections(call):
    """what check_model_filter and the entry points reject of the filter arguments, as (label, edited call, words of the text)"""
    abi, f = call.abi, call.v["f"]

    def fo(**kw):
        o = abi.ModelFilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), "must be finite and >= 0"),
        ("sigma_w negative", call.edit(f=fo(sigma_w=-1e-6)), "must be finite and >= 0"),
        ("sigma_w inf", call.edit(f=fo(sigma_w=float("inf"))), "must be finite and >= 0"),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), "must be finite and >= 0"),
        ("sigma_a negative", call.edit(f=fo(sigma_a=-1e-3)), "must be finite and >= 0"),
        ("sigma_g NaN", call.edit(f=fo(sigma_g=float("nan"))), "must be finite and >= 0"),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), "must be finite and >= 0"),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), "must be finite and >= 0"),
        ("sigma_a zero", call.edit(f=fo(sigma_a=0.0)), "sigma_a must be > 0"),
        ("sigma_g zero", call.edit(f=fo(sigma_g=0.0)), "sigma_g must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
    ]


# the long horizon: sigma_w chosen on the reference (tests/test_model_filtered.py prints the ratio it gives)
LONG_SIGMA_W = 3e-4


def long_case(pkg, ol, N, M):
    """``filtered_common.long_case`` (T = 1, the PD law regulating on the model's plant with plant noise, the reference's sensor
    figures, a gyro bias of filtered_common.GYRO_BIAS in a drawn direction, latency 0) flown behind this filter — sigma_g, sigma_a =
    p0_att the sensor's figures, p0_bias the bias' size, sigma_w = LONG_SIGMA_W — next to the six-state reference on the same draws"""
    c = fc.long_case(pkg, ol, N, M)
    tr = pkg.tracking
    filt = dict(sigma_v=0.0, sigma_w=LONG_SIGMA_W, sigma_u=0.0, sigma_a=tr.SENSOR_SIGMA_ATT, sigma_g=tr.SENSOR_SIGMA_GYRO,
                p0_att=tr.SENSOR_SIGMA_ATT, p0_bias=fc.GYRO_BIAS)
    kw = dict(c["kw"], filt=filt)
    ref = pairs_of(ol, pkg._abi, "pd", c["b"], c["x0s"], (sc.KD, sc.KP), c["o"], c["pairs"], **kw)
    return dict(c, kw=kw, ref=ref, six=c["ref"])


def assert_filter_works(c):
    """on the references alone, over the last half of the horizon: the rms rate error of the estimate is below a quarter of the raw
    sample's; the rms attitude error is no worse than the six-state reference's on the same draws within 10 %; the bias estimate is
    inside 3 x its own sqrt(diag P_bb) on every realisation"""
    ref, six, N = c["ref"], c["six"], c["b"].N
    half = slice(N // 2, N - 1)
    we, wr, ae, a6 = [], [], [], []
    for i, (t, m) in enumerate(c["pairs"]):
        true = ref["X_sim"][i, half]
        we.append(np.mean(np.sum((ref["X_hat"][i, half, 0:3] - true[:, 0:3]) ** 2, axis=1)))
        wr.append(np.mean(np.sum((ref["Y_raw"][i, half, 0:3] - true[:, 0:3]) ** 2, axis=1)))
        ae.append(np.mean(fc._angles(ref["X_hat"][i, half, 3:7], true[:, 3:7]) ** 2))
        a6.append(np.mean(fc._angles(six["X_hat"][i, half, 3:7], six["X_sim"][i, half, 3:7]) ** 2))
    we, wr, ae, a6 = (math.sqrt(float(np.mean(v))) for v in (we, wr, ae, a6))
    print(f"rms over the last half: rate error of the estimate {we:.2e} rad/s against the raw sample's {wr:.2e}: ratio "
          f"{we / wr:.3f}; attitude error {math.degrees(ae):.3f} deg against the six-state reference's {math.degrees(a6):.3f} deg")
    assert we < 0.25 * wr, "the filter does not smooth the gyro noise"
    assert ae <= 1.10 * a6, "the attitude estimate is worse than the six-state filter's"
    pr = c["pairs"]
    db = np.abs(ref["filt_final"][:, 0:3] - c["sensor"][pr[:, 0], pr[:, 1], 0:3])
    print(f"|b^ - bw| / sqrt(diag P_bb) at the end: max {float(np.max(db / ref['filt_final'][:, 9:12])):.2f}")
    assert np.all(db < 3.0 * ref["filt_final"][:, 9:12]), "the bias estimate is outside 3 sigma of its own covariance"
