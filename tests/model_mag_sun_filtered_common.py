"""Shared pieces of tests/test_model_mag_sun_filtered.py (CPU tier) and tests/test_gpu_model_mag_sun_filtered.py (GPU tier): the
ensemble controllers behind the magnetometer-updated model filter WITH A SUN SENSOR THAT ECLIPSE BLINDS
(tsat_tvlqr_ensemble_model_mag_sun_filtered, tsat_pd_ensemble_model_mag_sun_filtered).

THE REFERENCE (``pairs_of``): ``reference_rollout.ensemble_loop`` does not hand the estimator the true state, which the sun sample is
formed from, and that file stays as it is; so the loop is restated ONCE here (``loop``) from ``rr.plant_step``, ``rr.limit``,
``rr.LAWS`` and ``sc.measure``, with the sun sample of include/tortoise_hip.h drawn beside the measurement. With the sun table None or
all zero it has to equal ``model_mag_filtered_common.pairs_of`` with max |d| = 0 (tests/test_model_mag_sun_filtered.py). The recursion
is ``ModelMagSunEkf``: ``model_mag_filtered_common.ModelMagEkf`` and ``_sun``, block a. with (s_j, s_m, sigma_s) in the places of
(r_j, b_m, sigma_m), behind ``SunState``, the parent's sequencing handing over the sun sample and the row it was formed with. Numpy
and the oracle's primitives only.

THE CASE is the parent's (``pd_common.case``: 8 slews, N = 20, ragged horizons 20 13 6 7 20 19 6 20, two field tables, M = 63 and
64, all five plant dispersions, plant noise on, gravity on, ``sensed_common`` levels, ``model_mag_filtered_common.FILT``) with
sigma_s = sigma_sun = SIGMA_SUN (0.5 deg) and ``sun_table``: one sun direction per field table, at least 20 deg from every field row
the case reads (asserted on the inputs), and an eclipse window per table in different places: under the case's clock (row
floor(0.25 + 0.9 k)) rows 5 .. 10 of table 0 are zero — knots 6 .. 11 of its slews are dark — and rows 2 .. 4 of table 1 — knots
2 .. 5 of its slews. ``assert_lit_and_dark`` asserts that every compared slew whose horizon holds the six updates has at least three
lit and three dark ones; the slews of 6 and 7 knots make at most five updates and cannot: those on table 1 have lit and dark
updates, those on table 0 end before its window and are lit throughout.

Every parity test first asserts its conditions on references alone with the bar ``gg_common.MOVED`` (``conditions``); a label that
does not show on the case would get a case of its own; all five show here, and the pairing of the delayed sun sample is flown on
``pairing_table`` besides, where a wrong pairing drops an update or feeds in a sample that never existed."""
import ctypes as C
import dataclasses
import math

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import filtered_common as fc
import gg_common as gc
import mag_filtered_common as gfc
import model_filtered_common as mfc
import model_mag_filtered_common as mc
import mpc_held_common as hc
import pd_common as pc
import reference_rollout as rr
import sensed_common as sc

FILTER_W = 12
SIGMA_SUN = math.radians(0.5)
FILT = dict(mc.FILT, sigma_s=SIGMA_SUN)
LEVELS = ("sigma_v", "sigma_w", "sigma_u", "sigma_g", "sigma_m", "sigma_s", "p0_att", "p0_bias")
VARIANT = dict(mc.VARIANT, sun=True)          # ``sun`` False leaves the sun update out
MIN_ANGLE = math.radians(20.0)
KINDS = mc.KINDS
cut, nomp, moved, first_record = mc.cut, mc.nomp, mc.moved, mc.first_record


class ModelMagSunEkf(mc.ModelMagEkf):
    """the recursion of include/tortoise_hip.h: the parent's ``update`` (a. magnetometer, b. gyro), then c. ``_sun`` where the row
    is not zero"""

    def __init__(self, ol, h, J, us, filt, variant=VARIANT):
        super().__init__(ol, h, J, us, filt, variant)

    def _sun(self, s_m, s):
        if not self.v["sun"]:
            return
        ol, f, P = self.ol, self.f, self.P
        n = self.q / math.sqrt(float(self.q @ self.q))
        z = s_m - ol.qrot(n, s)
        Hs = gfc.h_matrix(n, s)
        PH = P[:, 0:3] @ Hs.T
        S = mfc._sym(Hs @ PH[0:3]) + f["sigma_s"] ** 2 * np.eye(3)
        self._apply(PH, S, z)

    def update(self, w_m, b_m, r, s_m=None, s=None):
        super().update(w_m, b_m, r)
        if s is not None and np.any(s != 0.0):                 # a dark knot: no sample exists and no update is made
            self._sun(np.zeros(3) if s_m is None else s_m, s)  # (None only under the wrong pairing, a condition of the tests)


class SunState(mc.ModelMagState):
    """``model_mag_filtered_common.ModelMagState``'s sequencing, each update also against the sun sample and the sun row it was
    formed with (``sun`` = (s_m, its own row s_{k-1} for the delayed sample of latency 1, the row s_k of the knot)).
    ``sun_own_row`` False pairs the delayed sample with s_k: a condition of the tests"""

    def __init__(self, ekf, predict=True, pair_own_row=True, sun_own_row=True):
        super().__init__(ekf, predict, pair_own_row)
        self.sun_own_row = sun_own_row

    def sample(self, k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev, sun=None):
        e = self.ekf
        r = row_m if self.pair_own_row else rows[0]
        s_m, s_own, s_now = (None, None, None) if sun is None else sun
        s = s_own if self.sun_own_row else s_now
        if k == 0:
            e.first(w_m, q_m)
            e.u = np.zeros(3)
            self.fin, post = e.final(), (e.w, e.q)
        elif latency:
            if k > 1:                                       # m_0 handed over a second time: no update
                e.update(w_m, b_m, r, s_m, s)
            self.fin, post = e.final(), (e.w, e.q)
            self._predict(u_prev, rows_prev)
        else:
            self._predict(u_prev, rows_prev)
            e.update(w_m, b_m, r, s_m, s)
            self.fin, post = e.final(), (e.w, e.q)
        return (e.w, e.q) if self.predict else post


def estimator(ol, batch, opts, filt, variant=VARIANT, pair_own_row=True, sun_own_row=True):
    """t -> the estimator of one loop of slew t. ``filt`` None: the raw measurement"""
    if filt is None:
        return lambda t: rr.Raw(FILTER_W)
    return lambda t: SunState(ModelMagSunEkf(ol, float(batch.dt[t]), np.asarray(batch.Jmat[t]).reshape(3, 3).T, float(opts.u_scale), filt,
                                             variant), variant["predict"], pair_own_row, sun_own_row)


def row_index(batch, t, k):
    """the index of the stage-0 row of knot k in the slew's tables: ``dispersed_common._row``'s, found by running it on a table
    of indices"""
    idx = np.broadcast_to(np.arange(batch.n_tab, dtype=np.float64)[None, :, None], (batch.Btab.shape[0], batch.n_tab, 3))
    return int(dc._row(dataclasses.replace(batch, Btab=idx), t, k, 0.0)[0])


def sun_row(batch, Stab, t, k):
    """s_k: the stage-0 row of knot k in the slew's sun table, on the clock of the field table"""
    return Stab[batch.btab_idx[t], row_index(batch, t, k)]


def sun_sample(ol, x, s, opts, gid, k, sigma_sun, noisy):
    """s_m of the true state x at a lit knot: qrot(x[3:7] / |x[3:7]|, s_k) + sigma_sun n_s, n_s the gyro triple of stage index 6"""
    n_s = ol.plant_noise(int(opts.noise_seed), int(gid), k, 6, sigma_sun, 0.0, 0.0)[0:3] if noisy else np.zeros(3)
    return ol.qrot(x[3:7] / math.sqrt(float(x[3:7] @ x[3:7])), s) + n_s


def loop(ol, law, batch, t, Xr, Ur, gains, x0, opts, gid, Rtab=None, gm=0.0, plant=None, lo=None, hi=None, limit_mode=0, noisy=True,
         sens=None, latency=0, bias=None, est=None, Stab=None, sigma_sun=0.0):
    """``reference_rollout.ensemble_loop`` under a sensor (``sens`` given), restated with the sun sensor: per knot one sun sample
    where the row s_k of ``Stab`` is not zero, held one knot at ``latency`` 1 with its own row, handed to ``est.sample`` as
    ``sun`` = (s_m, its row, s_k) when the estimator is a ``SunState``. Returns a ``reference_rollout.Rollout``."""
    NS = batch.N
    N = NS if batch.n_knots is None else int(batch.n_knots[t])
    us, h = float(opts.u_scale), float(batch.dt[t])
    P = rr.plant_of(batch, t, plant)
    est = rr.Raw() if est is None else est
    Xs, Uc, Xh, Ym = np.zeros((NS, 7)), np.zeros((NS - 1, 3)), np.zeros((NS, 7)), np.zeros((NS, 7))
    x = np.array(x0, dtype=np.float64)
    n_sure = n_maybe = 0
    betas = []
    held = held_sun = u_prev = rows_prev = None
    for k in range(N - 1):
        Xs[k] = x
        xr = batch.xf[t] if Xr is None else Xr[k]
        rows = rr.rows_of(batch, t, k)
        row_m = rows[0]
        y = sc.measure(ol, batch, t, k, x, opts, gid, sens, bias, noisy)
        sun = None
        if Stab is not None:
            s_k = sun_row(batch, Stab, t, k)
            lit = bool(np.any(s_k != 0.0))
            sun = (sun_sample(ol, x, s_k, opts, gid, k, sigma_sun, noisy) if lit else None, s_k)
        if latency and held is not None:                                    # y_max(k-1, 0), and the rows it was formed with
            y, held, row_m = held, y, rows_prev[0]
            sun, held_sun = held_sun, sun
        else:
            held, held_sun = y, sun
        w_m, q_m, b_m = y
        Ym[k] = np.r_[w_m, q_m]
        if isinstance(est, SunState):
            w, q = est.sample(k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev,
                              None if sun is None else (sun[0], sun[1], sun_row(batch, Stab, t, k)))
        else:
            w, q = est.sample(k, latency, w_m, q_m, b_m, row_m, rows, rows_prev, u_prev)
        if est.estimates:
            Xh[k] = np.r_[w, q]
        u = rr.LAWS[law](ol, xr, None if Ur is None else Ur[k], gains[k] if law == "tv" else gains, w, q, b_m, us, True)
        Uc[k] = u
        u, (sure, maybe), beta = rr.limit(u, lo, hi, limit_mode)
        n_sure, n_maybe = n_sure + sure, n_maybe + maybe
        if beta is not None:
            betas.append(beta)
        u_prev, rows_prev = np.array(u, dtype=np.float64), rows
        x = rr.plant_step(ol, batch, t, k, x, u, P, us, h, opts, gid, k, noisy, Rtab, gm)
    Xs[N - 1] = x
    return rr.Rollout(Xs, (n_sure, n_maybe), Uc, betas, Xh, est.final(), Ym)


def pairs_of(ol, abi, law, batch, x0_sim, gains, opts, pairs, X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=None, limit_mode=0,
             x0_nom=None, noise_id0=None, sens=None, latency=0, sensor=None, filt=None, variant=VARIANT, pair_own_row=True,
             sun_own_row=True, Stab=None, sigma_sun=0.0):
    """``reference_rollout.pairs_of`` around ``loop``: its dict; m = -1 is the noise-free model plant with the ideal sensors"""
    T, M = x0_sim.shape[:2]
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    if law == "pd":
        gains = (np.broadcast_to(gains[0], (T, 3)), np.broadcast_to(gains[1], (T, 3)))
    est = estimator(ol, batch, opts, filt, variant, pair_own_row, sun_own_row)
    ol.load()
    res = []
    for p in pairs:
        t, m = int(p[0]), int(p[1])
        g = gains[t] if law == "tv" else (gains[0][t], gains[1][t])
        kw = dict(lo=None if lo is None else lo[t], hi=None if hi is None else hi[t], limit_mode=limit_mode, sens=sens, latency=latency,
                  est=est(t), Stab=Stab, sigma_sun=sigma_sun)
        Xr, Ur = None if X is None else X[t], None if U is None else U[t]
        if m < 0:
            x0 = x0_nom[t] if x0_nom is not None else X[t, 0]
            res.append(loop(ol, law, batch, t, Xr, Ur, g, x0, opts, 0, Rtab, gm, None, noisy=False, **kw))
        else:
            res.append(loop(ol, law, batch, t, Xr, Ur, g, x0_sim[t, m], opts, id0[t] + m, Rtab, gm,
                            None if plant is None else plant[t, m], bias=None if sensor is None else sensor[t, m], **kw))
    pairs = np.asarray(pairs)
    Xs = np.stack([r.X_sim for r in res])
    nk = ec.horizons(batch)[pairs[:, 0]]
    xf = batch.xf[pairs[:, 0]]
    st = dc.stats_of(abi, Xs, xf, nk, batch.dt[pairs[:, 0]], opts.min_steps, opts.w_tol, opts.angle_tol)
    return dict(X_sim=Xs, stats=st, n_sure=np.array([r.clips[0] for r in res]), n_maybe=np.array([r.clips[1] for r in res]), xf=xf,
                n_knots=nk, U_cmd=np.stack([r.U_cmd for r in res]), betas=[r.betas for r in res], X_hat=np.stack([r.X_hat for r in res]),
                filt_final=np.stack([r.filt_final for r in res]), Y_raw=np.stack([r.Y_raw for r in res]))


# ---- the sun tables of the case ------------------------------------------------------------------------------------------------

DARK_ROWS = {0: (5, 10), 1: (2, 4)}          # first and last zero row of each table's eclipse window


def angle_to_rows(s, rows):
    """the smallest angle between the line of s and the lines of the non-zero ``rows`` (n, 3)"""
    rows = rows[np.any(rows != 0.0, axis=1)]
    c = np.abs(rows @ s) / (np.linalg.norm(rows, axis=1) * np.linalg.norm(s))
    return float(np.min(np.arccos(np.minimum(c, 1.0))))


def sun_directions(batch, min_angle=MIN_ANGLE, seed=23):
    """one unit vector per field table, drawn until it is ``min_angle`` from (the line of) every row of that table"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch.Btab.shape[0]):
        for _ in range(1000):
            s = rng.standard_normal(3)
            s /= np.linalg.norm(s)
            if angle_to_rows(s, batch.Btab[i, :batch.n_tab]) >= min_angle:
                break
        else:
            raise AssertionError("no sun direction away from the field rows")
        out.append(s)
    return np.array(out)


def sun_table(batch, dark=DARK_ROWS, lit_only=False):
    """Stab (n_btab, n_tab, 3) of the case: ``sun_directions`` on every row, the rows of ``dark`` zeroed. Asserts the 20 deg on
    the inputs"""
    s = sun_directions(batch)
    S = np.ascontiguousarray(np.broadcast_to(s[:, None, :], (batch.Btab.shape[0], batch.n_tab, 3)))
    for i in range(S.shape[0]):
        assert angle_to_rows(s[i], batch.Btab[i, :batch.n_tab]) >= MIN_ANGLE
    if not lit_only:
        for i, (a, b) in dark.items():
            S[i, a:b + 1] = 0.0
    return S


def updates_of(batch, Stab, t, latency):
    """(lit, dark) counts of the sun rows the updates of slew t are made against"""
    n = int(ec.horizons(batch)[t])
    ks = range(1, n - 1) if not latency else range(1, n - 2)          # the knots whose samples are used in an update
    lit = sum(bool(np.any(sun_row(batch, Stab, t, k) != 0.0)) for k in ks)
    return lit, len(ks) - lit


def assert_lit_and_dark(batch, Stab, slews, latency):
    """every compared slew that makes at least six updates has three lit and three dark ones; the short ones are printed"""
    full = 0
    for t in sorted(set(int(s) for s in slews)):
        lit, dark = updates_of(batch, Stab, t, latency)
        if lit + dark >= 6:
            assert lit >= 3 and dark >= 3, (t, lit, dark)
            full += 1
        else:
            print(f"  slew {t} ({int(ec.horizons(batch)[t])} knots) makes {lit + dark} updates: {lit} lit, {dark} dark")
    assert full >= 3


def pairing_table(batch):
    """the case of SUN_PAIRING, at latency 1: rows that alternate lit / dark, so that at one knot row k - 1 is lit and row k dark and
    at the next the other way round. A wrong pairing drops an update or feeds in a sample that never existed (zero)"""
    S = sun_table(batch, lit_only=True)
    S[:, 1::2] = 0.0
    return S


# ---- conditions -----------------------------------------------------------------------------------------------------------------

SUN = "the sun update on against off"
SIGMA_S = "sigma_s against three times it"
NOISE = "sigma_sun against zero"
ECLIPSE = "the eclipse window against none"
SUN_PAIRING = "the delayed sun sample against s_{k-1}, not s_k"
LEFT = ()          # every label shows on the case (the pairing by 2e-5 .. 7e-5); ``pairing_table`` flies it on a case of its own too


def conditions(ref_of, batch, latency, kw, skip=LEFT):
    """on references alone (bar gg_common.MOVED on the final states), each figure printed: the sun update on against off, sigma_s
    against three times itself, sigma_sun against zero, the eclipse window against a table lit throughout and, at latency 1, the row
    the delayed sun sample is paired with. ``skip`` names the labels left to the case that shows them. Returns the reference."""
    ref = ref_of()
    filt = kw["filt"]
    terms = [(SUN, dict(variant=dict(VARIANT, sun=False))), (SIGMA_S, dict(filt=dict(filt, sigma_s=3.0 * filt["sigma_s"]))),
             (NOISE, dict(sigma_sun=0.0)), (ECLIPSE, dict(Stab=sun_table(batch, lit_only=True)))]
    if latency:
        terms.append((SUN_PAIRING, dict(sun_own_row=False)))
    short = []
    for label, over in terms:
        d = moved(ref, ref_of(**over))
        print(f"  condition: {label}: max|d final state| {d:.2e}" + ("  (left to the case that shows it)" if label in skip else ""))
        if label not in skip and not d >= gc.MOVED:
            short.append(f"{label} moves the final state by {d:.2e} only")
    assert not short, short
    return ref


# ---- the calls of both tiers ----------------------------------------------------------------------------------------------------

def filter_options(abi, filt):
    return abi.ModelMagSunFilterOptions(sigma_v=filt["sigma_v"], sigma_w=filt["sigma_w"], sigma_u=filt["sigma_u"], sigma_g=filt["sigma_g"],
                                        sigma_m=filt["sigma_m"], sigma_s=filt["sigma_s"], p0_att=filt["p0_att"], p0_bias=filt["p0_bias"],
                                        reserved=0)


FAMILY = fc.Family(filter_options, FILTER_W, FILT, "model_mag_sun_filtered", "emu_model_mag_sun_filter_check")


def _sun_tail(v, abi):
    return [abi.as_dp(v["Stab"]), C.c_double(v["sigma_sun"])]


class TvCall(fc.TvCall):
    """filtered_common.TvCall of this family followed by the sun table and sigma_sun"""

    def __init__(self, abi, *a, Stab=None, sigma_sun=0.0, **kw):
        super().__init__(abi, *a, family=FAMILY, **kw)
        self.v["Stab"], self.v["sigma_sun"] = sc._dc(Stab), float(sigma_sun)

    def c_args(self, emu=False):
        return super().c_args(emu) + _sun_tail(self.v, self.abi)


class PdCall(fc.PdCall):
    def __init__(self, abi, *a, Stab=None, sigma_sun=0.0, **kw):
        super().__init__(abi, *a, family=FAMILY, **kw)
        self.v["Stab"], self.v["sigma_sun"] = sc._dc(Stab), float(sigma_sun)

    def c_args(self, names=pc.FIELDS):
        return super().c_args(names) + _sun_tail(self.v, self.abi)


class EmuModelMagSunFiltered(fc.EmuFiltered):
    """ctypes binding of tests/emu/libtsat_emu_model_mag_sun_filtered.so, built by the emulator's pattern rule"""

    def __init__(self, abi):
        super().__init__(abi, FAMILY)

    def tv(self, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K, **kw):
        return self._run("tvlqr", TvCall(self.abi, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K=K, **kw), True)

    def pd(self, batch, opts, x0_sim, kd, kp, **kw):
        return self._run("pd", PdCall(self.abi, batch, opts, x0_sim, kd, kp, **kw))

    def check(self, call):
        """check_sun_arguments and check_model_mag_sun_filter of the library on the filter and sun arguments of a call"""
        text = C.create_string_buffer(256)
        v = call.v
        rows = v["n_btab"] * v["o"].n_tab
        rc = self.lib.emu_model_mag_sun_filter_check(None if v["f"] is None else C.byref(v["f"]), self.abi.as_dp(v["Stab"]),
                                                     C.c_double(v["sigma_sun"]), C.c_int64(rows), text, C.c_int32(256))
        return rc, text.value.decode()


def filter_rejections(call):
    """what the entry points reject of the filter and sun arguments, as (label, edited call, words of the text); ``call`` a good
    call with a sun table"""
    abi, f, S = call.abi, call.v["f"], call.v["Stab"]

    def fo(**kw):
        o = abi.ModelMagSunFilterOptions.from_buffer_copy(f)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def bad(idx, val):
        z = S.copy()
        z[idx] = val
        return z

    default = abi.ModelMagSunFilterOptions()
    abi.load().tsat_model_mag_sun_filter_default_options(C.byref(default))
    n = "must be finite and >= 0"
    return [
        ("sigma_v NaN", call.edit(f=fo(sigma_v=float("nan"))), n),
        ("sigma_w negative", call.edit(f=fo(sigma_w=-1e-6)), n),
        ("sigma_u inf", call.edit(f=fo(sigma_u=float("inf"))), n),
        ("sigma_g NaN", call.edit(f=fo(sigma_g=float("nan"))), n),
        ("sigma_m negative", call.edit(f=fo(sigma_m=-1e-9)), n),
        ("sigma_s negative", call.edit(f=fo(sigma_s=-1e-3)), n),
        ("sigma_s NaN", call.edit(f=fo(sigma_s=float("nan"))), n),
        ("p0_att negative", call.edit(f=fo(p0_att=-1.0)), n),
        ("p0_bias NaN", call.edit(f=fo(p0_bias=float("nan"))), n),
        ("sigma_g zero", call.edit(f=fo(sigma_g=0.0)), "sigma_g must be > 0"),
        ("sigma_m zero", call.edit(f=fo(sigma_m=0.0)), "sigma_m must be > 0"),
        ("sigma_s zero with Stab", call.edit(f=fo(sigma_s=0.0)), "sigma_s must be > 0"),
        ("the default options as they are", call.edit(f=default), "sigma_m must be > 0"),
        ("reserved 1", call.edit(f=fo(reserved=1)), "reserved must be 0"),
        ("sigma_sun negative", call.edit(sigma_sun=-1e-3), "sigma_sun must be finite and >= 0"),
        ("sigma_sun NaN", call.edit(sigma_sun=float("nan")), "sigma_sun must be finite and >= 0"),
        ("sigma_sun inf", call.edit(sigma_sun=float("inf")), "sigma_sun must be finite and >= 0"),
        ("Stab NaN", call.edit(Stab=bad((1, 3, 2), np.nan)), "non-finite Stab entry"),
        ("Stab inf", call.edit(Stab=bad((0, 0, 0), np.inf)), "non-finite Stab entry"),
        ("f NULL with Stab", call.edit(f=None, X_hat=None, filt_final=None), "Stab must be NULL"),
        ("Stab NULL with sigma_sun", call.edit(Stab=None), "sigma_sun must be 0"),
        ("Stab NULL, reserved 1", call.edit(Stab=None, sigma_sun=0.0, f=fo(reserved=1)), "reserved must be 0"),
        ("Stab NULL, sigma_m zero", call.edit(Stab=None, sigma_sun=0.0, f=fo(sigma_m=0.0)), "sigma_m must be > 0"),
    ]


def tv_kw(e, M, **over):
    kw = dict(mc.tv_kw(e, M), filt=FILT, Stab=e["Stab"], sigma_sun=SIGMA_SUN)
    kw.update(over)
    return kw


def pd_kw(e, kind, mode, M, **over):
    kw = dict(mc.pd_kw(e, kind, mode, M), filt=FILT, Stab=e["Stab"], sigma_sun=SIGMA_SUN)
    kw.update(over)
    return kw


def parent_kw(kw):
    """the keyword arguments of the model-mag-filtered parent out of this family's"""
    out = {k: v for k, v in kw.items() if k not in ("Stab", "sigma_sun")}
    if out.get("filt") is not None:
        out["filt"] = {k: v for k, v in out["filt"].items() if k != "sigma_s"}
    return out


def ref_of(pkg, ol, e, M, law, pairs, kw, batch=None):
    if law == "tv":
        return pairs_of(ol, pkg._abi, "tv", batch or e["b"], e["x0s"][:, :M], e["K"], e["o"], pairs, X=e["X"], U=e["U"], **kw)
    return pairs_of(ol, pkg._abi, "pd", batch or e["b"], e["x0s"][:, :M], (sc.KD, sc.KP), e["o"], pairs, **kw)


def compare_estimates(ref, got, pairs, idx=None):
    assert got["filt_final"].shape[-1] == FILTER_W
    fc.compare_estimates(ref, got, pairs, idx)


def parity(pkg, ol, run, e, M, law, kw, skip=LEFT, batch=None, pairs=None):
    """``model_mag_filtered_common.parity`` for this family: 34 seeded (t, m) drawn (or ``pairs``), the first 32 off the statistic's
    thresholds compared (``gg_common.kept``: the reference alone has to stay inside N_DRAWN - N_KEPT); the lit / dark counts and the
    conditions are asserted first (``skip`` None: neither). Returns (ref, got, keep)."""
    b = batch or e["b"]
    sampled = pairs is None
    pairs = dc.sampled_pairs(b.T, M) if sampled else pairs
    ref = ref_of(pkg, ol, e, M, law, pairs, kw, batch)
    if sampled:
        keep = gc.kept(ref, e["o"])
    else:
        o = e["o"]
        ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], o.min_steps, o.w_tol, o.angle_tol)
                       > dc.MARGIN for i in range(len(pairs))])
        assert np.count_nonzero(~ok) <= dc.N_DRAWN - dc.N_KEPT, "more than 2 realisations sit on a threshold"
        keep = np.flatnonzero(ok)
    if skip is not None:
        assert_lit_and_dark(b, kw["Stab"], pairs[keep, 0], kw["latency"])
        cp = mc.cond_pairs(dict(e, b=b), ref, pairs, keep)
        conditions(lambda **o: ref_of(pkg, ol, e, M, law, cp, dict(kw, **o), batch), b, kw["latency"], kw, skip=skip)
    got = run(law, e, M, kw, batch)
    dc.compare(ref, got, pairs, keep)
    compare_estimates(ref, got, pairs, keep)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    for t, n in enumerate(b.n_knots):
        assert np.all(got["X_sim"][t, :, n:] == 0) and np.all(got["X_hat"][t, :, n - 1:] == 0)
    ec.same_stats(ref_of(pkg, ol, e, M, law, nomp(b), kw, batch)["stats"], got["nominal"])
    return ref, got, keep


def same_bytes(a, c, keys=("X_sim", "stats", "summary", "nominal", "n_clipped", "X_hat", "filt_final")):
    """difference 0 and equal bytes on every named output"""
    for k in keys:
        if a[k] is None:
            assert c[k] is None, k
            continue
        if a[k].dtype.kind == "f":
            assert float(np.max(np.abs(a[k] - c[k]))) == 0.0, k
        assert a[k].tobytes() == c[k].tobytes(), k


def check_tiny(pkg, ol, run, e, M, b):
    """latency 1 on ``model_mag_filtered_common.tiny_batch`` (n_knots = 2, 3 and 4 among the slews) with a table lit throughout:
    with 2 and 3 knots no update is made and filt_final is ``first_record``; with 4 the first sun update is made at k = 2 — the
    record differs from the parent's reference of the same slew, which makes the magnetometer and gyro updates only"""
    pairs = dc.sampled_pairs(b.T, M)
    S = sun_table(b, lit_only=True)
    for law, kw in (("tv", tv_kw(e, M, latency=1, Stab=S)), ("pd", pd_kw(e, "track_ff", 0, M, latency=1, Stab=S)),
                    ("pd", pd_kw(e, "regulate", 1, M, latency=1, Stab=S))):
        ref = ref_of(pkg, ol, e, M, law, pairs, kw, b)
        tiny = np.flatnonzero(ref["n_knots"] <= 4)
        assert set(ref["n_knots"][tiny]) == {2, 3, 4}, "the sample must hold the three tiny horizons"
        got = run(law, e, M, kw, b)
        none = np.flatnonzero(ref["n_knots"] <= 3)
        big = np.flatnonzero(ref["n_knots"] > 3)
        o = e["o"]
        ok = np.array([ec.margin(ref["X_sim"][i:i + 1], ref["xf"][i:i + 1], ref["n_knots"][i:i + 1], o.min_steps, o.w_tol, o.angle_tol)
                       > dc.MARGIN for i in big])
        assert np.count_nonzero(~ok) <= dc.N_DRAWN - dc.N_KEPT, "more than 2 of the sampled realisations sit on a threshold"
        idx = np.concatenate([none, big[ok]])
        assert np.isin(tiny, idx).all(), "a tiny horizon sits on a threshold"
        dc.compare(ref, got, pairs, idx)
        compare_estimates(ref, got, pairs, idx)
        ec.same_stats(ref_of(pkg, ol, e, M, law, nomp(b), kw, b)["stats"], got["nominal"])
        np.testing.assert_allclose(got["filt_final"][pairs[none, 0], pairs[none, 1]],
                                   np.broadcast_to(first_record(kw["filt"]), (len(none), FILTER_W)), rtol=1e-15, atol=0)
        four = tiny[ref["n_knots"][tiny] == 4]
        par = ref_of(pkg, ol, e, M, law, pairs[four], dict(kw, Stab=None, sigma_sun=0.0), b)
        d = float(np.min(np.max(np.abs(par["filt_final"] - ref["filt_final"][four]), axis=1)))
        print(f"  4-knot slews: the sun update at k = 2 moves filt_final by at least {d:.2e}")
        assert d > 1e-6, "the sun update at k = 2 was not made"


# ---- the long horizon -----------------------------------------------------------------------------------------------------------

LONG_MIN_ANGLE = math.radians(30.0)


def long_case(pkg, ol, N, M, dark_from=100):
    """``model_mag_filtered_common.long_case`` (T = 1, the PD law regulating on the model's plant, 0.38 deg/s gyro noise, 5e-7 T
    magnetometer noise, a gyro bias, latency 0) with a sun sensor of SIGMA_SUN and a sun direction at least 30 deg from the field
    throughout (asserted): the references of this filter lit throughout (``ref``), dark from the row of knot ``dark_from`` on
    (``half``) and the parent's on the same draws (``par``)"""
    c = mc.long_case(pkg, ol, N, M)
    b = c["b"]
    s = sun_directions(b, LONG_MIN_ANGLE)[0]
    assert angle_to_rows(s, b.Btab[0, :b.n_tab]) >= LONG_MIN_ANGLE
    lit = np.ascontiguousarray(np.broadcast_to(s, (1, b.n_tab, 3)))
    dark = lit.copy()
    dark[0, row_index(b, 0, dark_from):] = 0.0
    assert all(np.any(sun_row(b, dark, 0, k) != 0) == (k < dark_from) for k in range(N - 1))
    filt = dict(c["kw"]["filt"], sigma_s=SIGMA_SUN)
    kw = dict(c["kw"], filt=filt, Stab=lit, sigma_sun=SIGMA_SUN)
    args = (ol, pkg._abi, "pd", b, c["x0s"], (sc.KD, sc.KP), c["o"], c["pairs"])
    ref = pairs_of(*args, **kw)
    half = pairs_of(*args, **dict(kw, Stab=dark))
    return dict(c, kw=kw, kw_half=dict(kw, Stab=dark), ref=ref, half=half, par=c["ref"])


def assert_sun_helps(c):
    """on the references alone, rms over the last half of the horizon: lit throughout, the mean attitude error is below the
    model-mag filter's on the same draws; dark from knot 100 on it is above the lit one; the rate bar of the parent's
    ``assert_filter_works`` (0.25 x the raw sample's) still holds. Every figure is printed."""
    N = c["b"].N
    half = slice(N // 2, N - 1)
    lit, dark, par = (gfc.rms_attitude_error(c[k], N) for k in ("ref", "half", "par"))
    deg = np.degrees
    rates = {}
    for name in ("ref", "half"):
        r = c[name]
        we = [np.mean(np.sum((r["X_hat"][i, half, 0:3] - r["X_sim"][i, half, 0:3]) ** 2, axis=1)) for i in range(len(c["pairs"]))]
        wr = [np.mean(np.sum((r["Y_raw"][i, half, 0:3] - r["X_sim"][i, half, 0:3]) ** 2, axis=1)) for i in range(len(c["pairs"]))]
        rates[name] = (math.sqrt(float(np.mean(we))), math.sqrt(float(np.mean(wr))))
    print(f"rms attitude error over the last half, deg: lit throughout {deg(lit).min():.2f} .. {deg(lit).max():.2f} (mean "
          f"{deg(lit).mean():.2f}); dark from knot 100 {deg(dark).min():.2f} .. {deg(dark).max():.2f} (mean {deg(dark).mean():.2f}); the "
          f"model-mag filter {deg(par).min():.2f} .. {deg(par).max():.2f} (mean {deg(par).mean():.2f}); rate error lit "
          f"{rates['ref'][0]:.2e} rad/s, half dark {rates['half'][0]:.2e}, the raw sample's {rates['ref'][1]:.2e}")
    for name in ("ref", "half"):
        assert np.isfinite(c[name]["X_hat"]).all() and np.isfinite(c[name]["filt_final"]).all()
        assert rates[name][0] < 0.25 * rates[name][1], "the filter does not smooth the gyro noise"
    assert lit.mean() < par.mean(), "the sun vector does not improve the attitude estimate"
    assert dark.mean() > lit.mean(), "the eclipse does not show in the attitude estimate"
