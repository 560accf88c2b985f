"""Shared pieces of tests/test_every_realisation.py (CPU tier) and tests/test_gpu_every_realisation.py (GPU tier): EVERY REALISATION
of calls that fill more than one wavefront, for every family of ensemble roll-outs that the tiers of its own fly at M = 63 and 64
only (gg, pd, sensed, filtered, model_filtered, mag_filtered, mag_bias_filtered, model_mag_filtered).

The roll-outs run one realisation per lane: wavefront w of slew t flies realisations 64 w .. 64 w + 63, slot M is the noise-free
model, lanes past M duplicate it and store nothing. At M = 64 no realisation with an index >= 64 exists, so everything addressed by
the realisation r — the start, the plant record, the component-major sensor record [T][SNW][Mp] with Mp = 64 waves, the generator id
nid0[t] + r, the X_sim / X_hat / filt_final / stats slabs — has only ever run with r < 64. Here M = 70 (a second wavefront of 6
realisations, the model slot and 57 duplicates) and M = 128 (two full wavefronts, the model slot alone in a third, Mp = 192), and
the comparison is on ``dispersed_common.all_pairs``: every (t, m).

THE CASE is ``pd_common.case(pkg, T=3)``: N = 20, horizons 20 / 13 / 6, all five plant dispersions, ``sensed_common.biases``, plant
noise and gravity gradient on, TVLQR weights r = sensed_common.R_LQR, PD gains sensed_common.KD / KP. The plan comes from the tier
(the oracle on the CPU tier, the library at the 1 x 3 budget on the GPU tier); the gains of the references are the oracle's.

ONE TABLE of families (``FAMILIES``): a row names the family's reference, its emulator binding, its pair of ``tracking`` wrappers and
its filter levels. A family added later costs one row.

THE CONDITIONS are asserted on references alone before anything is compared (``reference_all``): every realisation is off the
thresholds of the statistic (``off_thresholds``), and the second wavefront is distinguishable from the first (``distinguishable``):
the reference of realisation m >= 64 with ONE of its per-realisation inputs — start, plant record, sensor record, generator id —
replaced by that of realisation m - 64 ends >= gg_common.MOVED away, so a kernel that addressed that input by the lane, not by
64 wave + lane, misses the 1e-9 bar."""
import dataclasses

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import filtered_common as fc
import gg_common as gc
import mag_bias_filtered_common as mbc
import mag_filtered_common as gfc
import model_filtered_common as mfc
import model_mag_filtered_common as mmc
import mpc_held_common as hc
import pd_common as pc
import sensed_common as sc

T = 3
MS = (70, 128)
M_MAX = 128
N_COND = 4               # realisations of the second wavefront on which ``distinguishable`` is evaluated, as model_mag_filtered_common.N_COND
MAX_LEFT_OUT = 2         # realisations on a threshold that may leave the comparison of the statistic, of all; none with m >= FIRST_EDGE
FIRST_EDGE = 62
STAT = dict(min_steps=hc.MIN_STEPS, w_tol=hc.W_TOL, angle_tol=hc.ANGLE_TOL)
ID0 = np.arange(T, dtype=np.int64) * 1000 + 2 ** 33          # the explicit generator ids of the prefix tests
KINDS = ("track", "track_ff", "regulate")


class _EmuGg:
    """gg_common.EmuGg behind the argument order of the sensed and filtered bindings"""

    def __init__(self, abi):
        self.emu = gc.EmuGg(abi)

    def tv(self, batch, opts, X, U, Qd, Qfd, Rd, x0_sim, K, plant, Rtab, gm, sat=None, noise_id0=None):
        return self.emu.ensemble(batch, X, U, Qd, Qfd, Rd, x0_sim, K, opts, plant, Rtab, gm, sat, noise_id0)


class _EmuPd:
    def __init__(self, abi):
        self.pd = pc.EmuPd(abi).run


def _gg_pairs(ol, abi, law, batch, x0_sim, K, opts, pairs, X, U, Rtab, gm, **kw):
    return gc.ensemble_pairs(ol, abi, batch, X, U, K, x0_sim, opts, pairs, Rtab, gm, **kw)


def _pd_pairs(ol, abi, law, batch, x0_sim, gains, opts, pairs, **kw):
    return pc.reference_pairs(ol, abi, batch, x0_sim, gains[0], gains[1], opts, pairs, **kw)


@dataclasses.dataclass(frozen=True)
class Row:
    """one family of roll-outs"""
    name: str
    laws: tuple                   # of "tv" and "pd": the laws it has
    ref: object                   # (ol, abi, law, batch, x0_sim, gains, opts, pairs, **kw) -> the dict of ``reference_rollout.pairs_of``
    emu: object                   # abi -> the emulator binding, with ``tv`` and / or ``pd``
    wrappers: tuple               # the names in ``tracking`` of its (TVLQR, PD) wrappers; None where it has no such law
    sensor: bool = False          # whether it takes ``sens``, ``latency`` and ``sensor``
    levels: dict = None           # the filter levels of its parity tests; None: no filter
    options: str = None           # the name in ``tracking`` of the builder of its filter options
    estimates: object = None      # its ``compare_estimates``


def _filtered(name, mod, levels, emu):
    return Row(name, ("tv", "pd"), mod.pairs_of, emu, (f"attitude_ensemble_{name}", f"attitude_ensemble_pd_{name}"), True, levels,
               name.replace("filtered", "filter_options"), mod.compare_estimates)


FAMILIES = (
    Row("gg", ("tv",), _gg_pairs, _EmuGg, ("attitude_ensemble_gg", None)),
    Row("pd", ("pd",), _pd_pairs, _EmuPd, (None, "attitude_ensemble_pd")),
    Row("sensed", ("tv", "pd"), sc.pairs_of, sc.EmuSensed, ("attitude_ensemble_sensed", "attitude_ensemble_pd_sensed"), True),
    _filtered("filtered", fc, fc.FILT, fc.bindings(fc.SIX_STATE)[2]),
    _filtered("model_filtered", mfc, mfc.FILT, fc.bindings(mfc.FAMILY)[2]),
    _filtered("mag_filtered", gfc, gfc.MFILT, fc.bindings(gfc.FAMILY)[2]),
    _filtered("mag_bias_filtered", mbc, mbc.MBFILT, fc.bindings(mbc.FAMILY)[2]),
    _filtered("model_mag_filtered", mmc, mmc.FILT, fc.bindings(mmc.FAMILY)[2]),
)
NAMES = tuple(r.name for r in FAMILIES)
PARITY = tuple((r.name, law) for r in FAMILIES for law in r.laws)          # the calls of the parity tests, one per law a family has


def row(name):
    return FAMILIES[NAMES.index(name)]


# ---- the case -------------------------------------------------------------------------------------------------------------------

def plan_case(pkg, ol, solve):
    """the batch, its orbit table, the plan ``solve(batch)`` -> dict(X, U) and the oracle's gains of it; what does not depend on M"""
    b, Rtab = pc.case(pkg, T=T)
    r = solve(b)
    W = pkg.tracking.tvlqr_weights(b.T, r=sc.R_LQR)
    K = ol.tvlqr_batch(b, r["X"], r["U"], *W, r["X"][:, 0])["K"]
    assert list(b.n_knots) == [20, 13, 6] and b.N == 20
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], W=W, K=K, o=pc.options(ol), x0n=np.ascontiguousarray(b.x0))


def at(pkg, plan, M):
    """the case at M realisations: starts, plants and sensor biases drawn for M"""
    b = plan["b"]
    return dict(plan, M=M, x0s=pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5)), plant=dc.all_five_plants(pkg, b, M),
                sensor=sc.biases(pkg, b.T, M))


def cut(c, M):
    """the first M realisations of a case"""
    return dict(c, M=M, **{k: np.ascontiguousarray(c[k][:, :M]) for k in ("x0s", "plant", "sensor")})


def call_kw(c, fam, law, kind="track_ff", mode=1, latency=0, sat=None, noise_id0=None):
    """the keyword arguments of one call as the family's reference and emulator binding take them (and, ``sens`` spread and ``filt``
    as ``filter``, its wrapper). ``law`` "tv": limits ``sat`` (default pd_common.WIDE); "pd": ``kind`` of KINDS, ``mode`` the
    limit_mode, limits ``sat`` (default mpc_held_common.SAT). A family without a sensor takes no latency."""
    kw = dict(Rtab=c["Rtab"], gm=gc.GM, plant=c["plant"], sat=sat if sat is not None else (pc.WIDE if law == "tv" else hc.SAT))
    if noise_id0 is not None:
        kw["noise_id0"] = noise_id0
    if law == "pd":
        kw.update(X=None if kind == "regulate" else c["X"], U=c["U"] if kind == "track_ff" else None, limit_mode=mode, x0_nom=c["x0n"])
    if fam.sensor:
        kw.update(sens=sc.SIGMAS, latency=latency, sensor=c["sensor"])
    if fam.levels is not None:
        kw["filt"] = fam.levels
    return kw


def parity_kw(c, fam, law):
    """the two calls of the parity tests: TVLQR at latency 1 under +-25; PD track_ff, limit_mode 1, at latency 0 under +-0.6"""
    return call_kw(c, fam, law, latency=1) if law == "tv" else call_kw(c, fam, law, "track_ff", 1, latency=0)


def combinations(fam):
    """every combination the family has of law / kind, limit_mode and latency, as (label, law, the arguments of ``call_kw``)"""
    lat = (0, 1) if fam.sensor else (0,)
    out = [(f"tv, latency {l}", "tv", dict(latency=l, sat=hc.SAT)) for l in lat if "tv" in fam.laws]
    if "pd" in fam.laws:
        out += [(f"{k}, limit_mode {m}, latency {l}", "pd", dict(kind=k, mode=m, latency=l)) for k in KINDS for m in (0, 1) for l in lat]
    return out


# ---- the three ways a call is flown ---------------------------------------------------------------------------------------------

def reference(pkg, ol, c, fam, law, pairs, kw):
    if law == "tv":
        return fam.ref(ol, pkg._abi, "tv", c["b"], c["x0s"], c["K"], c["o"], pairs, X=c["X"], U=c["U"], **kw)
    return fam.ref(ol, pkg._abi, "pd", c["b"], c["x0s"], (sc.KD, sc.KP), c["o"], pairs, **kw)


def emulated(emu, c, law, kw):
    """the emulated kernels of the family whose binding ``emu`` is"""
    if law == "tv":
        return emu.tv(c["b"], c["o"], c["X"], c["U"], *c["W"], c["x0s"], c["K"], **kw)
    return emu.pd(c["b"], c["o"], c["x0s"], sc.KD, sc.KP, **kw)


def library(pkg, solver, c, fam, law, kw):
    """the library through the family's ``tracking`` wrapper, trajectories and estimates asked for"""
    tr, kw = pkg.tracking, dict(kw)
    if fam.sensor:
        kw.update(kw.pop("sens"))
    if fam.levels is not None:
        kw.update(filter=getattr(tr, fam.options)(**kw.pop("filt")), want_estimates=True)
    if law == "tv":
        return getattr(tr, fam.wrappers[0])(solver, c["b"], c["X"], c["U"], c["x0s"], *c["W"], ec.SEED, want_K=True, want_trajectories=True,
                                            **STAT, **kw)
    return getattr(tr, fam.wrappers[1])(solver, c["b"], c["x0s"], sc.KD, sc.KP, ec.SEED, want_trajectories=True, **STAT, **kw)


# ---- the conditions, on references alone ----------------------------------------------------------------------------------------

def off_thresholds(X_sim, xf, n_knots, o):
    """per trajectory: whether it is off the thresholds of the statistic by more than dispersed_common.MARGIN"""
    return np.array([ec.margin(X_sim[i:i + 1], xf[i:i + 1], n_knots[i:i + 1], o.min_steps, o.w_tol, o.angle_tol) > dc.MARGIN
                     for i in range(len(X_sim))])


def _final(ref):
    n = ref["n_knots"]
    return ref["X_sim"][np.arange(len(n)), n - 1]


def _replaced(c, kw, keys, dst, src):
    """the case and the call with the records ``keys`` of realisation (t, dst[i]) replaced by those of (t, src[i])"""
    c2, kw2 = dict(c), dict(kw)
    for k in keys:
        a = c[k].copy()
        a[dst[:, 0], dst[:, 1]] = c[k][src[:, 0], src[:, 1]]
        c2[k] = a
        if k in kw2 and k != "x0s":
            kw2[k] = a
    return c2, kw2


def distinguishable(pkg, ol, c, fam, law, kw, ref, pairs):
    """the second wavefront against the first, on N_COND realisations m >= 64 of the slews of full horizon: each of the start, the
    plant record, the sensor record (where the family has one) and the generator id replaced, one at a time, by that of realisation
    m - 64 moves the final state of the reference of every one of them by >= gg_common.MOVED. Returns {input: the smallest move}."""
    b, M = c["b"], c["M"]
    full = np.flatnonzero(ec.horizons(b) == b.N)
    assert full.size > 0 and M > 64
    ms = np.unique(np.rint(np.linspace(64, M - 1, N_COND)).astype(int))
    ts = full[np.arange(len(ms)) % full.size]
    here = np.stack([ts, ms], axis=1)
    there = np.stack([ts, ms - 64], axis=1)
    assert len(here) == N_COND
    base = _final(ref)[here[:, 0] * M + here[:, 1]]
    assert np.array_equal(pairs[here[:, 0] * M + here[:, 1]], here)
    records = ("x0s", "plant") + (("sensor",) if fam.sensor else ())
    moves = {}
    for label, keys, dst, src, flown in [("start", ("x0s",), here, there, here), ("plant record", ("plant",), here, there, here)] + \
            ([("sensor record", ("sensor",), here, there, here)] if fam.sensor else []) + [("generator id", records, there, here, there)]:
        # the generator id of m - 64 with everything else of m: realisation m - 64 flown with the records of m
        c2, kw2 = _replaced(c, kw, keys, dst, src)
        moves[label] = float(np.min(np.max(np.abs(_final(reference(pkg, ol, c2, fam, law, flown, kw2)) - base), axis=1)))
    print("  condition: the second wavefront is distinguishable: the smallest move of a final state over "
          f"m = {ms.tolist()} with that of m - 64 in its place: " + ", ".join(f"{k} {v:.2e}" for k, v in moves.items()))
    short = [k for k, v in moves.items() if not v >= gc.MOVED]
    assert not short, f"{short} of realisation m - 64 in the place of m's does not show: a kernel that addressed it by the lane would pass"
    return moves


def reference_all(pkg, ol, c, fam, law, kw, label=""):
    """the reference of every realisation of a call, with what ``check_all`` needs beside it — the reference of the noise-free model
    slots (``nominal``), which realisations are off the thresholds (``off``), the family's comparison of the estimates — after the
    two conditions, asserted here on references alone. Returns (ref, pairs)."""
    b, M = c["b"], c["M"]
    pairs = dc.all_pairs(b.T, M)
    ref = reference(pkg, ol, c, fam, law, pairs, kw)
    off = off_thresholds(ref["X_sim"], ref["xf"], ref["n_knots"], c["o"])
    out = pairs[~off]
    print(f"{label}: realisations on a threshold of the statistic: {len(out)} of {len(pairs)}" + (f": (t, m) = {out.tolist()}" if len(out) else "")
          + f"; clipped knots {ref['n_sure'].min()} .. {ref['n_sure'].max()}; arrivals {int(np.count_nonzero(ref['stats']['failed'] == 0))}")
    assert len(out) <= MAX_LEFT_OUT and np.all(out[:, 1] < FIRST_EDGE), "too many realisations, or one at the edge of a wavefront, on a threshold"
    moves = distinguishable(pkg, ol, c, fam, law, kw, ref, pairs)
    nom = reference(pkg, ol, c, fam, law, np.array([(t, -1) for t in range(b.T)]), kw)
    return dict(ref, nominal=nom["stats"], off=off, estimates=fam.estimates, label=label, moves=moves), pairs


# ---- the comparison -------------------------------------------------------------------------------------------------------------

def _worst(a, b, sel):
    return float(np.max(np.abs(a[sel] - b[sel]))) if np.any(sel) else 0.0


def check_all(ref, got, pairs):
    """every (t, m) of a call against its reference (``reference_all``), by the project's bars, unchanged: ``dispersed_common.compare``
    (|dX_sim| < 1e-9, same_stats, n_sure <= n_clipped <= n_maybe), the family's ``compare_estimates`` (1e-9 on X_hat and filt_final)
    where it has estimates, ``summary`` against ``ensemble_common.summary_numpy``, the statistic of the noise-free model slots, zero
    fill beyond each horizon. Realisations on a threshold leave the comparison of the statistic only. Prints and returns the worst
    errors separately for m < 64 and m >= 64."""
    t, m = pairs[:, 0], pairs[:, 1]
    Tn, M = got["stats"].shape
    assert len(pairs) == Tn * M and np.array_equal(pairs, dc.all_pairs(Tn, M)), "every realisation of the call is compared"
    est = ref["estimates"] is not None
    fig = {}
    for name, sel in (("m < 64", m < 64), ("m >= 64", m >= 64)):
        fig[name] = dict(X_sim=_worst(ref["X_sim"], got["X_sim"][t, m], sel))
        if est:
            fig[name].update(X_hat=_worst(ref["X_hat"], got["X_hat"][t, m], sel), filt_final=_worst(ref["filt_final"], got["filt_final"][t, m], sel))
    left = int(np.count_nonzero(~ref["off"]))
    print(f"every realisation: {ref['label']}: " + "; ".join(f"{k}: " + ", ".join(f"max|d{q}| {v:.2e}" for q, v in f.items()) for k, f in fig.items())
          + f"; left out of the statistic: {left} of {len(pairs)}")
    dX = float(np.max(np.abs(ref["X_sim"] - got["X_sim"][t, m])))
    assert dX < 1e-9, dX
    n = got["n_clipped"][t, m]
    assert np.all(ref["n_sure"] <= n) and np.all(n <= ref["n_maybe"])
    dc.compare(ref, got, pairs, np.flatnonzero(ref["off"]))
    if est:
        ref["estimates"](ref, got, pairs)
    np.testing.assert_allclose(got["summary"], ec.summary_numpy(got["stats"]), rtol=1e-12)
    ec.same_stats(ref["nominal"], got["nominal"])
    for s in range(Tn):
        nk = int(ref["n_knots"][s * M])
        assert np.all(got["X_sim"][s, :, nk:] == 0) and np.all(np.abs(got["X_sim"][s, :, :nk, 3:7]).max(axis=2) > 0)
        if est:
            assert np.all(got["X_hat"][s, :, nk - 1:] == 0)
    return dict(fig, left_out=left)


def against_emulator(emu_run, got, o, xf, n_knots, label=""):
    """the library against the emulated kernels of the same source on every realisation: X_sim, X_hat and filt_final to 1e-9 (the
    bar of test_gpu_dispersed_matches_reference_small), ``ensemble_common.same_stats`` on the realisations whose emulated run is off
    the thresholds. Returns the worst error."""
    Tn, M = got["stats"].shape
    worst = {k: float(np.max(np.abs(emu_run[k] - got[k]))) for k in ("X_sim", "X_hat", "filt_final") if emu_run.get(k) is not None}
    tt = np.repeat(np.arange(Tn), M)
    off = off_thresholds(emu_run["X_sim"].reshape(Tn * M, *emu_run["X_sim"].shape[2:]), xf[tt], n_knots[tt], o).reshape(Tn, M)
    print(f"library against emulator: {label}: " + ", ".join(f"max|d{k}| {v:.2e}" for k, v in worst.items())
          + f"; on a threshold {int(np.count_nonzero(~off))} of {Tn * M}")
    assert max(worst.values()) < 1e-9, (label, worst)
    ec.same_stats(emu_run["stats"][off], got["stats"][off])
    return max(worst.values())


def same_prefix(small, large, M, keys):
    """realisations 0 .. M - 1 of ``large`` are ``small``, byte for byte; ``nominal`` is equal"""
    for k in keys:
        assert small[k].tobytes() == np.ascontiguousarray(large[k][:, :M]).tobytes(), (k, M)
    assert small["nominal"].tobytes() == large["nominal"].tobytes(), M
