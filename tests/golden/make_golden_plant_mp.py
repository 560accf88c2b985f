#!/usr/bin/env python3
"""Generates tests/golden/plant_mp.npz: inputs of every case of tests/plant_mp_common.py and what tsat_tvlqr_batch computes on
them when no operation rounds — tests/refmath_mp.py::tracking_reference at 50 digits, rounded once to the nearest float64
(K, X_sim, U_sim, the statistic).

Plans are not solved slews (the call tracks whatever it is given): roll-outs by the oracle's RK4 step of random bounded controls
over the dipole tables of slew_setup, so nothing here needs a solve. Table clocks are dyadic (tau0, dtau multiples of 1/4): every
table argument (k + c) dtau + tau0 is then exact in float64 and the row index cannot depend on a rounding; the gain rows, whose
argument carries dt, keep a distance from the integers that is asserted.

The script asserts that no sample of any run lies within MARGIN of w_tol (its rate) or angle_tol (its error angle): index
equality of the statistic is then asserted on every run by the tests, none left out.

    python tests/golden/make_golden_plant_mp.py            write the file
    python tests/golden/make_golden_plant_mp.py --check    regenerate everything and require bit equality with the file
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]
import numpy as np  # noqa: E402

PATH = os.path.join(HERE, "plant_mp.npz")
MARGIN = 1e-7              # the value of tests/dispersed_common.py
ROW_GAP = 1e-6             # distance of a non-integer table argument from the integers
N_TAB = 64
DEG = np.pi / 180.0
SIGMAS = ((0.38 * DEG) ** 2, DEG ** 2, 1e-10)          # sigma_gyro, sigma_att, field_amp of tsat_tvlqr_default_options
SEED = 20190530
J_KINDS = (np.diag([0.00125] * 3), np.diag([0.0011, 0.00125, 0.0016]),
           np.array([[0.00125, 1.2e-4, -0.8e-4], [1.2e-4, 0.0014, 0.6e-4], [-0.8e-4, 0.6e-4, 0.0011]]))
# option vector of a run
O_LIN, O_MIN, O_US, O_WTOL, O_ATOL, O_MODE, O_RAW, O_SEED, O_SG, O_SA, O_FA = range(11)


def tables(ss):
    """three tables of 64 rows: two orbits of the dipole, and the first with rows 0..3 zero (the zero field row)"""
    a = ss.dipole_btable(N_TAB, 12.0, 6771.0, 96.6, 30.0, 40.0)
    b = ss.dipole_btable(N_TAB, 9.0, 6771.0, 51.6, 200.0, 250.0)
    z = a.copy()
    z[:4] = 0.0
    return np.ascontiguousarray(np.stack([a, b, z]))


def _row(Btab, bi, tau0, dtau, k, c):
    v = (k + c) * dtau + tau0                      # exact: dyadic clocks
    i = int(np.floor(v))
    return Btab[bi, min(max(i, 0), N_TAB - 1)]


def _unit(rng):
    v = rng.standard_normal(4)
    return v / np.linalg.norm(v)


def _small_rotation(ss, q, rng, angle):
    v = rng.standard_normal(3)
    v *= angle / np.linalg.norm(v)
    return ss.qmult(q, np.r_[np.cos(angle / 2), v / angle * np.sin(angle / 2)])


def make_batch(ss, ol, Btab, seed, Ns, jkind=0, r=0.5e3, u_max=10.0, goal="end", clocks=None, w0=0.02):
    """inputs of one call: T = len(Ns) plans of Ns[t] knots in slabs of stride max(Ns)"""
    rng = np.random.default_rng(seed)
    T, NS = len(Ns), int(max(Ns))
    J = J_KINDS[jkind]
    d = dict(n_knots=np.array(Ns, dtype=np.int32), X=np.zeros((T, NS, 7)), U=np.zeros((T, NS - 1, 3)), xf=np.zeros((T, 7)),
             btab_idx=np.zeros(T, dtype=np.int32), tau0=np.zeros(T), dtau=np.zeros(T), dt=np.full(T, 0.2),
             Jmat=np.repeat(ss.jmat_cm(J)[None], T, axis=0), x0_sim=np.zeros((T, 7)))
    d["Qd"] = np.tile(np.r_[np.full(3, 10.0), np.full(3, 10.0)], (T, 1))
    d["Qfd"] = 100.0 * d["Qd"]
    d["Rd"] = np.full((T, 3), float(r))
    for t, N in enumerate(Ns):
        bi, tau0, dtau = clocks[t] if clocks else (t % 2, (2.25, -1.5, 40.0, 0.5)[t % 4], (0.75, 0.5, 0.25, 1.0)[t % 4])
        d["btab_idx"][t], d["tau0"][t], d["dtau"][t] = bi, tau0, dtau
        x = np.r_[w0 * rng.standard_normal(3), _unit(rng)]
        for k in range(N - 1):
            u = rng.uniform(-u_max, u_max, 3)
            d["X"][t, k], d["U"][t, k] = x, u
            x = ol.rk_step(4, x, u, _row(Btab, bi, tau0, dtau, k, 0.0), _row(Btab, bi, tau0, dtau, k, 0.5),
                           _row(Btab, bi, tau0, dtau, k, 1.0), 0.2, J)
        d["X"][t, N - 1] = x
        g = goal[t] if isinstance(goal, (list, tuple)) else goal
        d["xf"][t, 3:] = x[3:7] / np.linalg.norm(x[3:7]) if g == "end" else _unit(rng)
        x0 = d["X"][t, 0].copy()
        x0[:3] += 1e-3 * rng.standard_normal(3)
        x0[3:] = _small_rotation(ss, x0[3:], rng, 1e-2)
        d["x0_sim"][t] = x0
    return d


def opts_vec(lin=1, min_steps=10, w_tol=0.05, angle_tol=0.08727, mode=0, raw=0, seed=SEED, scale=1.0):
    return np.array([lin, min_steps, 1e-2, w_tol, angle_tol, mode, raw, seed, SIGMAS[0] * scale, SIGMAS[1] * scale, SIGMAS[2]])


def array_noise(tr, seed, T, NS, scale=1.0):
    """(T, NS-1, 4, 9) values of array mode, a function of `seed` alone that every machine evaluates to the same bits, so the file
    need not hold them: Philox words w under the key (seed, 'nois'), gyro and attitude sigma (w - 2^31) / 2^30 (uniform on
    [-2, 2) sigma: array mode takes whatever it is given), field field_amp w / 2^32 — exact integers and powers of two up to the
    one product"""
    ctr = np.zeros((T, NS - 1, 4, 3, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(T, dtype=np.uint64)[:, None, None, None]
    ctr[..., 1] = np.arange(NS - 1, dtype=np.uint64)[None, :, None, None]
    ctr[..., 2] = np.arange(4, dtype=np.uint64)[None, None, :, None]
    ctr[..., 3] = np.arange(3, dtype=np.uint64)[None, None, None, :]
    w = tr.philox4x32_10(np.array([seed, 0x6E6F6973], dtype=np.uint64), ctr).astype(np.float64).reshape(T, NS - 1, 4, 12)
    sym = (w[..., :6] - 2.0 ** 31) / 2.0 ** 30
    return np.ascontiguousarray(np.concatenate([SIGMAS[0] * scale * sym[..., :3], SIGMAS[1] * scale * sym[..., 3:6],
                                                SIGMAS[2] * (w[..., 6:9] / 2.0 ** 32)], axis=3))


def philox_words(tr, seed, ids, N):
    """(T, N-1, 4, 3, 4) words of noise_mode = 1 (include/tortoise_hip.h), by the integer numpy Philox of the host module: exact"""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    lo = np.uint64(0xFFFFFFFF)
    key = np.array([np.uint64(seed) & lo, np.uint64(seed) >> np.uint64(32)], dtype=np.uint64)
    ctr = np.zeros((len(ids), N - 1, 4, 3, 4), dtype=np.uint64)
    ctr[..., 0] = (ids & lo)[:, None, None, None]
    ctr[..., 1] = (ids >> np.uint64(32))[:, None, None, None]
    ctr[..., 2] = np.arange(N - 1, dtype=np.uint64)[None, :, None, None]
    ctr[..., 3] = (4 * np.arange(4, dtype=np.uint64))[None, None, :, None] + np.arange(3, dtype=np.uint64)[None, None, None, :]
    return tr.philox4x32_10(key, ctr)


def extreme_ids(tr, seed=SEED, n=1 << 16):
    """of the first n ids: the one whose first Box-Muller word (knot 0, stage 0) is smallest, the one where it is largest, and the
    one whose second word is nearest to a multiple of 2^30 (an angle at a quarter turn)"""
    w = philox_words(tr, seed, np.arange(n), 2)[:, 0, 0, 0, :].astype(np.int64)
    off = np.minimum(w[:, 1] % (1 << 30), (1 << 30) - w[:, 1] % (1 << 30))
    return np.array([int(np.argmin(w[:, 0])), int(np.argmax(w[:, 0])), int(np.argmin(off))], dtype=np.int64), w


def build_cases(pkg, ol):
    """-> (Btab, batches: name -> inputs, runs: name -> dict(batch, opts, [noise], [ids]))"""
    ss, tr = pkg.slew_setup, pkg.tracking
    Btab = tables(ss)
    B, R = {}, {}

    def run(name, batch, noise=None, ids=None, **o):
        R[name] = dict(batch=batch, opts=opts_vec(**o))
        if isinstance(noise, int):                            # array_noise(seed): regenerated by whoever reads the file
            R[name]["noise_seed"] = np.array(noise, dtype=np.int64)
            R[name]["noise"] = array_noise(tr, noise, *B[batch]["X"].shape[:2])
        elif noise is not None:                               # edited by hand below: stored (one-step cases)
            R[name]["noise"] = noise
        if ids is not None:
            R[name]["ids"] = np.asarray(ids, dtype=np.int64)

    # ---- uniform batches of the short horizons: two slews a call -----------------------------------------------------
    modes = {1: (("free", 1), ("array", 0), ("gen", 1)), 2: (("free", 0), ("array", 1), ("gen", 0)),
             15: (("gen", 1),), 16: (("gen", 1), ("gen", 0), ("array", 1)), 17: (("gen", 0),),
             31: (("array", 0),), 32: (("array", 1), ("gen", 0)), 33: (("array", 0), ("free", 1))}
    for i, (n1, ms) in enumerate(modes.items()):
        N = n1 + 1
        bn = f"u{n1}"
        B[bn] = make_batch(ss, ol, Btab, 100 + n1, [N, N], jkind=i % 3, r=(0.5e3, 0.05)[i % 2])
        for m, lin in ms:
            nm = f"{bn}_{m}_lin{lin}"
            if m == "free":
                run(nm, bn, lin=lin)
            elif m == "array":
                run(nm, bn, noise=200 + n1, lin=lin)
            else:
                run(nm, bn, ids=[7 + n1, 2 ** 33 + n1], lin=lin, mode=1)
    # ---- ragged batches: a long and a short horizon in one call; every horizon once ----------------------------------
    B["r106"] = make_batch(ss, ol, Btab, 301, [106, 2, 17, 52], jkind=2)
    run("r106_gen_lin1", "r106", ids=[3, 1, 2 ** 35, 0], lin=1, mode=1)
    B["r105"] = make_batch(ss, ol, Btab, 302, [3, 105, 33, 53], jkind=0, r=0.05)
    run("r105_array_lin0", "r105", noise=402, lin=0)
    B["r66"] = make_batch(ss, ol, Btab, 303, [66, 18, 54, 32], jkind=1)
    run("r66_free_lin1", "r66", lin=1)
    B["r65"] = make_batch(ss, ol, Btab, 304, [65, 16, 34], jkind=2, r=0.05)
    run("r65_gen_lin0", "r65", ids=[900, 5, 77], lin=0, mode=1)
    # ---- one step, at the inputs where the step goes wrong ------------------------------------------------------------
    rng = np.random.default_rng(11)
    B["s1"] = make_batch(ss, ol, Btab, 501, [2, 2, 2, 2], jkind=2)
    nz = array_noise(tr, 601, 4, 2)
    nz[0] = 0.0                                               # all nine values zero
    nz[1, :, :, 3:6] = 0.0                                    # the attitude triple zero, the rest not
    nz[2, :, :, 3:6] = 1e-170 * np.array([1.0, -2.0, 0.5])    # squares underflow: th == 0
    nz[3, :, :, 3:6] = 1e-8 * rng.standard_normal((1, 4, 3))
    run("s1_zero_att", "s1", noise=nz, lin=1)
    B["s2"] = make_batch(ss, ol, Btab, 502, [2, 2, 2, 2], jkind=1, goal=["end", "end", "end", "other"])
    nz = array_noise(tr, 602, 4, 2)
    ax = rng.standard_normal((4, 3))
    nz[0, 0, :, 3:6] = (2 * np.pi - 1e-9) * ax / np.linalg.norm(ax, axis=1, keepdims=True)    # th next to a full turn
    B["s2"]["x0_sim"][1, 3:] *= 1e-3                          # quaternion norms far from one
    B["s2"]["x0_sim"][2, 3:] *= 1e3
    if B["s2"]["x0_sim"][3, 3] > 0:                           # a negative scalar part
        B["s2"]["x0_sim"][3, 3:] *= -1.0
    run("s2_turn_norms", "s2", noise=nz, lin=0)
    B["s3"] = make_batch(ss, ol, Btab, 503, [2, 2, 2], jkind=0, clocks=[(0, 2.25, 0.75), (1, 3.0, 0.5), (2, 0.0, 1.0)], u_max=10.0)
    B["s3"]["X"][0, :, :3] = 0.0; B["s3"]["x0_sim"][0, :3] = 0.0          # zero rate, plan and plant
    B["s3"]["U"][1] = 0.0; B["s3"]["x0_sim"][1] = B["s3"]["X"][1, 0]      # zero control: no command, no error to feed back
    nz = array_noise(tr, 603, 3, 2)
    nz[0, :, :, 0:3] = 0.0
    nz[2, :, :, 6:9] = 0.0                                                  # rows 0..1 of table 2 are zero, and stay zero
    run("s3_zero_inputs", "s3", noise=nz, lin=1)
    # ---- the generator at its extreme words -----------------------------------------------------------------------------
    ids, _ = extreme_ids(tr)
    B["gx"] = make_batch(ss, ol, Btab, 504, [3, 3, 3], jkind=1)
    run("gx_extreme_words", "gx", ids=ids, lin=1, mode=1, scale=60.0)
    # ---- the statistic --------------------------------------------------------------------------------------------------
    B["st10"] = make_batch(ss, ol, Btab, 505, [10, 10], jkind=0)            # N <= min_steps: nothing is judged
    run("st10_short", "st10", lin=1, w_tol=10.0, angle_tol=7.0)
    B["st12"] = make_batch(ss, ol, Btab, 507, [12, 12, 12], jkind=2, goal=["end", "other", "end"])
    run("st12_arrivals", "st12", ids=[4, 5, 6], lin=1, mode=1, min_steps=3, w_tol=0.042, angle_tol=0.3)
    run("st12_as_written", "st12", ids=[0, 4000, 0], lin=1, mode=1, min_steps=3, w_tol=0.042, angle_tol=0.3, raw=1)
    return Btab, B, R


def compute_run(tr, Btab, batch, run):
    """the 50-digit results of one run, rounded to float64: dict(K, X_sim, U_sim, slew_index, failed, slew_time, final_w_norm,
    final_angle) in the shapes of the ABI wrappers, and the smallest distances from the thresholds / the integers"""
    import refmath_mp as rmp          # mpmath is needed here alone: the tests that only read the file never import it

    o = run["opts"]
    nk = batch["n_knots"]
    T, NS = len(nk), batch["X"].shape[1]
    out = dict(K=np.zeros((T, NS - 1, 6, 3)), X_sim=np.zeros((T, NS, 7)), U_sim=np.zeros((T, NS - 1, 3)),
               slew_index=np.zeros(T, dtype=np.int32), failed=np.zeros(T, dtype=np.int32), slew_time=np.zeros(T),
               final_w_norm=np.zeros(T), final_angle=np.zeros(T))
    margin, gap = np.inf, np.inf
    words = philox_words(tr, int(o[O_SEED]), run["ids"], NS) if o[O_MODE] == 1 else None
    for t in range(T):
        N = int(nk[t])
        ref = rmp.tracking_reference(
            batch["X"][t, :N], batch["U"][t, :N - 1], batch["xf"][t], Btab[batch["btab_idx"][t]], batch["tau0"][t], batch["dtau"][t],
            batch["dt"][t], batch["Jmat"][t], batch["Qd"][t], batch["Qfd"][t], batch["Rd"][t], batch["x0_sim"][t],
            noise=run["noise"][t, :N - 1] if "noise" in run else None, words=None if words is None else words[t, :N - 1],
            lin_sq=int(o[O_LIN]), u_scale=o[O_US], min_steps=int(o[O_MIN]), w_tol=o[O_WTOL], angle_tol=o[O_ATOL],
            sigmas=(o[O_SG], o[O_SA], o[O_FA]), rate_as_written=int(o[O_RAW]), trial_id=int(run["ids"][t]) if "ids" in run else t)
        f = lambda a: np.array(a, dtype=object).astype(np.float64)          # mpf -> nearest float64
        out["K"][t, :N - 1], out["X_sim"][t, :N], out["U_sim"][t, :N - 1] = f(ref["K"]), f(ref["X_sim"]), f(ref["U_sim"])
        st = ref["stats"]
        out["slew_index"][t], out["failed"][t] = st[0], st[1]
        out["slew_time"][t], out["final_w_norm"][t], out["final_angle"][t] = float(st[2]), float(st[3]), float(st[4])
        with rmp.mp.workdps(rmp.TRACK_DPS):
            margin = min([margin] + [float(abs(w - rmp.mpf(float(o[O_WTOL])))) for w in ref["rates"]]
                         + [float(abs(a - rmp.mpf(float(o[O_ATOL])))) for a in ref["ang"]])
            gap = min(gap, float(ref["gap"]))
    return out, margin, gap


def flatten(Btab, B, R, results):
    d = {"Btab": Btab}
    for bn, b in B.items():
        for k, v in b.items():
            d[f"b/{bn}/{k}"] = v
    for rn, r in R.items():
        d[f"r/{rn}/batch"] = np.array(r["batch"])
        for k in ("opts", "noise_seed", "ids") + (() if "noise_seed" in r else ("noise",)):
            if k in r:
                d[f"r/{rn}/{k}"] = r[k]
        for k, v in results[rn].items():
            d[f"r/{rn}/{k}"] = v
    return d


def generate(pkg, ol, only=None, log=print):
    Btab, B, R = build_cases(pkg, ol)
    results = {}
    for rn, r in R.items():
        if only is not None and rn not in only:
            continue
        t0 = time.time()
        results[rn], margin, gap = compute_run(pkg.tracking, Btab, B[r["batch"]], r)
        log(f"{rn:22s} knots {B[r['batch']]['n_knots'].tolist()} margin {margin:.2e} row gap {gap:.2e} "
            f"index {results[rn]['slew_index'].tolist()} failed {results[rn]['failed'].tolist()}  {time.time() - t0:.1f} s")
        assert margin > MARGIN, (rn, "a sample sits on a threshold: take another seed", margin)
        assert gap > ROW_GAP, (rn, "a table argument sits on an integer", gap)
    return Btab, B, R, results


def expectations(results):
    """what the cases are there for"""
    assert results["st10_short"]["failed"].tolist() == [1, 1] and np.array_equal(results["st10_short"]["slew_time"], [0.2 * 10] * 2)
    a = results["st12_arrivals"]
    assert a["failed"].tolist() == [0, 1, 1] and a["slew_index"][0] > 3, a          # one arrives, two do not
    w = results["st12_as_written"]                                                  # ids 0, 4000 (past the end: the last sample), 0
    assert w["failed"].tolist() == [1, 1, 0], "the two readings of the rate have to differ on slews 0 and 2"
    for rn in ("u1_free_lin1", "u2_gen_lin0"):
        assert np.all(results[rn]["failed"] == 1)


if __name__ == "__main__":
    import oracle_lib as ol
    from tsat_loader import load_package

    pkg = load_package()
    t0 = time.time()
    Btab, B, R, results = generate(pkg, ol)
    expectations(results)
    d = flatten(Btab, B, R, results)
    if "--check" in sys.argv:
        z = np.load(PATH)
        assert sorted(z.files) == sorted(d), "the file and the script hold different arrays"
        for k, v in d.items():
            assert np.asarray(v).tobytes() == z[k].tobytes() and np.asarray(v).shape == z[k].shape, k
        print(f"check: {len(d)} arrays of {len(R)} runs regenerated bit for bit in {time.time() - t0:.0f} s")
    else:
        np.savez_compressed(PATH, **d)
        print(f"{PATH}: {os.path.getsize(PATH)} bytes, {len(R)} runs, {time.time() - t0:.0f} s")
