"""Shared by tests/test_plant_mp.py (CPU tier: oracle, emulator) and tests/test_gpu_plant_mp.py (GPU tier): the cases of
tests/golden/plant_mp.npz — tsat_tvlqr_batch at the loop boundaries of the tracking kernel (gain chunks of 52 knots, forward
chunks of 32, generated-noise chunks of 16), at the inputs where one plant step goes wrong, at the extreme words of the
generator and on the statistic — with what the call computes when no operation rounds (tests/refmath_mp.py::tracking_reference,
50 digits, rounded once to float64; written by tests/golden/make_golden_plant_mp.py), and the assertions every implementation
meets on them. Nothing here imports mpmath: the tests read the file.

The bars, per run, per slew and per quantity (K, X_sim, U_sim):
  * the oracle against the file: |dX_sim| < 1e-9, |dK| < 1e-8 max(1, |K|), |dU_sim| < 1e-8 — the figures of
    tests/test_tracking.py::_same_tracking, here against something that shares no formula with the oracle;
  * E_ref = the oracle's error against the file, measured where the test runs; an implementation (emulator, kernel) is within
    FACTOR max(E_ref, floor) of the file. FACTOR = 4 is the factor of tests/stage_edges_common.py for the same formulas summed in
    another order with another math library; floor = FLOOR_ULPS = 8 units in the last place of the quantity's largest magnitude
    on the slew, per knot travelled, so that an E_ref that happens to be zero on a two-knot slew does not demand bit equality;
  * the implementation against the oracle: _same_tracking, unchanged;
  * slew_index, failed and slew_time equal to the file's on every run (the script asserts that no sample is within 1e-7 of a
    threshold), final_angle and final_w_norm at the tolerances of _same_tracking;
  * every output finite; zero beyond a slew's own horizon.
"""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np

from test_tracking import _same_tracking

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "plant_mp.npz")
FACTOR, FLOOR_ULPS, ULP = 4.0, 8.0, 2.0 ** -52
QUANTITIES = ("K", "X_sim", "U_sim")


@functools.lru_cache(maxsize=None)
def script():
    """tests/golden/make_golden_plant_mp.py as a module (the layout of the option vector, the regenerable noise; the CPU test
    also regenerates the short cases with it)"""
    spec = importlib.util.spec_from_file_location("make_golden_plant_mp", os.path.join(HERE, "golden", "make_golden_plant_mp.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _names():
    with np.load(PATH) as z:
        return tuple(sorted({k.split("/")[1] for k in z.files if k.startswith("r/")}))


RUN_NAMES = _names()


@functools.lru_cache(maxsize=None)
def fixture():
    """(Btab, batches, runs) of the file; never modified"""
    with np.load(PATH) as z:
        B, R = {}, {}
        for k in z.files:
            p = k.split("/")
            if p[0] in ("b", "r"):
                (B if p[0] == "b" else R).setdefault(p[1], {})[p[2]] = z[k]
        return z["Btab"], B, R


def case(pkg, name):
    """-> (SlewBatch, inputs of the batch, run) with the run's array noise regenerated where the file holds only its seed"""
    Btab, B, R = fixture()
    r = dict(R[name])
    b = B[str(r["batch"])]
    if "noise_seed" in r:
        r["noise"] = script().array_noise(pkg.tracking, int(r["noise_seed"]), *b["X"].shape[:2])
    T, NS = b["X"].shape[:2]
    sb = pkg.slew_setup.SlewBatch(N=NS, n_tab=Btab.shape[1], x0=np.ascontiguousarray(b["X"][:, 0]), xf=b["xf"], Btab=Btab, btab_idx=b["btab_idx"],
                                  tau0=b["tau0"], dtau=b["dtau"], dt=b["dt"], Jmat=b["Jmat"], Qd=None, Qfd=None, Rd=None, ulo=None, uhi=None,
                                  U0=None, n_knots=None if np.all(b["n_knots"] == NS) else b["n_knots"])
    return sb, b, r


def fill_options(o, v):
    """the option vector of a run into a tsat_tvlqr_options structure"""
    s = script()
    o.linearize_dt_sq, o.min_steps, o.u_scale, o.w_tol, o.angle_tol = int(v[s.O_LIN]), int(v[s.O_MIN]), v[s.O_US], v[s.O_WTOL], v[s.O_ATOL]
    o.noise_mode, o.rate_as_written, o.noise_seed = int(v[s.O_MODE]), int(v[s.O_RAW]), int(v[s.O_SEED])
    o.sigma_gyro, o.sigma_att, o.field_amp = v[s.O_SG], v[s.O_SA], v[s.O_FA]
    return o


def run_oracle(ol, pkg, name, opts=None, noise="run"):
    sb, b, r = case(pkg, name)
    o = opts if opts is not None else fill_options(ol.tvlqr_default_options(), r["opts"])
    return ol.tvlqr_batch(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], b["x0_sim"], noise=r.get("noise") if isinstance(noise, str) else noise,
                          opts=o, noise_ids=r.get("ids"))


def run_emu(emu, pkg, name, opts=None, noise="run"):
    sb, b, r = case(pkg, name)
    o = opts if opts is not None else fill_options(pkg._abi.TvlqrOptions(), r["opts"])
    return emu.tvlqr(sb, b["X"], b["U"], b["Qd"], b["Qfd"], b["Rd"], b["x0_sim"], noise=r.get("noise") if isinstance(noise, str) else noise,
                     opts=o, noise_ids=r.get("ids"))


def run_gpu(pkg, solver, name, opts=None, noise="run"):
    """tsat_tvlqr_batch through the C ABI with the run's own option block (the Python wrapper does not expose the noise levels)"""
    sb, b, r = case(pkg, name)
    abi, lib = pkg._abi, pkg._abi.load()
    o = opts if opts is not None else fill_options(abi.TvlqrOptions(), r["opts"])
    T, N = sb.T, sb.N
    o.n_knots, o.n_tab = N, sb.n_tab
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    nz = c(r.get("noise") if isinstance(noise, str) else noise)
    ids = None if "ids" not in r else np.ascontiguousarray(r["ids"], dtype=np.int64)
    nk = None if sb.n_knots is None else np.ascontiguousarray(sb.n_knots, dtype=np.int32)
    Xs, Us, K = np.full((T, N, 7), np.nan), np.full((T, N - 1, 3), np.nan), np.full((T, N - 1, 6, 3), np.nan)
    st = np.zeros(T, dtype=abi.TVLQR_STATS_DTYPE)
    d = abi.as_dp
    rc = lib.tsat_tvlqr_batch(solver._h, C.byref(o), T, sb.Btab.shape[0], d(c(b["X"])), d(c(b["U"])), d(c(sb.xf)), d(c(sb.Btab)), abi.as_ip(sb.btab_idx),
                              d(c(sb.tau0)), d(c(sb.dtau)), d(c(sb.dt)), d(c(sb.Jmat)), d(c(b["Qd"])), d(c(b["Qfd"])), d(c(b["Rd"])), d(c(b["x0_sim"])),
                              d(nz), d(Xs), d(Us), d(K), st.ctypes.data_as(C.c_void_p), abi.as_ip(nk),
                              None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)))
    solver._check(rc, "tsat_tvlqr_batch")
    return dict(X_sim=Xs, U_sim=Us, K=K, stats=st)


def errors(name, got):
    """per slew and quantity: (worst absolute error against the file, floor of the bar)"""
    _, B, R = fixture()
    r = R[name]
    nk = B[str(r["batch"])]["n_knots"]
    out = []
    for t, n in enumerate(nk):
        row = {}
        for q in QUANTITIES:
            m = n if q == "X_sim" else n - 1
            ref, g = r[q][t, :m], got[q][t, :m]
            e = float(np.max(np.abs(g - ref))) if np.all(np.isfinite(g)) else np.inf
            row[q] = (e, FLOOR_ULPS * ULP * float(np.max(np.abs(ref))) * (n - 1))
        out.append(row)
    return out


def all_finite(got):
    st = got["stats"]
    return all(np.all(np.isfinite(got[q])) for q in QUANTITIES) and all(np.all(np.isfinite(st[f])) for f in ("slew_time", "final_w_norm", "final_angle"))


def check_stats(name, got, who):
    _, B, R = fixture()
    r, st = R[name], got["stats"]
    assert np.array_equal(st["slew_index"], r["slew_index"]), (name, who, st["slew_index"], r["slew_index"])
    assert np.array_equal(st["failed"], r["failed"]), (name, who)
    assert np.array_equal(st["slew_time"], r["slew_time"]), (name, who, st["slew_time"], r["slew_time"])
    np.testing.assert_allclose(st["final_angle"], r["final_angle"], rtol=1e-6, atol=1e-9, err_msg=f"{name} {who}")
    np.testing.assert_allclose(st["final_w_norm"], r["final_w_norm"], rtol=1e-6, atol=1e-12, err_msg=f"{name} {who}")


def check_zero_fill(name, got, who):
    _, B, R = fixture()
    for t, n in enumerate(B[str(R[name]["batch"])]["n_knots"]):
        assert np.all(got["X_sim"][t, n:] == 0) and np.all(got["U_sim"][t, n - 1:] == 0) and np.all(got["K"][t, n - 1:] == 0), (name, who, t)


def check_oracle(name, ora):
    """the oracle against the file. Returns its errors: E_ref."""
    assert all_finite(ora), (name, "oracle: non-finite output")
    E = errors(name, ora)
    _, B, R = fixture()
    for t, row in enumerate(E):
        kscale = max(float(np.max(np.abs(R[name]["K"][t]))), 1.0)
        assert row["X_sim"][0] < 1e-9 and row["K"][0] < 1e-8 * kscale and row["U_sim"][0] < 1e-8, (name, t, row)
    check_stats(name, ora, "oracle")
    check_zero_fill(name, ora, "oracle")
    return E


def check_impl(name, got, oracles, who):
    """an implementation against the file, with E_ref the larger error of the given oracle builds; prints the table row"""
    finite = all_finite(got)
    E = errors(name, got)
    Eo = [errors(name, o) for o in oracles]
    lines, worst = [], 0.0
    for t, row in enumerate(E):
        for q in QUANTITIES:
            e_ref = max(eo[t][q][0] for eo in Eo)
            bar = FACTOR * max(e_ref, row[q][1])
            part = 0.0 if row[q][0] == 0 else row[q][0] / bar if bar > 0 else np.inf     # an all-zero quantity: the bar is zero too
            worst = max(worst, part)
            lines.append(f"plant_mp {name}[{t}] {q:5s}: E_ref {' / '.join(f'{eo[t][q][0]:.2e}' for eo in Eo)} floor {row[q][1]:.2e} | {who} {row[q][0]:.2e} "
                         f"bar {bar:.2e} ({part:.2f} of it)")
    print("\n".join(lines))
    assert finite, (name, who, "non-finite output")
    for t, row in enumerate(E):
        for q in QUANTITIES:
            e_ref = max(eo[t][q][0] for eo in Eo)
            assert row[q][0] <= FACTOR * max(e_ref, row[q][1]), (name, who, t, q, row[q], e_ref)
    _same_tracking(oracles[0], got)
    check_stats(name, got, who)
    check_zero_fill(name, got, who)
    return worst


# ======================================================================================================================
# Zero noise levels (a property: no 50-digit reference)
# ======================================================================================================================
ZERO_RUN = "u16_gen_lin1"          # two slews of 17 knots


def x_floor(X_ref, n_knots):
    """the floor of the bar above on X_sim: 8 ulp of the largest magnitude per knot travelled"""
    return FLOOR_ULPS * ULP * float(np.max(np.abs(X_ref))) * (int(np.max(n_knots)) - 1)


def check_zero_sigmas(free, zero, n_knots, who):
    """noise_mode = 1 with every level zero against the noise-free run: finite, same verdicts, X_sim equal to rounding (the noisy
    path normalises the quaternion once more: no bit equality)"""
    Xf, Xz = np.asarray(free["X_sim"]), np.asarray(zero["X_sim"])
    assert np.all(np.isfinite(Xz)), (who, "zero noise levels give non-finite states")
    for f in ("slew_time", "final_w_norm", "final_angle"):
        assert np.all(np.isfinite(zero["stats"][f])), (who, f)
    d, bar = float(np.max(np.abs(Xf - Xz))), x_floor(Xf, n_knots)
    print(f"zero sigmas {who}: |dX_sim| {d:.2e}, bar {bar:.2e}")
    assert np.array_equal(free["stats"]["slew_index"], zero["stats"]["slew_index"]) and np.array_equal(free["stats"]["failed"], zero["stats"]["failed"]), who
    assert d <= bar, (who, d, bar)


def tvlqr_zero_sigma_checks(pkg, make_opts, run, who):
    """tsat_tvlqr_batch: all three levels zero = the noise-free run; sigma_att = 0 alone = array mode fed the same draws"""
    sb, b, r = case(pkg, ZERO_RUN)
    v = np.array(r["opts"])
    s = script()
    v0 = v.copy(); v0[s.O_MODE] = 0
    free = run(ZERO_RUN, fill_options(make_opts(), v0), None)
    vz = v.copy(); vz[[s.O_SG, s.O_SA, s.O_FA]] = 0.0
    check_zero_sigmas(free, run(ZERO_RUN, fill_options(make_opts(), vz), None), b["n_knots"], who)
    va = v.copy(); va[s.O_SA] = 0.0
    gen = run(ZERO_RUN, fill_options(make_opts(), va), None)
    nz = pkg.tracking.generated_noise(int(v[s.O_SEED]), r["ids"], sb.N, sigma_gyro=v[s.O_SG], sigma_att=0.0, field_amp=v[s.O_FA])
    assert np.all(nz[..., 3:6] == 0) and np.any(nz[..., :3] != 0)
    arr = run(ZERO_RUN, fill_options(make_opts(), v0), nz)
    assert np.all(np.isfinite(gen["X_sim"])) and np.all(np.isfinite(arr["X_sim"])), (who, "sigma_att = 0 gives non-finite states")
    d = float(np.max(np.abs(gen["X_sim"] - arr["X_sim"])))
    print(f"sigma_att = 0 {who}: seeded against array |dX_sim| {d:.2e}")
    assert d < 1e-12 and np.array_equal(gen["stats"]["slew_index"], arr["stats"]["slew_index"]), (who, d)
    assert np.max(np.abs(gen["X_sim"] - free["X_sim"])) > 1e-9          # the gyro and field draws are still there


# ---- the ensemble entry points and the loops ---------------------------------------------------------------------------
TINY_ATT = 1e-150     # a level of attitude noise whose draws square without underflow (th != 0) and rotate by nothing a float64 sees
ENSEMBLES = ("ensemble", "dispersed", "gg", "sensed", "filtered", "model_filtered")


def ensemble_case(pkg):
    """the 17-knot batch of ZERO_RUN with M = 3 initial states per slew, dispersed plants, an orbit table and the file's gains"""
    import dispersed_common as dc

    sb, b, r = case(pkg, ZERO_RUN)
    x0 = np.ascontiguousarray(np.stack([b["x0_sim"], b["X"][:, 0], 0.5 * (b["x0_sim"] + b["X"][:, 0])], axis=1))
    ss = pkg.slew_setup
    Rtab = np.ascontiguousarray(np.stack([ss.circular_orbit_rows(sb.n_tab, 12.0, 6771.0, 96.6, ra, nu) for ra, nu in ((30.0, 40.0), (200.0, 250.0), (0.0, 0.0))]))
    return dict(sb=sb, b=b, r=r, x0=x0, Rtab=Rtab, plant=dc.all_five_plants(pkg, sb, 3), K=fixture()[2][ZERO_RUN]["K"])


def level_options(make_opts, r, sigma_att=0.0):
    """the run's options in generator mode with no gyro and no field noise and the given attitude level"""
    s = script()
    v = np.array(r["opts"])
    v[s.O_MODE], v[s.O_SG], v[s.O_SA], v[s.O_FA] = 1, 0.0, sigma_att, 0.0
    return fill_options(make_opts(), v)


def gpu_ensemble(pkg, solver, entry, c, o, sens=None):
    """one of the six TVLQR ensemble entry points through the C ABI with the option block `o` (the wrappers of tracking.py take no
    field_amp), on the arguments tracking._ensemble_call marshals. Returns dict(X_sim (T, M, N, 7), stats (T, M))."""
    tr, abi = pkg.tracking, pkg._abi
    sb, b = c["sb"], c["b"]
    lib, head, tail, out = tr._ensemble_call(solver, sb, b["X"], b["U"], c["x0"], b["Qd"], b["Qfd"], b["Rd"], int(o.noise_seed), None, 1.0, False, True,
                                             bool(o.linearize_dt_sq), o.u_scale, o.min_steps, o.w_tol, o.angle_tol)
    o = abi.TvlqrOptions.from_buffer_copy(o)
    o.n_knots, o.n_tab = sb.N, sb.n_tab
    head[1] = C.byref(o)
    T, M = out["stats"].shape
    d = abi.as_dp
    plant = np.ascontiguousarray(c["plant"])
    ncl = np.zeros((T, M), dtype=np.int32)
    args = [*head, d(plant), None, None, *tail, abi.as_ip(ncl)]
    if entry == "ensemble":
        rc = lib.tsat_tvlqr_ensemble(*head, *tail)
    elif entry == "dispersed":
        rc = lib.tsat_tvlqr_ensemble_dispersed(*args)
    else:
        args += [d(c["Rtab"]), float(3.986004418e5)]
        if entry == "gg":
            rc = lib.tsat_tvlqr_ensemble_gg(*args)
        else:
            so, _ = tr._sensing(T, M, None, sens["sigma_gyro"], sens["sigma_att"], sens["sigma_mag"], 0)
            args += [C.byref(so), None]
            if entry == "sensed":
                rc = lib.tsat_tvlqr_ensemble_sensed(*args)
            elif entry == "filtered":
                fo, Xh, ff = tr._filtering(T, M, sb.N, None, False)
                rc = lib.tsat_tvlqr_ensemble_filtered(*args, C.byref(fo), d(Xh), d(ff))
            else:
                fo, Xh, ff = tr._model_filtering(T, M, sb.N, tr.model_filter_options(3e-4, 5e-3, sens["sigma_att"]), False)
                rc = lib.tsat_tvlqr_ensemble_model_filtered(*args, C.byref(fo), d(Xh), d(ff))
    assert rc == 0, (entry, lib.tsat_ensemble_last_error().decode())
    return out


def check_same_limit(zero, tiny, n_knots, who):
    """every level zero against the same call with an attitude level of TINY_ATT — the limit from above, which never took the
    0/0 path: finite, same verdicts, X_sim equal to rounding"""
    check_zero_sigmas(tiny, zero, n_knots, who)
