"""Case tables and 80-digit references shared by tests/test_stage_edges.py (oracle, emulator) and
tests/test_gpu_stage_edges.py (GPU): the field-table kernel (btable_trajectory / igrf12_eval) and the horizon kernel
(horizon_trajectory) at the shapes and inputs where a lane = table-row kernel goes wrong. References: tests/refmath_mp.py,
computed once per process (functools.lru_cache) and never modified."""
import functools

import numpy as np
from mpmath import mp, mpf

import refmath_igrf as ri
import refmath_mp as rmp
from test_magnetic import KEP

MJD, GM, R_IGRF = 58155.0, 3.986004418e5, 6771.0

# ======================================================================================================================
# Field tables
# ======================================================================================================================
# The as-written algorithm computes sin(theta) as sqrt(1 - cos(theta)^2) and divides the east component by sin(theta): closer
# than about 1e-3 rad to a pole (and not exactly on the north pole, which has a branch of its own) its result hinges on how
# far cos(theta) rounds towards +-1, which libm and the device library need not agree on (profiles/stages/
# edge_accuracy.txt). Rows inside that zone carry no assertion; the boundary itself (cases 5, 6) does, so the zone ends a
# rounding error short of 1e-3.
POLAR_ZONE = 1e-3 - 1e-12

N_EDGE = 33                          # 66 rows: one full 64-lane pass and a 2-row tail; 67 positions
FIELD_CASES = [                      # (orbit [e, a, i, RAAN, argp, anomaly], t0, tf)
    (KEP[0], 0.0, 300.0),                                                  # 0 today's workload
    (KEP[1], 5.0, 400.0),                                                  # 1 t0 enters mean anomaly and GMST
    (KEP[2], 12.0, 362.0),                                                 # 2 e = 0.02
    ([0.3, 9000.0, 63.4, 200.0, 270.0, 10.0], 100.0, 1000.0),              # 3 Newton loop at real eccentricity, argp / RAAN
    ([0.0, 6771.0, 90.0, 0.0, 0.0, 90.0], 0.0, 330.0),                     # 4 row 0 exactly on the north pole: theta == 0
    ([0.0, 6771.0, 90.0, 0.0, 0.0, 90.0 - np.degrees(1e-3)], 0.0, 310.0),  # 5 1e-3 rad short of the north pole
    ([0.0, 6771.0, 90.0, 0.0, 0.0, 270.0 + np.degrees(1e-3)], 0.0, 320.0), # 6 1e-3 rad past the south pole (theta near pi)
    ([0.0, 6771.0, 0.0, 0.0, 0.0, 180.0], 30.0, 2830.0),                   # 7 equatorial, a whole revolution: lon wraps
]
# single-orbit calls at the row counts where the `i += WAVE` loop can go wrong: (n_half, orbit, t0, tf)
SHAPE_CASES = [(1, FIELD_CASES[3][0], 100.0, 130.0),      # 2 rows, row 1 zero, 3 positions
               (32, FIELD_CASES[3][0], 100.0, 1060.0),    # exactly 64 rows
               (96, KEP[2], 7.0, 967.0)]                  # exactly 3 passes


def field_calls():
    """name -> (kep (T,6), t0 (T,), tf (T,), n_half)"""
    calls = {"edge8": (np.array([c[0] for c in FIELD_CASES], dtype=np.float64), np.array([c[1] for c in FIELD_CASES]),
                       np.array([c[2] for c in FIELD_CASES]), N_EDGE)}
    for n, kep, t0, tf in SHAPE_CASES:
        calls[f"n{n}"] = (np.array([kep], dtype=np.float64), np.array([t0]), np.array([tf]), n)
    return calls


def _err(a, ref):
    """max |a - ref| of a float64 array against an mpf object array of the same shape, as a float"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=object)
    assert a.shape == ref.shape
    if a.size == 0:
        return 0.0
    if not np.all(np.isfinite(a)):
        return np.inf
    return max(float(abs(mpf(float(x)) - r)) for x, r in zip(a.ravel(), ref.ravel()))


class FieldRef:
    """80-digit tables of one call and, per trajectory, the rows that carry assertions, the scale max|B| and E_ref: the
    worst error of the float64 transcription (refmath_igrf.magnetic_simulation) against them"""

    def __init__(self, kep, t0, tf, N):
        self.N, self.T = N, len(kep)
        self.B, self.pos, self.rows, self.bmax, self.E_B, self.E_pos, self.polar = [], [], [], [], [], [], []
        for t in range(self.T):
            B, pos, lat = rmp.magnetic_simulation(kep[t], t0[t], tf[t], N, MJD, GM, R_IGRF)
            with mp.workdps(rmp.DPS):
                d = np.array([float(min(mp.pi / 2 - x, mp.pi / 2 + x)) for x in lat])
            rows = np.nonzero((d < 1e-20) | (d >= POLAR_ZONE))[0]       # exactly on a pole, or outside the zone
            self.B.append(B); self.pos.append(pos); self.rows.append(rows); self.polar.append(d)
            self.bmax.append(max(float(abs(x)) for x in B.ravel()))
            B64, p64 = ri.magnetic_simulation(kep[t].copy(), t0[t], tf[t], N, MJD, GM, R_IGRF)
            self.E_B.append(self.err_B(t, B64))
            self.E_pos.append(self.err_pos(t, p64))

    def err_B(self, t, B):
        """worst error of table B (2N, 3) of trajectory t on the asserted rows, relative to max|B| of the 80-digit table"""
        r = self.rows[t]
        return _err(np.asarray(B)[r], self.B[t][r]) / self.bmax[t]

    def err_pos(self, t, pos):
        """worst error of the positions (2N+1, 3), km"""
        return _err(pos, self.pos[t])


@functools.lru_cache(maxsize=None)
def field_ref(name):
    return FieldRef(*field_calls()[name])


def field_checks(name, B, pos, Bo, po, who, pos_bar=1e-7):
    """the assertions every implementation (emulator, GPU) meets on one call: 4 E_ref against the 80-digit tables, the parity
    bars against the oracle's (Bo, po), the zero last row. Returns the per-trajectory (err_B, err_pos) it printed."""
    ref = field_ref(name)
    out = []
    for t in range(ref.T):
        eB, eP = ref.err_B(t, B[t]), ref.err_pos(t, pos[t])
        print(f"field {name}[{t}] rows {len(ref.rows[t])}/{2 * ref.N - 1}: E_ref B {ref.E_B[t]:.3e} pos {ref.E_pos[t]:.3e} km | "
              f"{who} B {eB:.3e} pos {eP:.3e} km | oracle B {ref.err_B(t, Bo[t]):.3e} pos {ref.err_pos(t, po[t]):.3e} km")
        out.append((eB, eP))
    for t in range(ref.T):
        eB, eP = out[t]
        # the factor 4: the 104 harmonics are summed in another order and the math library is another one
        assert eB <= 4 * ref.E_B[t], (name, t, eB, ref.E_B[t])
        assert eP <= 4 * ref.E_pos[t], (name, t, eP, ref.E_pos[t])
        r = ref.rows[t]
        assert np.max(np.abs(B[t][r] - Bo[t][r])) < 1e-9 * np.max(np.abs(Bo[t])), (name, t)
        assert np.max(np.abs(pos[t] - po[t])) < pos_bar, (name, t)
        assert np.all(B[t, -1] == 0), (name, t)                         # row 2N-1
    return out


# ======================================================================================================================
# Horizon
# ======================================================================================================================
N_BLOCKS = 200
BLOCK_KS = (2, 63, 64, 65, 127, 128, 129, 199, 200)
SHORT_NS = (1, 2, 63, 64, 65)
# three orbits of the dipole table; every table spans 2400 s. dt_row is an argument of its own (the reference passes the
# table's step; the Gramian does not care), so the three use three weights.
_ORBITS = ((96.6, 40.0, 10.0), (81.0, 200.0, 30.0), (51.6, 300.0, 250.0))
_DTS = (12.0, 9.0, 15.0)
RANK2_CAP = 1e12    # cond[1] is infinite (one slice: rank 2); float64 evaluations of it land anywhere above 1e15


def dipole_table(pkg, n, orbit=0):
    inc, raan, nu = _ORBITS[orbit]
    return pkg.slew_setup.dipole_btable(n, 2400.0 / n, 6771.0, inc, raan, nu)


@functools.lru_cache(maxsize=None)
def _conds_cached(key, dt):
    B = np.frombuffer(key[0], dtype=np.float64).reshape(key[1], 3)
    return tuple(rmp.gramian_conditions(B, dt))


def conds_mp(B, dt):
    """80-digit condition sequence of one table (n, 3), cached on the table's bytes"""
    B = np.ascontiguousarray(B, dtype=np.float64)
    return _conds_cached((B.tobytes(), B.shape[0]), float(dt))


def steer(conds, k, gap=1e-6):
    """cutoff that puts the hit on row k (1-based): the geometric mean of cond[k-1] and cond[k]. Valid only on a strictly
    decreasing sequence whose every value up to k keeps a relative distance `gap` from the cutoff — asserted."""
    hi, lo = conds[k - 2], conds[k - 1]
    if hi == mp.inf:
        hi = mpf(RANK2_CAP)
    cut = float(mp.sqrt(hi * lo))
    for j in range(1, k):
        assert conds[j] < conds[j - 1], ("not strictly decreasing", j)
    assert_gap(conds, k, cut, gap)
    assert rmp.condition_based_time(conds, cut) == k
    return cut


def assert_gap(conds, upto, cut, gap):
    for j in range(upto):
        assert conds[j] == mp.inf or abs(conds[j] / mpf(cut) - 1) >= gap, ("cutoff too close to cond", j, float(conds[j]), cut)


def synthetic_first_hit_table():
    """192 rows whose condition sequence falls, rises by orders of magnitude and falls again, lower than before"""
    rng = np.random.default_rng(41)
    iso = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.standard_normal((n, 3)))
    B = np.concatenate([1e-5 * iso(40), 1e-3 * np.tile([[0.0, 0.0, 1.0]], (60, 1)), 1e-3 * iso(92)])
    return np.ascontiguousarray(B)


SYN_DT = 0.01       # with the first slice unscaled it dominates rows 1..39: their minimum stays above the final value


class HorizonCall:
    def __init__(self, name, B, dt, cut, idx, cond, check_cond):
        self.name = name
        self.B, self.dt, self.cut = np.ascontiguousarray(B), np.asarray(dt, dtype=np.float64), np.asarray(cut, dtype=np.float64)
        self.idx, self.cond, self.check_cond = np.asarray(idx, dtype=np.int32), np.asarray(cond, dtype=np.float64), np.asarray(check_cond)


def _call(name, tables, dts, cuts, gaps=None, index_only=False):
    idx, cond, chk = [], [], []
    for j, (B, dt, cut) in enumerate(zip(tables, dts, cuts)):
        c = conds_mp(B, dt)
        k = rmp.condition_based_time(c, cut)
        assert_gap(c, k if k else len(c), cut, 1e-6 if gaps is None else gaps[j])
        idx.append(k)
        cond.append(float(c[k - 1]) if k else np.inf)
        chk.append(bool(k) and cut <= 1e3 and not index_only)
    return HorizonCall(name, np.stack(tables), dts, cuts, idx, cond, chk)


@functools.lru_cache(maxsize=None)
def horizon_calls(pkg):
    """name -> HorizonCall; every validity condition is asserted while the calls are built"""
    calls = {}
    # block and carry edges: 200 rows, hits on the first / last lanes of every block, per-trajectory cutoff and dt_row arrays
    tabs = [dipole_table(pkg, N_BLOCKS, j % 3) for j in range(len(BLOCK_KS))]
    dts = [_DTS[j % 3] for j in range(len(BLOCK_KS))]
    cuts = [steer(conds_mp(B, dt), k) for B, dt, k in zip(tabs, dts, BLOCK_KS)]
    calls["block_edges"] = c = _call("block_edges", tabs, dts, cuts)
    assert tuple(c.idx) == BLOCK_KS
    # short tables: the hit on the last row (k = n_rows), and a cutoff just under everything the table reaches
    for n in SHORT_NS:
        B = dipole_table(pkg, n, 0)
        cm = conds_mp(B, 2400.0 / n)
        if n == 1:
            cuts, want = [30.0, 1e3], (0, 0)            # a single slice has a rank-2 Gramian
        else:
            cuts, want = [steer(cm, n), 0.99 * float(min(cm))], (n, 0)
        calls[f"short_n{n}"] = c = _call(f"short_n{n}", [B, B], [2400.0 / n] * 2, cuts)
        assert tuple(c.idx) == want
    # never reached: cond >= 1
    tabs = [dipole_table(pkg, N_BLOCKS, j) for j in range(3)]
    calls["never"] = c = _call("never", tabs, list(_DTS), [1.01] * 3)
    assert tuple(c.idx) == (0, 0, 0) and np.all(np.isinf(c.cond))
    # first hit wins on a non-monotone sequence
    S = synthetic_first_hit_table()
    cs = conds_mp(S, SYN_DT)
    m0 = min(cs[:64])                                   # the first minimum: lowest value block 0 reaches
    assert cs[39] < cs[1] / 10 and max(cs[40:100]) > 100 * m0 and min(cs[100:]) < m0 * mpf("0.9")   # falls, rises, falls lower
    cutA, cutB = float(m0) * 1.02, float(m0) * 0.98
    calls["first_hit"] = c = _call("first_hit", [S, S], [SYN_DT] * 2, [cutA, cutB])
    assert 1 <= c.idx[0] <= 64 and min(cs[c.idx[0]:]) < cs[c.idx[0] - 1]     # A: block 0, though a later row is lower
    assert c.idx[1] > 64                                                      # B: not in block 0
    # large cutoff: index only
    B = dipole_table(pkg, N_BLOCKS, 0)
    calls["large_cutoff"] = c = _call("large_cutoff", [B], [1e-4], [1e6], gaps=[1e-4], index_only=True)
    assert c.idx[0] > 2
    return calls


HORIZON_CALL_NAMES = ("block_edges",) + tuple(f"short_n{n}" for n in SHORT_NS) + ("never", "first_hit", "large_cutoff")


def horizon_checks(call, idx, cond, who):
    """tf_index equals the 80-digit index exactly; cond_at within rtol 1e-9 of the 80-digit value for cutoffs <= 1e3 (the
    tolerance the suite uses for this quantity), inf where the cutoff is never reached. Returns the worst relative error."""
    idx, cond = np.asarray(idx), np.asarray(cond)
    rel = np.where(call.check_cond, np.abs(cond / np.where(call.idx > 0, call.cond, 1.0) - 1), 0.0)
    print(f"horizon {call.name}: index {call.idx.tolist()} | {who} index {idx.tolist()} worst cond_at rel err {rel.max():.3e}")
    assert np.array_equal(idx, call.idx), (call.name, list(idx), list(call.idx))
    assert np.all(np.isinf(cond[call.idx == 0])), call.name
    assert np.all(rel <= 1e-9), (call.name, rel)
    return float(rel.max())
