"""Field-table and horizon kernels at their edge shapes on the GPU, through magnetic.magnetic_simulation and
horizon.condition_based_time, against the 80-digit transcription (tests/refmath_mp.py). The case table and the assertions
are those of the CPU tier (tests/stage_edges_common.py, tests/test_stage_edges.py). Every test is a handful of launches with
T <= 9 and <= 200 rows; the stale-workspace test makes one 5000-row call on purpose."""
import numpy as np
import pytest

import stage_edges_common as sc

pytestmark = pytest.mark.gpu

FIELD_NAMES = ("edge8", "n1", "n32", "n96")


@pytest.fixture(scope="module")
def solver(pkg):
    s = pkg.trajopt.AugmentedLagrangianSolver(None, None)
    yield s
    s.close()


@pytest.fixture(scope="module")
def oracle_tables(ol):
    return {name: ol.btable_batch(kep, t0, tf, N) for name, (kep, t0, tf, N) in sc.field_calls().items()}


@pytest.fixture(scope="module")
def hz_calls(pkg):
    return sc.horizon_calls(pkg)


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_gpu_field_tables(name, pkg, solver, oracle_tables):
    kep, t0, tf, N = sc.field_calls()[name]
    B, pos = pkg.magnetic.magnetic_simulation(solver, kep, t0, tf, N)
    assert B.shape == (len(kep), 2 * N, 3) and pos.shape == (len(kep), 2 * N + 1, 3)
    sc.field_checks(name, B, pos, *oracle_tables[name], who="GPU")
    B2, none = pkg.magnetic.magnetic_simulation(solver, kep, t0, tf, N, want_pos=False)
    assert none is None and np.array_equal(B, B2)


def test_gpu_field_table_prefix(pkg, solver):
    """(t0, tf, N) and (t0, t0 + 2 (tf - t0), 2N) have the same step: rows 0 .. 2N-2 and positions 0 .. 2N are the same numbers,
    though every row now sits on another lane and pass"""
    kep, t0, tf, N = sc.field_calls()["edge8"]
    B1, p1 = pkg.magnetic.magnetic_simulation(solver, kep, t0, tf, N)
    B2, p2 = pkg.magnetic.magnetic_simulation(solver, kep, t0, t0 + 2 * (tf - t0), 2 * N)
    assert np.array_equal((tf - t0) / N, (t0 + 2 * (tf - t0) - t0) / (2 * N))
    assert np.array_equal(B1[:, :2 * N - 1], B2[:, :2 * N - 1]) and np.array_equal(p1, p2[:, :2 * N + 1])
    assert np.all(B2[:, 2 * N - 1] != 0) and np.all(B2[:, -1] == 0)


@pytest.mark.parametrize("name", sc.HORIZON_CALL_NAMES)
def test_gpu_horizon(name, pkg, solver, hz_calls):
    c = hz_calls[name]
    sc.horizon_checks(c, *pkg.horizon.condition_based_time(solver, c.B, c.dt, c.cut), who="GPU")


def test_gpu_horizon_after_a_larger_call(pkg, hz_calls):
    """a 65-row call on a handle whose workspace still holds a 5000-row call gives what a fresh handle gives"""
    hz, to = pkg.horizon, pkg.trajopt
    c = hz_calls["short_n65"]
    big = np.stack([pkg.slew_setup.dipole_btable(5000, 0.48, 6771.0, 96.6 - 15 * t, 50.0 * t, 70.0 * t) for t in range(6)])
    used, fresh = to.AugmentedLagrangianSolver(None, None), to.AugmentedLagrangianSolver(None, None)
    try:
        idx_big, _ = hz.condition_based_time(used, big, 0.48, 30.0)
        assert np.all(idx_big > 65)
        i1, c1 = hz.condition_based_time(used, c.B, c.dt, c.cut)
        i2, c2 = hz.condition_based_time(fresh, c.B, c.dt, c.cut)
    finally:
        used.close(); fresh.close()
    assert np.array_equal(i1, i2) and np.array_equal(c1, c2)
    sc.horizon_checks(c, i1, c1, who="GPU after a 5000-row call")


def test_gpu_horizon_on_resident_tables(pkg, solver, ol):
    """host=False leaves the tables on the device: same positions, and the horizon read there is the horizon of the downloaded
    table — the B left behind is the B of the plain call"""
    mg, hz = pkg.magnetic, pkg.horizon
    kep, t0, tf, N = sc.field_calls()["edge8"]
    T = len(kep)
    B, pos = mg.magnetic_simulation(solver, kep, t0, tf, N)
    dt = (tf - t0) / N
    call = ol.horizon_batch(B, dt, 1.0, want_all=True)[2]
    # cutoffs early, mid-table and on the last rows of the first pass: cond_at is a function of every row up to the hit. Both
    # calls get the same numbers, so nothing hinges on how close a cutoff is to a condition number.
    cuts = [np.sqrt(call[:, a] * call[:, a + 1]) for a in (5, 40, 63)]
    host = [hz.condition_based_time(solver, B, dt, cut) for cut in cuts]
    none, pos_r = mg.magnetic_simulation(solver, kep, t0, tf, N, host=False)
    assert none is None and np.array_equal(pos_r, pos)
    hits = 0
    for cut, (idx_h, cond_h) in zip(cuts, host):
        idx_r, cond_r = hz.condition_based_time(solver, None, dt, cut, resident_shape=(T, 2 * N))
        assert np.array_equal(idx_r, idx_h) and np.array_equal(cond_r, cond_h)
        hits += np.count_nonzero(idx_h)
    assert hits >= 2 * T
