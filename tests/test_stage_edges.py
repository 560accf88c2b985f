"""Field-table and horizon kernels at their edge shapes, CPU tier: the oracle and the emulated kernel source against the
80-digit transcription (tests/refmath_mp.py). Cases and assertions: tests/stage_edges_common.py; the same table runs on the
GPU in tests/test_gpu_stage_edges.py. Measured figures: profiles/stages/edge_accuracy.txt (tools/edge_accuracy.py)."""
import numpy as np
import pytest
from mpmath import mp

import refmath_igrf as ri
import refmath_mp as rmp
import stage_edges_common as sc

FIELD_NAMES = ("edge8", "n1", "n32", "n96")


@pytest.fixture(scope="module")
def oracle_tables(ol):
    """the oracle's tables of every field call, computed once"""
    return {name: ol.btable_batch(kep, t0, tf, N) for name, (kep, t0, tf, N) in sc.field_calls().items()}


@pytest.fixture(scope="module")
def hz_calls(pkg):
    return sc.horizon_calls(pkg)      # asserts every validity condition while it builds the calls: nothing is skipped


def test_reference_chain_against_float64_transcription():
    """the 80-digit chain and the float64 transcription are the same text: they differ by rounding only. The bound is what
    float64 can do to this chain, not what any implementation gives: the GMST argument is 3.7e5 rad, known to half an ulp
    (3e-11 rad), and rotates a vector of relative size 1 — so a few 1e-11 of max|B|; the positions are ~7e3 km (ulp 9e-13 km)
    through at most 193 Euler steps."""
    with mp.workdps(rmp.DPS):
        b = rmp.igrf12(mp.mpf(2019), mp.mpf(6771e3), mp.mpf(0.7), mp.mpf(-1.1))
    np.testing.assert_allclose([float(x) for x in b], ri.igrf12(2019, 6771e3, 0.7, -1.1), rtol=1e-12, atol=1e-9)
    for name in FIELD_NAMES:
        ref = sc.field_ref(name)
        for t in range(ref.T):
            print(f"field {name}[{t}]: E_ref B {ref.E_B[t]:.3e} of max|B| = {ref.bmax[t]:.3e} T, pos {ref.E_pos[t]:.3e} km")
            assert 0 < ref.E_B[t] < 2.5e-10 and 0 < ref.E_pos[t] < 2.5e-10      # 4 E_ref never exceeds the parity bars


def test_cases_reach_the_edges_they_are_for(ol):
    ref = sc.field_ref("edge8")
    kep, t0, tf, N = sc.field_calls()["edge8"]
    assert len(set(t0)) > 2 and len(set(tf)) == len(tf) and np.count_nonzero(t0) >= 3
    gmst = lambda t: (280.4606 + 360.9856473 * (t / 24 / 60 / 60 + sc.MJD) - 51544.5) / 180 * np.pi
    # case 4: row 0 exactly on the north pole in float64 — theta == 0, the pole branch
    r, _ = ol.kep_eci(kep[4], t0[4], sc.GM)
    pe = ri.Rz(gmst(t0[4])) @ r
    assert np.arcsin(pe[2] / np.linalg.norm(pe)) == np.pi / 2 and np.pi / 2 - np.arcsin(pe[2] / np.linalg.norm(pe)) == 0
    assert ref.polar[4][0] < 1e-20 and np.all(ref.polar[4][1:] > 1e-3)
    # cases 5, 6: row 0 at 1e-3 rad from the north / south pole, inside the asserted rows; no row of any case in the zone
    for t, sign in ((5, 1), (6, -1)):
        assert abs(ref.polar[t][0] - 1e-3) < 1e-12 and ref.rows[t][0] == 0
        assert np.sign(float(ref.pos[t][0][2])) == sign
    for name in FIELD_NAMES:
        rf = sc.field_ref(name)
        assert all(len(rf.rows[t]) == 2 * rf.N - 1 for t in range(rf.T)), name
    # case 7: the longitude goes negative and back along the table
    _, po = ol.btable_batch(kep[7:8], t0[7:8], tf[7:8], N)
    dt = (tf[7] - t0[7]) / N
    lon = np.array([np.arctan2(*(ri.Rz(gmst(t0[7] + dt * i)) @ po[0, i])[1::-1]) for i in range(2 * N - 1)])
    assert np.any(lon < 0) and np.any(lon > 0) and np.any(np.diff(np.sign(lon)) != 0)


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_emulated_field_tables(name, emu, oracle_tables):
    kep, t0, tf, N = sc.field_calls()[name]
    B, pos = emu.btable(kep, t0, tf, N)
    assert B.shape == (len(kep), 2 * N, 3) and pos.shape == (len(kep), 2 * N + 1, 3)
    sc.field_checks(name, B, pos, *oracle_tables[name], who="emulator")


def test_oracle_field_tables_hold_the_same_bar(oracle_tables):
    """the checker itself against 80 digits, at the same 4 E_ref"""
    for name in FIELD_NAMES:
        ref = sc.field_ref(name)
        Bo, po = oracle_tables[name]
        for t in range(ref.T):
            assert ref.err_B(t, Bo[t]) <= 4 * ref.E_B[t] and ref.err_pos(t, po[t]) <= 4 * ref.E_pos[t], (name, t)
            assert np.all(Bo[t, -1] == 0)


def test_emulated_field_table_prefix(emu):
    """(t0, tf, N) and (t0, t0 + 2 (tf - t0), 2N) have the same step: rows 0 .. 2N-2 and positions 0 .. 2N are the same numbers,
    though every row now sits on another lane and pass"""
    kep, t0, tf, N = sc.field_calls()["edge8"]
    B1, p1 = emu.btable(kep, t0, tf, N)
    B2, p2 = emu.btable(kep, t0, t0 + 2 * (tf - t0), 2 * N)
    assert np.array_equal((tf - t0) / N, (t0 + 2 * (tf - t0) - t0) / (2 * N))
    assert np.array_equal(B1[:, :2 * N - 1], B2[:, :2 * N - 1]) and np.array_equal(p1, p2[:, :2 * N + 1])
    assert np.all(B2[:, 2 * N - 1] != 0) and np.all(B2[:, -1] == 0)


@pytest.mark.parametrize("name", sc.HORIZON_CALL_NAMES)
def test_oracle_horizon(name, ol, hz_calls):
    c = hz_calls[name]
    sc.horizon_checks(c, *ol.horizon_batch(c.B, c.dt, c.cut), who="oracle")


@pytest.mark.parametrize("name", sc.HORIZON_CALL_NAMES)
def test_emulated_horizon(name, emu, hz_calls):
    c = hz_calls[name]
    sc.horizon_checks(c, *emu.horizon(c.B, c.dt, c.cut), who="emulator")
