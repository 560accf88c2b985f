"""``magnetic.sun_direction`` and ``magnetic.sun_rows``: the host helpers that make the sun table of the model-mag-sun-filtered
ensembles. The direction against the worked example of Vallado's Algorithm 29 and near the equinoxes; the shadow rule on circular
orbits whose dark fraction is known in closed form."""
import math

import numpy as np
import pytest

MJD_2006_04_02 = 53827.0           # 2 April 2006, 0 h UTC: JD 2453827.5


def _circular(n, a, u, v):
    """n positions of a circular orbit of radius a in the plane of the orthonormal u, v"""
    th = 2.0 * math.pi * (np.arange(n) + 0.5) / n
    return a * (np.cos(th)[:, None] * u + np.sin(th)[:, None] * v)


def test_sun_direction_matches_the_worked_example(pkg):
    """Vallado, Fundamentals of Astrodynamics and Applications, Algorithm 29, worked example: at 2 April 2006 0 h UTC the sun vector
    is 0.9771945, 0.1924424, 0.0834308 AU (mean equator of date). The series gives 0.97719464, 0.1924435, 0.08343122; the bar is
    5e-6 AU per component on the un-normalised vector — the reference prints seven digits and the bar sits about five times above
    the series' truncation seen here (1.1e-6 on y)"""
    mg = pkg.magnetic
    want = np.array([0.9771945, 0.1924424, 0.0834308])
    got = mg.sun_direction(MJD_2006_04_02, au=True)
    d = np.abs(got - want)
    print(f"sun vector {got[0]:.8f} {got[1]:.8f} {got[2]:.8f} AU; |d| per component {d[0]:.1e} {d[1]:.1e} {d[2]:.1e}")
    assert got.shape == (3,) and np.all(d < 5e-6)
    unit = mg.sun_direction(MJD_2006_04_02)
    assert abs(np.linalg.norm(unit) - 1.0) < 1e-15
    np.testing.assert_allclose(unit, got / np.linalg.norm(got), rtol=0, atol=1e-15)
    both = mg.sun_direction(np.array([MJD_2006_04_02, MJD_2006_04_02 + 1.0]))
    assert both.shape == (2, 3) and np.array_equal(both[0], unit)
    step = math.degrees(math.acos(min(1.0, float(both[0] @ both[1])))) / 24.0
    print(f"the direction moves {step:.3f} deg per hour")
    assert 0.035 < step < 0.045


def test_sun_direction_near_the_equinoxes(pkg):
    """within a day of an equinox the vector is within 1 deg of +X (March) or -X (September)"""
    mg = pkg.magnetic
    for mjd, sign in ((53814.77, 1.0), (54001.17, -1.0), (58562.92, 1.0), (58749.33, -1.0)):      # 20 Mar / 23 Sep 2006, 20 Mar / 23 Sep 2019
        for off in (-0.9, 0.0, 0.9):
            s = mg.sun_direction(mjd + off)
            a = math.degrees(math.acos(min(1.0, sign * float(s[0]))))
            assert a < 1.0, (mjd, off, a)


def test_sun_rows_dark_fraction_and_exact_rows(pkg):
    """a circular orbit in the ecliptic plane: the dark fraction is asin(R_E / a) / pi to one row; rows are exactly zero or exactly
    the direction; an orbit whose normal is the sun direction has no dark row; the direction is constant per table"""
    mg = pkg.magnetic
    R_E, a, n = 6371.0, 6771.0, 2000
    mjd = np.array([MJD_2006_04_02, 58155.0])
    s = mg.sun_direction(mjd)
    pole = np.array([0.0, -math.sin(math.radians(23.439291)), math.cos(math.radians(23.439291))])      # the ecliptic pole, to 1e-4
    R = np.empty((2, n, 3))
    for i in range(2):
        u = s[i]
        v = np.cross(pole, u)
        v /= np.linalg.norm(v)
        R[i] = _circular(n, a, u, v)
    S = mg.sun_rows(R, mjd, R_E)
    assert S.shape == R.shape and S.flags.c_contiguous
    for i in range(2):
        dark = ~np.any(S[i] != 0.0, axis=1)
        want = math.asin(R_E / a) / math.pi
        print(f"table {i}: dark rows {int(dark.sum())} of {n}, expected {want * n:.2f}")
        assert abs(int(dark.sum()) - want * n) <= 1.0
        assert np.all(S[i][dark] == 0.0) and np.array_equal(S[i][~dark], np.broadcast_to(s[i], (int((~dark).sum()), 3)))
        assert np.all(R[i][dark] @ s[i] < 0.0)
    assert not np.array_equal(s[0], s[1])
    # a scalar date serves every table
    one = mg.sun_rows(R, MJD_2006_04_02, R_E)
    assert np.array_equal(one[0], S[0]) and np.array_equal(one[1][np.any(one[1] != 0, axis=1)][0], s[0])
    # the orbit normal along the sun: always lit
    u = np.cross(s[0], [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    lit = mg.sun_rows(_circular(n, a, u, np.cross(s[0], u))[None], MJD_2006_04_02, R_E)
    assert np.all(np.any(lit != 0.0, axis=2)) and np.array_equal(lit[0], np.broadcast_to(s[0], (n, 3)))
    # a smaller Earth shades fewer rows; the shadow is behind the Earth only
    assert np.count_nonzero(~np.any(mg.sun_rows(R, mjd, 3000.0) != 0, axis=2)) < np.count_nonzero(~np.any(S != 0, axis=2))


def test_sun_rows_on_orbit_rows_and_rejections(pkg):
    """the table of ``magnetic.orbit_rows`` goes in as it is; shapes and values that make no table are refused"""
    mg = pkg.magnetic
    pos = np.random.default_rng(3).standard_normal((3, 41, 3)) * 7000.0
    R = mg.orbit_rows(pos, 16)
    S = mg.sun_rows(R, [58155.0, 58155.5, 58156.0])
    assert S.shape == (3, 16, 3) and S.dtype == np.float64
    for bad in (dict(Rtab=R[0], mjd=58155.0), dict(Rtab=R[..., :2], mjd=58155.0), dict(Rtab=R, mjd=[58155.0, 58156.0]),
                dict(Rtab=R, mjd=np.zeros((3, 1))), dict(Rtab=R, mjd=float("nan")), dict(Rtab=R, mjd=58155.0, R_E=0.0),
                dict(Rtab=np.where(np.arange(3)[:, None, None] == 1, np.nan, R), mjd=58155.0)):
        with pytest.raises(ValueError):
            mg.sun_rows(**bad)
