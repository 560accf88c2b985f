"""The field-table chain and the Gramian horizon once more, in mpmath at 80 significant digits, and (second half of the file) the
closed-loop tracking of tsat_tvlqr_batch at 50, and (last part) one trajectory of the AL-iLQR solve tsat_solve_batch at 50: what the reference's text
(for the solve: include/tortoise_hip.h and SURVEY.md Appendix A) computes when no operation rounds. Transcribed from the same Julia lines as refmath_igrf.py / refmath.py: kep_ECI
(src/kep_ECI.jl:1-49), OrbitPlotter (src/OrbitPlotter.jl:1-52), magnetic_simulation and magnetic_gramian /
condition_based_time (src/magnetic_toolbox.jl:1-106), igrf12 geocentric (src/igrf.jl:70-274), the Schmidt Legendre
functions (src/legendre.jl:254-292) and their derivatives (src/dlegendre.jl:221-309). Shares no code with oracle/ or the
package; the Gauss coefficients are refmath_igrf's arrays (data). Inputs are the callers' float64 values, converted exactly;
the decimal constants of the text enter as the float64 numbers every implementation parses them to; pi, the trigonometric
functions and every intermediate are mpf.

Two places differ from the text, both because the text is not a function of its mathematical argument there:
  * the degree functions (cosd, sind) are exact at multiples of 90 degrees, as Julia's are;
  * at theta == 0 (and theta == pi) the text switches formula (theta == 0) or divides by sin(pi) (theta == pi). Here the
    field is evaluated at polar distance 1e-25 instead and handed on in ECEF, where it does not depend on the longitude to
    1e-25: no separate pole formula."""
import numpy as np
from mpmath import mp, mpf

import refmath_igrf as ri

DPS = 80
POLE_EPS = "1e-25"


def _f(x):
    return mpf(float(x))           # float64 -> mpf, exact


def _cosd(x):
    return mp.cospi(x / 180)       # exact zeros / ones at multiples of 90 degrees


def _sind(x):
    return mp.sinpi(x / 180)


def _matvec(M, v):
    return [sum(M[i][k] * v[k] for k in range(3)) for i in range(3)]


def _matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _transpose(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _norm(v):
    return mp.sqrt(sum(x * x for x in v))


def legendre_schmidt(phi, n_max):
    # src/legendre.jl:254-292, ph_term = false
    P = [[mpf(0)] * (n_max + 1) for _ in range(n_max + 1)]
    c = mp.cos(phi)
    s = mp.sqrt(1 - c**2)
    P[0][0] = mpf(1)
    P[1][0] = c
    P[1][1] = s
    for n in range(2, n_max + 1):
        for m in range(0, n):
            aux = mpf((n - m) * (n + m))
            a_nm = mp.sqrt(mpf((2 * n - 1) * (2 * n - 1)) / aux)
            b_nm = mp.sqrt(mpf((n + m - 1) * (n - m - 1)) / aux)
            P[n][m] = a_nm * c * P[n - 1][m] - b_nm * P[n - 2][m]
        P[n][n] = s * mp.sqrt(mpf(2 * n - 1) / (2 * n)) * P[n - 1][n - 1]
    return P


def dlegendre_schmidt(phi, P):
    # src/dlegendre.jl:221-309 (the Schmidt variant forwards to it, :384-404), ph_term = false
    rows = len(P)
    dP = [[mpf(0)] * rows for _ in range(rows)]
    Pp = [list(r) + [mpf(0), mpf(0)] for r in P]
    fact = -1 if mp.fmod(phi, 2 * mp.pi) > mp.pi else 1
    for n in range(1, rows):
        for m in range(0, n + 1):
            if m == 0:
                aux = mp.sqrt(mpf(n * (n + 1)) / 2)
                dP[n][0] = -(aux / 2) * Pp[n][1] + (-aux / 2) * Pp[n][1]
            elif m == 1:
                a_nm = mp.sqrt(mpf(2 * n * (n + 1))) / 2
                b_nm = -mp.sqrt(mpf((n + 2) * (n - 1))) / 2
                dP[n][1] = a_nm * Pp[n][0] + b_nm * Pp[n][2]
            elif n != m:
                a_nm = mp.sqrt(mpf((n + m) * (n - m + 1))) / 2
                b_nm = -mp.sqrt(mpf((n + m + 1) * (n - m))) / 2
                dP[n][m] = a_nm * Pp[n][m - 1] + b_nm * Pp[n][m + 1]
            else:
                a_nm = mp.sqrt(mpf((n + m) * (n - m + 1))) / 2
                dP[n][m] = a_nm * Pp[n][m - 1]
            dP[n][m] *= fact
    return dP


def igrf12(date, r, lam, Om):
    """src/igrf.jl:70-274 for 2015 <= date < 2020, away from theta == 0 and theta == pi (see field_ecef). NED, nT."""
    theta = mp.pi / 2 - lam
    phi = Om if Om >= 0 else 2 * mp.pi + Om
    r = r / 1000
    dt = date - 2015
    n_max = 13
    P = legendre_schmidt(theta, n_max)
    dP = dlegendre_schmidt(theta, P)
    a = _f(6371.2)
    sin_p, cos_p = mp.sin(phi), mp.cos(phi)
    ratio = a / r
    fact = ratio
    dVr = dVt = dVp = mpf(0)
    kg = kh = 0
    for n in range(1, n_max + 1):
        aux_r = aux_t = aux_p = mpf(0)
        Gnm = _f(ri.G2015[kg]) + _f(ri.GSV[kg]) * dt
        kg += 1
        aux_r += -(n + 1) / r * Gnm * P[n][0]
        aux_t += Gnm * dP[n][0]
        sin_m1, sin_m2 = mpf(0), -sin_p
        cos_m1, cos_m2 = mpf(1), cos_p
        for m in range(1, n + 1):
            sin_m = 2 * cos_p * sin_m1 - sin_m2
            cos_m = 2 * cos_p * cos_m1 - cos_m2
            Gnm = _f(ri.G2015[kg]) + _f(ri.GSV[kg]) * dt
            Hnm = _f(ri.H2015[kh]) + _f(ri.HSV[kh]) * dt
            kg += 1
            kh += 1
            GcHs = Gnm * cos_m + Hnm * sin_m
            GsHc = Gnm * sin_m - Hnm * cos_m
            aux_r += -(n + 1) / r * GcHs * P[n][m]
            aux_t += GcHs * dP[n][m]
            aux_p += -m * GsHc * P[n][m]
            sin_m2, sin_m1 = sin_m1, sin_m
            cos_m2, cos_m1 = cos_m1, cos_m
        fact *= ratio
        dVr += aux_r * fact
        dVp += aux_p * fact
        dVt += aux_t * fact
    dVr *= a
    dVp *= a
    dVt *= a
    return [1 / r * dVt, -1 / (r * mp.sin(theta)) * dVp, dVr]


def _R_enu_to_xyz(lat, lon):
    # src/magnetic_toolbox.jl:92-95
    return [[-mp.sin(lon), -mp.sin(lat) * mp.cos(lon), mp.cos(lat) * mp.cos(lon)],
            [mp.cos(lon), -mp.sin(lat) * mp.sin(lon), mp.cos(lat) * mp.sin(lon)],
            [mpf(0), mp.cos(lat), mp.sin(lat)]]


def field_ecef(date, r_m, lat, lon):
    """igrf12 / 1e9, NED -> ENU -> ECEF (src/magnetic_toolbox.jl:74-96 without the GMST rotation), Tesla. Within 1e-25 rad
    of a pole the sample is moved to polar distance 1e-25 along its meridian."""
    with mp.workdps(DPS):
        date, r_m, lat, lon = mpf(date), mpf(r_m), mpf(lat), mpf(lon)
        eps = mpf(POLE_EPS)
        if mp.pi / 2 - lat < eps:
            lat = mp.pi / 2 - eps
        elif lat + mp.pi / 2 < eps:
            lat = -mp.pi / 2 + eps
        b = igrf12(date, r_m, lat, lon)
        enu = [b[1] / mpf(10) ** 9, b[0] / mpf(10) ** 9, -b[2] / mpf(10) ** 9]     # NED_to_ENU = [0 1 0; 1 0 0; 0 0 -1]
        return _matvec(_R_enu_to_xyz(lat, lon), enu)


def kep_ECI(kep, t0, GM):
    # src/kep_ECI.jl:1-35 (degrees; element 6 is used as the mean anomaly; the t0 term mixes rad into deg as written)
    A = [_f(x) for x in kep]
    t0, GM = _f(t0), _f(GM)
    A[5] = mp.fmod(A[5] + t0 * mp.sqrt(GM / A[1] ** 3), 360)
    E = A[5] / 180 * mp.pi
    for _ in range(100):
        E = E - (E - A[0] * mp.sin(E) - A[5] / 180 * mp.pi) / (1 - A[0] * mp.cos(E))
    nu = 2 * mp.atan2(mp.sqrt(1 + A[0]) * mp.sin(E / 2), mp.sqrt(1 - A[0]) * mp.cos(E / 2)) * 180 / mp.pi
    r_c = A[1] * (1 - A[0] * mp.cos(E))
    o = [r_c * _cosd(nu), r_c * _sind(nu), mpf(0)]
    k = mp.sqrt(GM * A[1]) / r_c
    o_dot = [k * -mp.sin(E), k * mp.sqrt(1 - A[0] ** 2) * mp.cos(E), mpf(0)]
    Rz = lambda g: [[_cosd(g), _sind(g), mpf(0)], [-_sind(g), _cosd(g), mpf(0)], [mpf(0), mpf(0), mpf(1)]]
    Rx = lambda g: [[mpf(1), mpf(0), mpf(0)], [mpf(0), _cosd(g), _sind(g)], [mpf(0), -_sind(g), _cosd(g)]]
    M = _matmul(_matmul(Rz(-A[3]), Rx(-A[2])), Rz(-A[4]))
    return _matvec(M, o), _matvec(M, o_dot)


def orbit_rhs(x):
    # src/OrbitPlotter.jl:1-48 (only the terms that reach the return value; the J2 term is as written)
    r, v = x[:3], x[3:]
    GM = _f(3.986004418e14) * (mpf(1) / 1000) ** 3
    nr = _norm(r)
    J2 = _f(0.0010826359)
    rho2 = r[0] ** 2 + r[1] ** 2
    f_J2 = [J2 * r[0] / nr**7 * (6 * r[2] - _f(1.5) * rho2),
            J2 * r[1] / nr**7 * (6 * r[2] - _f(1.5) * rho2),
            J2 * r[2] / nr**7 * (3 * r[2] - _f(4.5) * rho2)]
    return list(v) + [GM / nr**2 * -r[i] / nr + f_J2[i] for i in range(3)]


def _Rz(theta):
    # src/magnetic_toolbox.jl:136-140
    c, s = mp.cos(theta), mp.sin(theta)
    return [[c, s, mpf(0)], [-s, c, mpf(0)], [mpf(0), mpf(0), mpf(1)]]


def magnetic_simulation(kep, t0, tf, N, MJD, GM, r_igrf_km, date=2019):
    """src/magnetic_toolbox.jl:33-106. Returns (B (2N, 3), pos (2N+1, 3), lat (2N-1,)) as object arrays of mpf."""
    with mp.workdps(DPS):
        r0, v0 = kep_ECI(kep, t0, GM)
        u = list(r0) + list(v0)
        t0m, tfm = _f(t0), _f(tf)
        dt = (tfm - t0m) / N
        pos = []
        for i in range(2 * N + 1):           # Euler(), adaptive = false, tspan = (t0, 2 tf)
            pos.append(u[:3])
            f = orbit_rhs(u)
            u = [u[j] + dt * f[j] for j in range(6)]
        B = [[mpf(0)] * 3 for _ in range(2 * N)]
        lats = []
        for i in range(2 * N - 1):           # the last row stays zero
            t = t0m + dt * i
            GMST = (_f(280.4606) + _f(360.9856473) * (t / 24 / 60 / 60 + _f(MJD)) - _f(51544.5)) / 180 * mp.pi
            R = _Rz(GMST)
            pe = _matvec(R, pos[i])
            lat = mp.asin(pe[2] / _norm(pe))
            lon = mp.atan2(pe[1], pe[0])
            lats.append(lat)
            B[i] = _matvec(_transpose(R), field_ecef(_f(date), _f(r_igrf_km) * 1000, lat, lon))
        return np.array(B, dtype=object), np.array(pos, dtype=object), np.array(lats, dtype=object)


def _hat_hat_t(b):
    # hat(b) hat(b)' = |b|^2 I - b b'  (src/attitude_controller.jl:172-176)
    n2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    return [[(n2 if i == j else 0) - b[i] * b[j] for j in range(3)] for i in range(3)]


def gramian_conditions(B, dt):
    """magnetic_gramian (src/magnetic_toolbox.jl:1-12) and the 2-norm condition number of every prefix Gramian (:19-22, Julia's
    cond of a symmetric positive semidefinite matrix: largest over smallest eigenvalue). (n_rows,) list of mpf; a Gramian whose
    smallest eigenvalue is zero to the working precision (one slice: rank 2) has condition inf."""
    with mp.workdps(DPS):
        dt = _f(dt)
        conds = []
        G = [[mpf(0)] * 3 for _ in range(3)]
        for i in range(len(B)):
            S = _hat_hat_t([_f(x) for x in B[i]])
            w = mpf(1) if i == 0 else dt                      # the first slice is not scaled (:6)
            G = [[G[r][c] + S[r][c] * w for c in range(3)] for r in range(3)]
            ev = mp.eigsy(mp.matrix(G), eigvals_only=True)
            lo, hi = min(ev), max(ev)
            conds.append(hi / lo if lo > hi * mpf(10) ** (-DPS + 10) else mp.inf)
        return conds


def condition_based_time(conds, cutoff):
    # src/magnetic_toolbox.jl:23-30, 1-based, 0 = never
    cutoff = _f(cutoff)
    for i, c in enumerate(conds):
        if c < cutoff:
            return i + 1
    return 0


# ======================================================================================================================
# Closed-loop tracking (tsat_tvlqr_batch) at 50 digits
# ======================================================================================================================
# attitude_simulation / attitude_lqr (src/attitude_controller.jl:1-145), the plants simulator / gain_simulator
# (src/simulator.jl:1-42, src/gain_simulator.jl:1-53) and the slew-time statistic (src/monte_carlo.jl:242-262), with the
# conventions include/tortoise_hip.h fixes where the text leaves them open: table rows at floor((k + c) dtau + tau0) clamped to
# the table, the draws of noise_mode = 1 from Philox words, th == 0 -> no attitude-noise rotation, rate_as_written. The
# Jacobians are central differences of the RK4 map taken in this arithmetic (step FD_STEP: truncation ~ FD_STEP^2, rounding
# ~ 10^-TRACK_DPS / FD_STEP), so the gains share no derivative formula with the kernel (analytic tangents) or the oracle (dual
# numbers). Everything is per trajectory; inputs are float64 values converted exactly.
TRACK_DPS = 50
FD_STEP = "1e-20"


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _qmult(q1, q2):
    # src/simulator.jl:48-50
    c = _cross(q1[1:], q2[1:])
    return [q1[0] * q2[0] - sum(q1[1 + i] * q2[1 + i] for i in range(3))] + [q1[0] * q2[1 + i] + q2[0] * q1[1 + i] + c[i] for i in range(3)]


def _qrot(q, r):
    # src/simulator.jl:44-46
    c1 = _cross(q[1:], r)
    c2 = _cross(q[1:], [c1[i] + q[0] * r[i] for i in range(3)])
    return [r[i] + 2 * c2[i] for i in range(3)]


def unit_open(w):
    """U(w) = (w + 0.5) 2^-32 of a 32-bit word"""
    return (mpf(int(w)) + mpf(1) / 2) / mpf(2) ** 32


def box_muller(a, b):
    r, th = mp.sqrt(-2 * mp.log(unit_open(a))), 2 * mp.pi * unit_open(b)
    return r * mp.cos(th), r * mp.sin(th)


def plant_draws(words, sg, sa, fa):
    """the nine draws of one plant evaluation from its Philox words w[j][0..3], j = 0, 1, 2 (layout of include/tortoise_hip.h)"""
    w = [[int(x) for x in row] for row in words]
    z0, z1 = box_muller(w[0][0], w[0][1])
    z2, z3 = box_muller(w[0][2], w[0][3])
    z4, z5 = box_muller(w[1][0], w[1][1])
    return [sg * z0, sg * z1, sg * z2, sa * z3, sa * z4, sa * z5, fa * unit_open(w[1][2]), fa * unit_open(w[1][3]), fa * unit_open(w[2][0])]


class TrackingPlant:
    def __init__(self, Jcm, u_scale):
        self.J = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                self.J[r, c] = _f(Jcm[r + 3 * c])
        self.Jinv = self.J ** -1
        self.us = _f(u_scale)

    def f(self, x, u, b, nz=None):
        """simulator (nz: gyro (3), attitude rotation vector (3), field (3)) / gain_simulator (nz None) on the 7-state"""
        w = list(x[:3])
        nq = mp.sqrt(sum(v * v for v in x[3:7]))
        q = [v / nq for v in x[3:7]]
        b = list(b)
        if nz is not None:
            w = [w[i] + nz[i] for i in range(3)]
            th = mp.sqrt(sum(v * v for v in nz[3:6]))
            s = mpf(1) / 2 if th == 0 else mp.sin(th / 2) / th        # r sin(th/2) with r = n / th; no rotation at th == 0
            q = _qmult(q, [mp.cos(th / 2)] + [nz[3 + i] * s for i in range(3)])
            b = [b[i] + nz[6 + i] for i in range(3)]
        qd = _qmult(q, [mpf(0)] + w)
        tau = _cross([v * self.us for v in u], _qrot(q, b))
        Jw = [sum(self.J[r, c] * w[c] for c in range(3)) for r in range(3)]
        wJw = _cross(w, Jw)
        rhs = [tau[i] - wJw[i] for i in range(3)]
        return [sum(self.Jinv[r, c] * rhs[c] for c in range(3)) for r in range(3)] + [qd[i] / 2 for i in range(4)]

    def rk4(self, x, u, rows, h, nz=None):
        """src/attitude_controller.jl:122-132; rows = (b(c = 0), b(1/2), b(1)); nz: four records, one per stage"""
        n = (lambda s: None) if nz is None else (lambda s: nz[s])
        ax = lambda k, a: [x[i] + a * k[i] for i in range(7)]
        k1 = [h * v for v in self.f(x, u, rows[0], n(0))]
        k2 = [h * v for v in self.f(ax(k1, mpf(1) / 2), u, rows[1], n(1))]
        k3 = [h * v for v in self.f(ax(k2, mpf(1) / 2), u, rows[1], n(2))]
        k4 = [h * v for v in self.f(ax(k3, 1), u, rows[2], n(3))]
        return [x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) / 6 for i in range(7)]


def table_row(Bt, k, c, dtau, tau0):
    """row floor((k + c) dtau + tau0) of the table, clamped; also returns the distance of the argument from the nearest integer
    other than itself (a caller that wants index equality with float64 programs checks it)"""
    v = (k + c) * dtau + tau0
    i = int(mp.floor(v))
    frac = v - mp.floor(v)
    i = min(max(i, 0), len(Bt) - 1)
    return [_f(y) for y in Bt[i]], (mpf(1) if frac == 0 else min(frac, 1 - frac))


def _gmat(q):
    # G(q) = [-v'; s I + hat(v)]  (src/attitude_controller.jl:64-71), 4 x 3
    s, v = q[0], q[1:]
    hat = [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]
    return [[-v[0], -v[1], -v[2]]] + [[(s if r == c else 0) + hat[r][c] for c in range(3)] for r in range(3)]


def tracking_gains(plant, X, U, Bt, tau0, dtau, h, lin_sq, Qd, Qfd, Rd):
    """attitude_lqr: K (N-1) matrices 3 x 6. Returns (K, smallest distance of a table argument from an integer)."""
    N = len(X)
    hl = h * h if lin_sq else h
    frac = hl / h
    eps = mpf(FD_STEP)
    A, B, gap = [], [], mpf(1)
    for k in range(N - 1):
        rows = []
        for c in (mpf(0), frac / 2, frac):
            r, g = table_row(Bt, k, c, dtau, tau0)
            rows.append(r); gap = min(gap, g)
        x, u = X[k], U[k]
        Aq, Bq = mp.matrix(7, 7), mp.matrix(7, 3)
        for j in range(7):
            xp, xm = list(x), list(x)
            xp[j] += eps; xm[j] -= eps
            fp, fm = plant.rk4(xp, u, rows, hl), plant.rk4(xm, u, rows, hl)
            for i in range(7):
                Aq[i, j] = (fp[i] - fm[i]) / (2 * eps)
        for j in range(3):
            up, um = list(u), list(u)
            up[j] += eps; um[j] -= eps
            fp, fm = plant.rk4(x, up, rows, hl), plant.rk4(x, um, rows, hl)
            for i in range(7):
                Bq[i, j] = (fp[i] - fm[i]) / (2 * eps)
        Gk, Gn = _gmat(X[k][3:7]), _gmat(X[k + 1][3:7])
        Pn, Pk = mp.matrix(6, 7), mp.matrix(7, 6)
        for i in range(3):
            Pn[i, i] = 1; Pk[i, i] = 1
        for r in range(4):
            for c in range(3):
                Pn[3 + c, 3 + r] = Gn[r][c]
                Pk[3 + r, 3 + c] = Gk[r][c]
        A.append(Pn * Aq * Pk); B.append(Pn * Bq)
    Q, R, S = mp.diag([_f(v) for v in Qd]), mp.diag([_f(v) for v in Rd]), mp.diag([_f(v) for v in Qfd])
    K = [None] * (N - 1)
    for k in range(N - 2, -1, -1):                                   # src/attitude_controller.jl:83-92
        K[k] = (R + B[k].T * S * B[k]) ** -1 * (B[k].T * S * A[k])
        Acl = A[k] - B[k] * K[k]
        S = Q + K[k].T * R * K[k] + Acl.T * S * Acl
    return K, gap


def tracking_reference(X, U, xf, Bt, tau0, dtau, dt, Jcm, Qd, Qfd, Rd, x0_sim, noise=None, words=None, lin_sq=1, u_scale=1e-2,
                       min_steps=10, w_tol=0.05, angle_tol=0.08727, sigmas=None, rate_as_written=0, trial_id=0):
    """One trajectory of tsat_tvlqr_batch over its own N = len(X) knots. noise: (N-1, 4, 9) float64 (array mode), or words:
    (N-1, 4, 3, 4) Philox words with sigmas = (sigma_gyro, sigma_att, field_amp) (generator mode), or neither (noise-free).
    Returns dict of mpf: K (N-1, 6, 3) in the layout of the ABI, X_sim (N, 7), U_sim (N-1, 3), stats (slew_index, failed,
    slew_time, final_w_norm, final_angle), w / ang of every sample, gap (table arguments)."""
    with mp.workdps(TRACK_DPS):
        N = len(X)
        Xm = [[_f(v) for v in row] for row in X]
        Um = [[_f(v) for v in row] for row in U]
        plant = TrackingPlant(Jcm, u_scale)
        h, tau0, dtau = _f(dt), _f(tau0), _f(dtau)
        K, gap = tracking_gains(plant, Xm, Um, Bt, tau0, dtau, h, lin_sq, Qd, Qfd, Rd)
        x = [_f(v) for v in x0_sim]
        Xs, Us = [x], []
        sg = None if sigmas is None else [_f(v) for v in sigmas]
        for k in range(N - 1):
            xr = Xm[k]
            qe = _qmult([xr[3], -xr[4], -xr[5], -xr[6]], x[3:7])
            dX = [x[i] - xr[i] for i in range(3)] + qe[1:]
            u = [Um[k][a] - sum(K[k][a, j] * dX[j] for j in range(6)) for a in range(3)]
            Us.append(u)
            rows = []
            for c in (mpf(0), mpf(1) / 2, mpf(1)):
                r, g = table_row(Bt, k, c, dtau, tau0)
                rows.append(r); gap = min(gap, g)
            if words is not None:
                nz = [plant_draws(words[k][s], *sg) for s in range(4)]
            elif noise is not None:
                nz = [[_f(v) for v in noise[k][s]] for s in range(4)]
            else:
                nz = None
            x = plant.rk4(x, u, rows, h, nz)
            Xs.append(x)
        qf = [_f(v) for v in xf[3:7]]
        qfi = [qf[0], -qf[1], -qf[2], -qf[3]]
        wn = [mp.sqrt(sum(v * v for v in s[:3])) for s in Xs]
        e0 = [_qmult(qfi, s[3:7])[0] for s in Xs]
        assert all(e >= -1 for e in e0), "acos of a value below -1: the statistic is not defined on this case"
        ang = [2 * mp.acos(min(e, mpf(1))) for e in e0]
        ji = min(max(int(trial_id), 0), N - 1)
        first = 0
        for j in range(1, N + 1):
            rate = wn[ji] if rate_as_written else wn[j - 1]
            if j > min_steps and rate < _f(w_tol) and ang[j - 1] < _f(angle_tol):
                first = j
                break
        stats = (first, 0 if first else 1, h * (first if first else N), wn[-1], ang[-1])
        Kabi = [[[K[k][a, j] for a in range(3)] for j in range(6)] for k in range(N - 1)]
        rates = [wn[ji]] * N if rate_as_written else wn
        return dict(K=Kabi, X_sim=Xs, U_sim=Us, stats=stats, rates=rates, ang=ang, gap=gap)


# ======================================================================================================================
# The AL-iLQR solve (tsat_solve_batch, one trajectory) at 50 digits
# ======================================================================================================================
# solve_one of the definition (include/tortoise_hip.h): roll-out, AL cost of the control box and the goal,
# backward sweep, regularisation schedule, backtracking line search, the inner exits, dual and penalty update, final statistics.
# What it shares with neither the kernel (analytic tangents, cofactor inverses, reductions over lanes) nor the oracle (dual
# numbers, scalar loops): the dynamics are TrackingPlant.f above, the Jacobians central differences of the RK map in this
# arithmetic (step FD_STEP), the reductions and the sweep mp.matrix products, Quu^-1 is `** -1`. Every comparison is taken in
# this arithmetic and recorded with its margin: the relative distance of the compared quantity from the value at which the
# decision flips. A float64 program whose quantities are accurate to less than the smallest margin takes the same decisions.
SOLVE_DEFAULTS = dict(integrator=3, max_outer=20, max_inner=50, max_linesearch=20, dj_counter_limit=10, cost_tol=1e-4, grad_tol=1e-5,
                      constraint_tol=1e-3, penalty_init=1.0, penalty_scale=10.0, penalty_max=1e8, dual_max=1e8, reg_init=0.0,
                      reg_scale=1.6, reg_min=1e-8, reg_max=1e8, reg_fp=10.0, ls_lower=1e-8, ls_upper=10.0, max_state=1e8,
                      u_scale=1e-2, terminal_mask=0x7F, error_state=0)
ST_CONVERGED, ST_MAX_OUTER, ST_REG_FAIL, ST_DIVERGED = 0, 1, 2, 3


class Margins:
    """smallest margin of every kind of decision; `exact` counts the decisions that are ties by construction of the input"""

    def __init__(self):
        self.kinds, self.exact = {}, {}

    def add(self, kind, m):
        m = mpf(m)
        if kind not in self.kinds or m < self.kinds[kind]:
            self.kinds[kind] = m

    def tie(self, kind):
        self.exact[kind] = self.exact.get(kind, 0) + 1

    def rel(self, kind, a, b):
        """a compared with b: |a - b| / max(|a|, |b|)"""
        s = max(abs(a), abs(b))
        self.add(kind, mpf(1) if s == 0 else abs(a - b) / s)

    def min(self):
        return min(self.kinds.values()) if self.kinds else mpf(1)


class _Solve:
    def __init__(self, x0, xf, Bt, tau0, dtau, dt, Jcm, Qd, Qfd, Rd, ulo, uhi, o):
        self.o = o
        self.N = None
        self.plant = TrackingPlant(Jcm, o["u_scale"])
        self.x0, self.xf = [_f(v) for v in x0], [_f(v) for v in xf]
        self.Bt, self.tau0, self.dtau, self.h = Bt, _f(tau0), _f(dtau), _f(dt)
        self.Qd, self.Qfd, self.Rd = [_f(v) for v in Qd], [_f(v) for v in Qfd], [_f(v) for v in Rd]
        self.ulo, self.uhi = [_f(v) for v in ulo], [_f(v) for v in uhi]
        self.es, self.mask = int(o["error_state"]), int(o["terminal_mask"])
        self.max_state = _f(o["max_state"])
        self.mg = Margins()
        self.rows_cache = {}

    # ---- dynamics -----------------------------------------------------------------------------------------------------
    def rows(self, k):
        if k not in self.rows_cache:
            r = []
            for c in (mpf(0), mpf(1) / 2, mpf(1)):
                row, gap = table_row(self.Bt, k, c, self.dtau, self.tau0)
                v = (k + c) * self.dtau + self.tau0
                near = int(mp.floor(v + mpf(1) / 2))                   # the integer next to the argument: rows near - 1 and near
                if v == mp.floor(v):
                    self.mg.tie("table_gap")                           # an integer argument: exact in float64 and in fma too
                elif min(max(near - 1, 0), len(self.Bt) - 1) == min(max(near, 0), len(self.Bt) - 1):
                    pass                                               # both sides of that integer are clamped to the same row
                else:
                    self.mg.add("table_gap", gap)
                r.append(row)
            self.rows_cache[k] = r
        return self.rows_cache[k]

    def step(self, k, x, u):
        p, h, rows = self.plant, self.h, self.rows(k)
        if int(self.o["integrator"]) == 4:
            return p.rk4(x, u, rows, h)
        k1 = [h * v for v in p.f(x, u, rows[0])]                       # rk3: src/attitude_controller.jl:178-187
        k2 = [h * v for v in p.f([x[i] + k1[i] / 2 for i in range(7)], u, rows[1])]
        k3 = [h * v for v in p.f([x[i] - k1[i] + 2 * k2[i] for i in range(7)], u, rows[2])]
        return [x[i] + (k1[i] + 4 * k2[i] + k3[i]) / 6 for i in range(7)]

    def jacobians(self, k, x, u):
        eps = mpf(FD_STEP)
        A, B = mp.matrix(7, 7), mp.matrix(7, 3)
        for j in range(7):
            xp, xm = list(x), list(x)
            xp[j] += eps; xm[j] -= eps
            fp, fm = self.step(k, xp, u), self.step(k, xm, u)
            for i in range(7):
                A[i, j] = (fp[i] - fm[i]) / (2 * eps)
        for j in range(3):
            up, um = list(u), list(u)
            up[j] += eps; um[j] -= eps
            fp, fm = self.step(k, x, up), self.step(k, x, um)
            for i in range(7):
                B[i, j] = (fp[i] - fm[i]) / (2 * eps)
        return A, B

    # ---- cost ---------------------------------------------------------------------------------------------------------
    def box(self, u, lam):
        """the six rows (c, lambda, active) of one knot; the margin of c is relative to max(|u|, |bound|)"""
        out = []
        for a in range(3):
            for c, lm, s in ((u[a] - self.uhi[a], lam[a], max(abs(u[a]), abs(self.uhi[a]))),
                             (self.ulo[a] - u[a], lam[3 + a], max(abs(u[a]), abs(self.ulo[a])))):
                if lm > 0:
                    act = True
                else:
                    act = c > 0
                    if c == 0:
                        self.mg.tie("active_set")
                    else:
                        self.mg.add("active_set", abs(c) / s)
                out.append((c, lm, act))
        return out

    def total_cost(self, X, U, al, with_al=True):
        J = mpf(0)
        for k in range(self.N - 1):
            x, u = X[k], U[k]
            J += sum(self.Qd[i] * (x[i] - self.xf[i]) ** 2 for i in range(7)) / 2 + sum(self.Rd[a] * u[a] ** 2 for a in range(3)) / 2
            if with_al:
                for c, lm, act in self.box(u, al["lam"][k]):
                    J += lm * c + (al["mu"] * c * c / 2 if act else 0)
        x = X[self.N - 1]
        J += sum(self.Qfd[i] * (x[i] - self.xf[i]) ** 2 for i in range(7)) / 2
        if with_al:
            for i in range(7):
                if self.mask >> i & 1:
                    e = x[i] - self.xf[i]
                    J += al["nu"][i] * e + al["mu"] * e * e / 2
        return J

    def max_violation(self, X, U):
        c = mpf(0)
        for k in range(self.N - 1):
            for a in range(3):
                c = max(c, U[k][a] - self.uhi[a], self.ulo[a] - U[k][a])
        for i in range(7):
            if self.mask >> i & 1:
                c = max(c, abs(X[self.N - 1][i] - self.xf[i]))
        return c

    # ---- roll-out -----------------------------------------------------------------------------------------------------
    def within(self, v):
        self.mg.rel("max_state", abs(v), self.max_state)
        self.largest = max(self.largest, abs(v))
        return abs(v) <= self.max_state

    def state_diff(self, xn, xb):
        if not self.es:
            return [xn[j] - xb[j] for j in range(7)]
        qe = _qmult([xb[3], -xb[4], -xb[5], -xb[6]], xn[3:7])
        return [xn[j] - xb[j] for j in range(3)] + [qe[1 + j] / (1 + qe[0]) for j in range(3)]

    def rollout(self, X, U, K, d, alpha, closed):
        Xc, Uc, ok = [list(self.x0)], [], True
        self.largest = mpf(0)
        for k in range(self.N - 1):
            xc = Xc[k]
            u = list(U[k])
            if closed:
                dx = self.state_diff(xc, X[k])
                for a in range(3):
                    u[a] += sum(K[k][a, j] * dx[j] for j in range(len(dx))) + alpha * d[k][a]
            Uc.append(u)
            for v in xc + u:
                ok = self.within(v) and ok
            Xc.append(self.step(k, xc, u))
        for v in Xc[self.N - 1]:
            ok = self.within(v) and ok
        return ok, Xc, Uc

    # ---- backward sweep -----------------------------------------------------------------------------------------------
    def emat(self, q):
        E = mp.matrix(7, 6)
        G = _gmat(q)
        for i in range(3):
            E[i, i] = 1
        for r in range(4):
            for c in range(3):
                E[3 + r, 3 + c] = G[r][c]
        return E

    def backward(self, X, U, al, rho):
        N, es, mu = self.N, self.es, al["mu"]
        xN = X[N - 1]
        Sd, sf = [], mp.matrix(7, 1)
        for i in range(7):
            e = xN[i] - self.xf[i]
            m = self.mask >> i & 1
            Sd.append(self.Qfd[i] + (mu if m else 0))
            sf[i] = self.Qfd[i] * e + ((al["nu"][i] + mu * e) if m else 0)
        S, s = mp.diag(Sd), sf
        if es:
            E = self.emat(xN[3:7])
            S, s = E.T * S * E, E.T * s
        Qm = mp.diag(self.Qd)
        K, d = [None] * (N - 1), [None] * (N - 1)
        dV = [mpf(0), mpf(0)]
        for k in range(N - 2, -1, -1):
            x, u = X[k], U[k]
            A, B = self.jacobians(k, x, u)
            lx = mp.matrix([self.Qd[i] * (x[i] - self.xf[i]) for i in range(7)])
            Q0 = Qm
            if es:
                Ek, En = self.emat(x[3:7]), self.emat(X[k + 1][3:7])
                A, B, lx, Q0 = En.T * A * Ek, En.T * B, Ek.T * lx, Ek.T * Qm * Ek
            rows = self.box(u, al["lam"][k])
            lu, luu = mp.matrix(3, 1), [None] * 3
            for a in range(3):
                (cu, lmu, au), (cl, lml, alo) = rows[2 * a], rows[2 * a + 1]
                lu[a] = self.Rd[a] * u[a] + lmu + (mu * cu if au else 0) - lml - (mu * cl if alo else 0)
                luu[a] = self.Rd[a] + (mu if au else 0) + (mu if alo else 0)
            Qx, Qu = lx + A.T * s, lu + B.T * s
            Qxx, Quu, Qux = Q0 + A.T * S * A, mp.diag(luu) + B.T * S * B, B.T * S * A
            Qr = (Quu + Quu.T) / 2 + rho * mp.eye(3)
            q00 = Qr[0, 0]
            t1, t2 = Qr[0, 0] * Qr[1, 1], Qr[1, 0] * Qr[1, 0]
            c22 = t1 - t2
            det = mp.det(Qr)
            c00, c01, c02 = Qr[1, 1] * Qr[2, 2] - Qr[2, 1] ** 2, Qr[2, 0] * Qr[2, 1] - Qr[1, 0] * Qr[2, 2], Qr[1, 0] * Qr[2, 1] - Qr[2, 0] * Qr[1, 1]
            self.mg.add("pd_q00", abs(q00) / (abs(Quu[0, 0]) + abs(rho)))
            self.mg.add("pd_c22", abs(c22) / (abs(t1) + abs(t2)))
            self.mg.add("pd_det", abs(det) / (abs(Qr[0, 0] * c00) + abs(Qr[1, 0] * c01) + abs(Qr[2, 0] * c02)))
            if not (q00 > 0 and c22 > 0 and det > 0):
                return False, K, d, dV
            Qi = Qr ** -1
            K[k], d[k] = -Qi * Qux, -Qi * Qu
            QuuK, Quud = Quu * K[k], Quu * d[k]
            s = Qx + K[k].T * Quud + K[k].T * Qu + Qux.T * d[k]
            Sn = Qxx + K[k].T * QuuK + K[k].T * Qux + Qux.T * K[k]
            S = (Sn + Sn.T) / 2
            dV[0] += (d[k].T * Qu)[0]
            dV[1] += (d[k].T * Quud)[0] / 2
        return True, K, d, dV

    # ---- regularisation schedule --------------------------------------------------------------------------------------
    def reg_increase(self, rho, drho):
        sc = _f(self.o["reg_scale"])
        drho = max(drho * sc, sc)
        return max(rho * drho, _f(self.o["reg_min"])), drho

    def reg_decrease(self, rho, drho):
        sc = _f(self.o["reg_scale"])
        drho = min(drho / sc, 1 / sc)
        r = rho * drho
        self.mg.rel("reg_min", r, _f(self.o["reg_min"]))
        return (r if r > _f(self.o["reg_min"]) else mpf(0)), drho


def solve_reference(x0, xf, Bt, tau0, dtau, dt, Jcm, Qd, Qfd, Rd, ulo, uhi, U0, trace_rows=64, **options):
    """One trajectory of tsat_solve_batch over N = len(U0) + 1 knots. options: fields of tsat_options by name (SOLVE_DEFAULTS).
    Returns dict of mpf: X (N, 7), U (N-1, 3), K (N-1, 7, 3) of the last successful backward sweep in the layout of the ABI (None
    if there was none; column 6 zero with error_state = 1), d (N-1, 3), stats (dict of the fields of tsat_stats), trace (rows of
    8), ls_log (outer, inner, candidate, accepted roll-out, largest |x| or |u|) of every candidate, margins (kind -> smallest), exact (kind -> number of ties by construction), min_margin."""
    o = dict(SOLVE_DEFAULTS)
    o.update(options)
    with mp.workdps(TRACK_DPS):
        sv = _Solve(x0, xf, Bt, tau0, dtau, dt, Jcm, Qd, Qfd, Rd, ulo, uhi, o)
        N = sv.N = len(U0) + 1
        mg = sv.mg
        U = [[_f(v) for v in row] for row in U0]
        al = dict(lam=[[mpf(0)] * 6 for _ in range(N - 1)], nu=[mpf(0)] * 7, mu=_f(o["penalty_init"]))
        st = dict(status=ST_MAX_OUTER, outer_iters=0, inner_iters=0, ls_trials=0, n_backward=0, n_forward=1, bp_restarts=0, fp_fails=0,
                  grad=mpf(0))
        trace, ls_log, Kl, dl = [], [], None, None
        ok0, X, _ = sv.rollout(None, U, None, None, mpf(0), False)
        if not ok0:
            st["status"] = ST_DIVERGED
        else:
            for outer in range(1, int(o["max_outer"]) + 1):
                Jprev = sv.total_cost(X, U, al)
                rho, drho, djz, regfail = _f(o["reg_init"]), mpf(0), 0, False
                for it in range(1, int(o["max_inner"]) + 1):
                    while True:
                        st["n_backward"] += 1
                        good, K, d, dV = sv.backward(X, U, al, rho)
                        if good:
                            Kl, dl = K, d
                            break
                        st["bp_restarts"] += 1
                        rho, drho = sv.reg_increase(rho, drho)
                        mg.rel("reg_max", rho, _f(o["reg_max"]))
                        if rho > _f(o["reg_max"]):
                            regfail = True
                            break
                    if regfail:
                        break
                    rho_used = rho
                    rho, drho = sv.reg_decrease(rho, drho)
                    alpha, J, jacc = mpf(1), Jprev, -1
                    for j in range(int(o["max_linesearch"])):
                        st["n_forward"] += 1
                        st["ls_trials"] += 1
                        ok, Xc, Uc = sv.rollout(X, U, K, d, alpha, True)
                        ls_log.append((outer, it, j, ok, float(sv.largest)))
                        if ok:
                            Jc = sv.total_cost(Xc, Uc, al)
                            t1, t2 = -alpha * dV[0], -alpha * alpha * dV[1]
                            expected = t1 + t2
                            mg.add("expected", abs(expected) / (abs(t1) + abs(t2)) if expected != 0 else 0)
                            z = (Jprev - Jc) / expected if expected > 0 else mpf(-1)
                            lo, hi = _f(o["ls_lower"]), _f(o["ls_upper"])
                            m_lo, m_hi = abs(z - lo) / max(abs(z), lo), abs(z - hi) / max(abs(z), hi)
                            inr = z > lo and z <= hi
                            m_rng = min(m_lo, m_hi) if inr else max([m for m, f in ((m_lo, not z > lo), (m_hi, not z <= hi)) if f])
                            less = Jc < Jprev
                            m_J = abs(Jc - Jprev) / max(abs(Jc), abs(Jprev))
                            if inr or less:
                                mg.add("accept", max([m for m, f in ((m_rng, inr), (m_J, less)) if f]))
                                jacc, J = j, Jc
                                break
                            mg.add("accept", min(m_rng, m_J))
                        alpha = alpha / 2
                    if jacc >= 0:
                        X, U = Xc, Uc
                    else:
                        st["fp_fails"] += 1
                        J = Jprev
                        rho, drho = sv.reg_increase(rho, drho)
                        rho += _f(o["reg_fp"])
                    dJ = abs(J - Jprev)
                    if len(trace) < trace_rows:
                        trace.append([mpf(outer), mpf(it), Jprev, J, mpf(jacc), rho_used, dV[0], dV[1]])
                    if jacc >= 0:
                        mg.add("dJ_zero", dJ / max(abs(J), abs(Jprev)))
                    else:
                        mg.tie("dJ_zero")                               # no candidate accepted: J is Jprev itself
                    Jprev = J
                    djz = djz + 1 if dJ == 0 else 0
                    g = mpf(0)
                    for k in range(N - 1):
                        g += max(abs(d[k][a]) / (abs(U[k][a]) + 1) for a in range(3))
                    st["grad"] = g / (N - 1)
                    st["inner_iters"] += 1
                    if dJ > 0:
                        mg.rel("cost_tol", dJ, _f(o["cost_tol"]))
                        if dJ < _f(o["cost_tol"]):
                            break
                    mg.rel("grad_tol", st["grad"], _f(o["grad_tol"]))
                    if st["grad"] < _f(o["grad_tol"]):
                        break
                    if djz > int(o["dj_counter_limit"]):
                        break
                st["outer_iters"] = outer
                cm = sv.max_violation(X, U)
                if regfail:
                    st["status"] = ST_REG_FAIL
                    break
                mg.rel("constraint_tol", cm, _f(o["constraint_tol"]))
                if cm < _f(o["constraint_tol"]):
                    st["status"] = ST_CONVERGED
                    break
                if outer == int(o["max_outer"]):
                    break
                mu, dmax = al["mu"], _f(o["dual_max"])
                for k in range(N - 1):
                    for a in range(3):
                        for i, c in ((a, U[k][a] - sv.uhi[a]), (3 + a, sv.ulo[a] - U[k][a])):
                            v = al["lam"][k][i] + mu * c
                            if v == 0:
                                mg.tie("dual_clamp")                    # lambda = 0 and the control on its bound by construction
                            else:
                                mg.add("dual_clamp", abs(v) / (abs(al["lam"][k][i]) + abs(mu * c)))
                            mg.rel("dual_clamp", v, dmax)
                            al["lam"][k][i] = min(max(v, mpf(0)), dmax)
                for i in range(7):
                    if sv.mask >> i & 1:
                        v = al["nu"][i] + mu * (X[N - 1][i] - sv.xf[i])
                        mg.rel("dual_clamp", abs(v), dmax)
                        al["nu"][i] = min(max(v, -dmax), dmax)
                v = mu * _f(o["penalty_scale"])
                mg.rel("penalty_clamp", v, _f(o["penalty_max"]))
                al["mu"] = min(v, _f(o["penalty_max"]))
        st["c_max"] = sv.max_violation(X, U)
        st["cost"] = sv.total_cost(X, U, al, False)
        st["cost_al"] = sv.total_cost(X, U, al, True)
        for k in range(N - 1):
            sv.rows(k)                                                  # (a diverged roll-out has looked every row up already)
        Kabi = None
        if Kl is not None and all(k is not None for k in Kl):
            nh = 6 if sv.es else 7
            Kabi = [[[Kl[k][a, j] if j < nh else mpf(0) for a in range(3)] for j in range(7)] for k in range(N - 1)]
            dl = [[dl[k][a] for a in range(3)] for k in range(N - 1)]
        else:
            dl = None
        return dict(X=X, U=U, K=Kabi, d=dl, stats=st, trace=trace, ls_log=ls_log, margins=dict(mg.kinds), exact=dict(mg.exact), min_margin=mg.min())
