"""The field-table chain and the Gramian horizon once more, in mpmath at 80 significant digits, and (second half of the file) the
closed-loop tracking of tsat_tvlqr_batch at 50: what the reference's text computes when no operation rounds. Transcribed from the same Julia lines as refmath_igrf.py / refmath.py: kep_ECI
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
