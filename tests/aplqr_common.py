"""Shared pieces of tests/test_aplqr.py (CPU tier) and tests/test_gpu_aplqr.py (GPU tier): the ASYMPTOTIC PERIODIC LQR on the
dispersed plants (tsat_aplqr_gains, tsat_aplqr_ensemble).

THE REFERENCES
  roll-out   ``reference_loop``: a numpy closed loop of its own (``reference_rollout.ensemble_loop`` forms the body field for the PD
             law only), built from ``reference_rollout.plant_step``, ``limit``, ``rows_of``, ``plant_of`` and the oracle's
             primitives (``ol.qmult``, ``ol.qrot``), with the command of include/tortoise_hip.h: ``law``. ``reference_pairs`` drives
             it over (t, m) pairs and returns the dict of ``reference_rollout.pairs_of`` that ``dispersed_common.compare`` takes.
  synthesis  ``gamma_numpy`` (the Gramian, term by term as the header writes it); ``care_mp``: the sign iteration in mpmath at 50
             digits, run until the step is below 1e-45, its residual checked below 1e-40 — THE reference of P; ``care_scipy``
             (``scipy.linalg.solve_continuous_are``) as a second witness; ``care_numpy``: a numpy-double restatement of the
             iteration of tsat_aplqr.hpp (Gauss-Jordan with partial pivoting, |det| from the pivots, P by a Gram-Schmidt QR).
  THE CARE BAR  ``e_ref`` = the larger of the normalised elementwise errors of scipy and of the restatement against the 50-digit P,
             max_ij |dP_ij| / sqrt(P_ii P_jj); emulator and GPU must stay within 4 e_ref per case (the factor of
             profiles/solve_mp/e_ref.txt).

THE FIXTURE of the roll-out tests is that of tests/test_gpu_pd.py (``pd_common.case``); the weights QD, RD, ALPHA below were chosen so
that the conditions of ``conditions`` hold on the reference alone. Its tables span 3.2 s of an orbit, so Gamma is nearly of rank two and
the gain along the field is large (1e12): the equation is still solved (status 0), and a gain of that size is what makes the full-gain
slews clip at every knot."""
import ctypes as C
import math

import numpy as np

import dispersed_common as dc
import ensemble_common as ec
import gg_common as gc
import helpers
import pd_common as pc
import reference_rollout as rr

# the weights of the roll-out fixture: [theta (3); dw (3)], the dipole weights (1 / (A m^2)^2) and the gain scale
QD = np.array([3e-4, 2e-4, 4e-4, 2.0e2, 3.0e2, 1.5e2])
RD = np.array([2.0e3, 3.0e3, 2.5e3])
ALPHA = np.array([1.0, 1.0, 1.0, 0.01, 1.0, 0.01, 0.01, 1.0])     # per slew: the full gain clips at every knot of a regulation, 1 % never does
RES_TOL = 3.3e-12        # tracking.APLQR_RES_TOL, asserted equal in the tests
# the residual is a sum of 19 products per entry, each rounded, over a denominator that bounds their sizes: two evaluations of it in
# double agree to some 19 eps however small the residual itself is
RES_NOISE = 19 * np.finfo(float).eps

INFO_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("residual", "<f8"), ("pivot_min", "<f8")])


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def jmat_of(batch, t):
    return np.asarray(batch.Jmat[t], dtype=np.float64).reshape(3, 3).T


def double_integrator():
    A = np.zeros((6, 6))
    A[:3, 3:] = np.eye(3)
    return A


def gamma_numpy(ol, xf, rows, J, rd):
    """(1/n) sum_j B_j diag(1/rd) B_j', B_j = -inv(J) hat(qrot(xf[3:7] / |xf[3:7]|, row j))"""
    q = xf[3:7] / math.sqrt(float(xf[3:7] @ xf[3:7]))
    Ji = np.linalg.inv(J)
    G = np.zeros((3, 3))
    for b in rows:
        B = -Ji @ hat(ol.qrot(q, np.asarray(b, dtype=np.float64)))
        G += B @ np.diag(1.0 / np.asarray(rd)) @ B.T
    return G / len(rows)


def block_g(Gamma):
    """G = blockdiag(0, Gamma), exactly symmetric (a sum of B D B' is symmetric only to rounding, and the equation is posed for a
    symmetric G)"""
    G = np.zeros((6, 6))
    G[3:, 3:] = 0.5 * (Gamma + Gamma.T)
    return G


def residual(A, G, Q, P):
    """the relative residual of tsat_aplqr_info"""
    fro = np.linalg.norm
    return float(fro(A.T @ P + P @ A - P @ G @ P + Q) / (2 * fro(A) * fro(P) + fro(G) * fro(P) ** 2 + fro(Q)))


def _gauss_jordan(M, n):
    """[Z | R] -> inv(Z) R with partial pivoting, in place; (sum of log |pivot|, smallest |pivot|) or None at a zero / non-finite pivot"""
    logdet, pmin = 0.0, np.inf
    for p in range(n):
        pr = p + int(np.argmax(np.abs(M[p:n, p])))
        best = abs(M[pr, p])
        if not (best > 0.0) or not np.isfinite(best):
            return None
        logdet, pmin = logdet + math.log(best), min(pmin, best)
        if pr != p:
            M[[p, pr]] = M[[pr, p]]
        M[p] = M[p] * (1.0 / M[p, p])
        for r in range(n):
            if r != p:
                M[r] = M[r] - M[r, p] * M[p]
    return logdet, pmin


def care_numpy(A, G, Q, res_tol=np.inf, max_iter=32):
    """the restatement of care6 in numpy double: (P, status, iterations, residual, pivot_min); P zero unless status == 0"""
    n = 6
    Z = np.block([[A, -G], [-Q, -A.T]])
    pmin, it, ok = np.inf, 0, False
    for it in range(1, max_iter + 1):
        M = np.hstack([Z, np.eye(2 * n)])
        gj = _gauss_jordan(M, 2 * n)
        if gj is None:
            return np.zeros((n, n)), 2, it, 0.0, pmin
        pmin = min(pmin, gj[1])
        c = math.exp(-gj[0] / (2 * n))
        Zn = 0.5 * (c * Z + M[:, 2 * n:] / c)
        nd, nz = np.abs(Zn - Z).sum(axis=0).max(), np.abs(Zn).sum(axis=0).max()
        Z = Zn
        if nd <= 1e-14 * nz:
            ok = True
            break
    if not ok:
        return np.zeros((n, n)), 1, it, 0.0, pmin
    Mn = np.vstack([Z[:n, n:], Z[n:, n:] + np.eye(n)])
    Rn = -np.vstack([Z[:n, :n] + np.eye(n), Z[n:, :n]])
    # modified Gram-Schmidt over the columns of [Mn | Rn], then back-substitution
    W = np.hstack([Mn, Rn])
    R, Y = np.zeros((n, n)), np.zeros((n, n))
    for j in range(n):
        s2 = float(W[:, j] @ W[:, j])
        if not (s2 > 0.0) or not np.isfinite(s2):
            return np.zeros((n, n)), 2, it, 0.0, pmin
        q = W[:, j] / math.sqrt(s2)
        R[j, j] = math.sqrt(s2)
        d = q @ W
        R[j, j + 1:], Y[j] = d[j + 1:n], d[n:]
        keep = W[:, j].copy()
        W = W - np.outer(q, d)
        W[:, j] = keep
    pmin = min(pmin, float(np.diag(R).min()))
    X = np.zeros((n, n))
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - R[i, i + 1:] @ X[i + 1:]) / R[i, i]
    P = 0.5 * (X + X.T)
    res = residual(A, G, Q, P)
    if not (res <= res_tol):
        return np.zeros((n, n)), 3, it, res, pmin
    return P, 0, it, res, pmin


def care_mp(A, G, Q):
    """P by the same sign iteration in mpmath at 50 digits: run until the step is below 1e-45, the residual checked below 1e-40.
    Returns P as a numpy double array (the nearest doubles) — None when the iteration does not get there (no stabilising solution)"""
    import mpmath as mp
    with mp.workdps(50):
        n = 6
        H = np.block([[A, -G], [-Q, -A.T]])
        Z = mp.matrix(H.tolist())
        for _ in range(200):
            try:
                Zi = Z ** -1
                c = abs(mp.det(Z)) ** (mp.mpf(-1) / (2 * n))
            except ZeroDivisionError:
                return None
            Zn = (c * Z + Zi / c) / 2
            step = mp.mnorm(Zn - Z, 1) / mp.mnorm(Zn, 1)
            Z = Zn
            if step < mp.mpf("1e-45"):
                break
        else:
            return None
        I6 = mp.eye(n)
        Mn = mp.matrix(2 * n, n)
        Rn = mp.matrix(2 * n, n)
        for r in range(n):
            for j in range(n):
                Mn[r, j], Mn[n + r, j] = Z[r, n + j], Z[n + r, n + j] + I6[r, j]
                Rn[r, j], Rn[n + r, j] = -(Z[r, j] + I6[r, j]), -Z[n + r, j]
        Qm, Rm = mp.qr(Mn, mode="skinny")
        P = Rm ** -1 * (Qm.T * Rn)
        P = (P + P.T) / 2
        Am, Gm, Qm = mp.matrix(A.tolist()), mp.matrix(G.tolist()), mp.matrix(Q.tolist())
        R = Am.T * P + P * Am - P * Gm * P + Qm
        fro = lambda X: mp.mnorm(X, "f")
        res = fro(R) / (2 * fro(Am) * fro(P) + fro(Gm) * fro(P) ** 2 + fro(Qm))
        if not res < mp.mpf("1e-40"):
            return None
        return np.array([[float(P[i, j]) for j in range(n)] for i in range(n)])


def care_scipy(A, G, Q):
    """scipy's solution, with B B' = G from the symmetric eigen-decomposition (G is positive semi-definite) and R = I"""
    import scipy.linalg as sl
    w, V = np.linalg.eigh(0.5 * (G + G.T))
    B = V * np.sqrt(np.maximum(w, 0.0))
    return sl.solve_continuous_are(A, B, Q, np.eye(6))


def nerr(P, Pref):
    """max_ij |P_ij - Pref_ij| / sqrt(Pref_ii Pref_jj)"""
    d = np.sqrt(np.diag(Pref))
    return float(np.max(np.abs(P - Pref) / np.outer(d, d)))


def care_bar(A, G, Q):
    """(P_ref, e_ref, restatement's residual) of one case: the 50-digit P and the larger error of the two double witnesses"""
    Pref = care_mp(A, G, Q)
    assert Pref is not None, "the 50-digit iteration did not converge on a case that has to have a stabilising solution"
    Pn, status, _, res, _ = care_numpy(A, G, Q)
    assert status == 0, "the numpy restatement fails on this case"
    e_sc, e_np = nerr(care_scipy(A, G, Q), Pref), nerr(Pn, Pref)
    return Pref, max(e_sc, e_np), res, (e_sc, e_np)


def check_p(P, Pref, e_ref, A, G, label=""):
    """the CARE bar and the properties: within 4 e_ref, A - G P stable, P symmetric positive definite"""
    e = nerr(P, Pref)
    print(f"{label}: normalised error {e:.2e}, e_ref {e_ref:.2e} (bar {4 * e_ref:.2e})")
    assert e <= 4 * e_ref, (label, e, e_ref)
    assert np.array_equal(P, P.T)
    assert np.linalg.eigvalsh(P).min() > 0
    assert np.linalg.eigvals(A - G @ P).real.max() < 0


# ---- the cases of care6 alone -------------------------------------------------------------------------------------------------

W0 = 1.13e-3             # orbital rate of the sets below, rad/s
J_1U = np.diag([1.25e-3] * 3)
J_3U = np.diag([0.005256, 0.04939, 0.04939])
J_FULL = np.array([[1.2e-3, 1e-5, 0.0], [1e-5, 1.3e-3, 2e-5], [0.0, 2e-5, 1.1e-3]])


def _orbit_rows(inc_deg, n=400):
    im, t = np.deg2rad(inc_deg), np.linspace(0, 2 * np.pi / W0, n, endpoint=False)
    return (7.9e15 / 6771e3 ** 3 * np.array([np.cos(W0 * t) * np.sin(im), -np.cos(im) * np.ones_like(t), 2 * np.sin(W0 * t) * np.sin(im)])).T


def _gamma_plain(J, rinv, rows):
    Ji, G = np.linalg.inv(J), np.zeros((3, 3))
    for b in rows:
        B = -Ji @ hat(b)
        G += B @ np.diag(rinv) @ B.T
    return G / len(rows)


def reference_a(J):
    """the reference's own A (src/comparison/psiaki_dynamics.jl:113-119): local-level goal, orbit-rate and gravity-gradient terms"""
    s = [(J[1, 1] - J[2, 2]) / J[0, 0], (J[2, 2] - J[0, 0]) / J[1, 1], (J[0, 0] - J[1, 1]) / J[2, 2]]
    A = double_integrator()
    A[3, 0], A[3, 5] = -4 * W0 ** 2 * s[0], W0 * (1 - s[0])
    A[4, 1] = 3 * W0 ** 2 * s[1]
    A[5, 2], A[5, 3] = W0 ** 2 * s[2], -W0 * (1 + s[2])
    return A


def named_cases():
    """four weight / inertia sets on the double integrator — the reference's 1U weights, the 3U inertia, a full inertia tensor with
    Bryson-size weights, a 2 degree inclination dipole — and the reference's own A with the 3U inertia: (name, A, G, Q)"""
    A0 = double_integrator()
    sets = [("reference 1U weights", J_1U, [1 / 8e6] * 3, [1.5e-4] * 3 + [1e4] * 3, 88.0, A0),
            ("3U inertia", J_3U, [1 / 8e6] * 3, [1.5e-4] * 3 + [1e4] * 3, 51.0, A0),
            ("full tensor, Bryson-size weights", J_FULL, [1e2, 2e2, 1.5e2], [1e4] * 3 + [1e5] * 3, 97.0, A0),
            ("2 deg inclination", J_1U, [1 / 8e6] * 3, [1.0] * 6, 2.0, A0),
            ("reference A, 3U inertia", J_3U, [1 / 8e6] * 3, [1.5e-4] * 3 + [1e4] * 3, 51.0, reference_a(J_3U))]
    return [(name, A, block_g(_gamma_plain(J, rinv, _orbit_rows(inc))), np.diag(qd)) for name, J, rinv, qd, inc, A in sets]


def random_cases(n=20, seed=11):
    """random stabilisable (A, G >= 0, Q > 0): A dense of unit size, G = B B' with B 6 x 3 (controllable with probability one), Q a
    random positive definite matrix of condition <= 100"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        A = rng.standard_normal((6, 6))
        B = rng.standard_normal((6, 3))
        V, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        Q = (V * 10.0 ** rng.uniform(-1, 1, 6)) @ V.T
        out.append((f"random {i}", A, B @ B.T, 0.5 * (Q + Q.T)))
    return out


# ---- the synthesis on slews ----------------------------------------------------------------------------------------------------

N_ROWS = 130
WINDOWS = ((3, 5), (10, 73), (0, 64), (60, 125), (1, 130), (0, 130))     # 2, 63, 64, 65, 129 rows and the whole table
GAINS_BIDX = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)


def gains_case(pkg):
    """T = 6 slews sharing two 130-row dipole tables whose last row is zero, the 3U inertia on the even slews and a full tensor on the
    odd ones, the windows WINDOWS. Returns dict(xf, Btab, bidx, lo, hi, Jmat, qd, rd, alpha)."""
    ss = pkg.slew_setup
    rng = np.random.default_rng(23)
    T = len(WINDOWS)
    Btab = np.stack([ss.dipole_btable(N_ROWS, 40.0, gc.A_KM, gc.INC, ra, nu) for ra, nu in pc.ORBITS])
    Btab[:, -1, :] = 0.0
    xf = np.zeros((T, 7))
    q = rng.standard_normal((T, 4))
    xf[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None] * 1.0000003          # not exactly unit: the kernel normalises
    Jfull = 40.0 * J_FULL
    Jmat = np.stack([(J_3U if t % 2 == 0 else Jfull).T.reshape(9) for t in range(T)])
    qd = QD * rng.uniform(0.5, 2.0, (T, 6))
    rd = RD * rng.uniform(0.5, 2.0, (T, 3))
    return dict(xf=np.ascontiguousarray(xf), Btab=np.ascontiguousarray(Btab), bidx=GAINS_BIDX, lo=np.array([w[0] for w in WINDOWS], dtype=np.int32),
                hi=np.array([w[1] for w in WINDOWS], dtype=np.int32), Jmat=np.ascontiguousarray(Jmat), qd=qd, rd=rd,
                alpha=np.linspace(0.5, 1.5, T))


def gains_reference(ol, c):
    """per slew: Gamma (numpy), the 50-digit P with its e_ref, and Kg = alpha inv(J) P[3:6, :] as (6, 3)"""
    ol.load()
    out = []
    A = double_integrator()
    for t in range(len(c["lo"])):
        J = c["Jmat"][t].reshape(3, 3).T
        rows = c["Btab"][c["bidx"][t], c["lo"][t]:c["hi"][t]]
        Gm = gamma_numpy(ol, c["xf"][t], rows, J, c["rd"][t])
        G, Q = block_g(Gm), np.diag(c["qd"][t])
        Pref, e_ref, res, _ = care_bar(A, G, Q)
        out.append(dict(Gamma=Gm, G=G, Q=Q, P=Pref, e_ref=e_ref, res=res, Kg=(c["alpha"][t] * np.linalg.inv(J) @ Pref[3:6, :]).T, J=J,
                        alpha=float(c["alpha"][t])))
    return out


def check_gains(ref, Kg, info, label=""):
    """Gamma to 1e-13 of its LARGEST entry (normwise, not per entry: every entry is a sum over the rows of products of the size of
    the largest one, so an off-diagonal entry that cancels carries the rounding of terms of that size, and a bound relative to the
    cancelled value would measure the cancellation, not the kernel), P by the CARE bar, Kg by the bar its entries of P hand down"""
    A = double_integrator()
    for t, r in enumerate(ref):
        assert info["status"][t] == 0, (label, t, info["status"][t])
        dG = float(np.max(np.abs(info["Gamma"][t] - r["Gamma"])) / np.max(np.abs(r["Gamma"])))
        print(f"{label} slew {t}: Gamma relative error {dG:.2e}, {int(info['iterations'][t])} iterations, residual {info['residual'][t]:.2e}")
        assert dG <= 1e-13
        check_p(info["P"][t], r["P"], r["e_ref"], A, r["G"], f"{label} slew {t}")
        # Kg[j, c] = alpha sum_i inv(J)[c, i] P[3 + i, j]: each term inherits the bar of its entry of P; 4 ulp for the sum itself
        d, Ji = np.sqrt(np.diag(r["P"])), np.abs(np.linalg.inv(r["J"]))
        bound = r["alpha"] * 4 * r["e_ref"] * np.outer(d, Ji @ d[3:6]) + 4 * np.finfo(float).eps * np.abs(r["Kg"]).max()
        assert np.all(np.abs(Kg[t] - r["Kg"]) <= bound), (label, t)
        assert abs(info["residual"][t] - residual(A, r["G"], r["Q"], info["P"][t])) <= 1e-3 * info["residual"][t] + RES_NOISE


def rank_case(ol, c):
    """two slews on table 0 of ``gains_case``: a ONE-ROW window (Gamma of rank two) and a window of two rows 1e-2 rad apart. Asserted
    here, on the numpy restatement alone: it fails on the first and solves the second within RES_TOL"""
    B = c["Btab"].copy()
    b = B[0, 20]
    axis = np.cross(b, [0.0, 0.0, 1.0])
    axis /= np.linalg.norm(axis)
    B[0, 21] = b + 1e-2 * np.cross(axis, b)
    two = {k: (v[:2].copy() if k != "Btab" else np.ascontiguousarray(B)) for k, v in c.items()}
    two["bidx"][:] = 0
    two["lo"][:], two["hi"][:] = (20, 20), (21, 22)
    two["Jmat"][1] = two["Jmat"][0]
    ol.load()
    status = []
    for t in range(2):
        Gm = gamma_numpy(ol, two["xf"][t], B[0, two["lo"][t]:two["hi"][t]], two["Jmat"][t].reshape(3, 3).T, two["rd"][t])
        status.append(care_numpy(double_integrator(), block_g(Gm), np.diag(two["qd"][t]), RES_TOL)[1])
    assert status[0] != 0, "the restatement solves the one-row window: not the case this is about"
    assert status[1] == 0, "the restatement fails on the two nearly parallel rows: not the case this is about"
    return two


def check_rank_case(Kg, info, label=""):
    """the one-row window comes back with a status, zero-filled and finite; the two nearly parallel rows with status 0, a gain, and a
    stable A - G P"""
    print(f"{label}: one row: status {info['status'][0]} after {info['iterations'][0]} iterations, smallest pivot {info['pivot_min'][0]:.2e}; "
          f"two rows: status {info['status'][1]} after {info['iterations'][1]} iterations, residual {info['residual'][1]:.2e}, "
          f"smallest pivot {info['pivot_min'][1]:.2e}")
    assert info["status"][0] != 0 and not Kg[0].any() and not info["P"][0].any()
    assert np.all(np.isfinite(Kg)) and np.all(np.isfinite(info["P"])) and np.all(np.isfinite(info["Gamma"]))
    assert np.linalg.matrix_rank(info["Gamma"][0], tol=1e-12 * np.abs(info["Gamma"][0]).max()) == 2
    assert info["status"][1] == 0 and Kg[1].any()
    assert np.linalg.eigvals(double_integrator() - block_g(info["Gamma"][1]) @ info["P"][1]).real.max() < 0


class GainsCall:
    """the arguments of tsat_aplqr_gains after the handle, by name, for the rejection tests"""
    FIELDS = ("T", "n_btab", "n_tab", "xf", "Btab", "btab_idx", "avg_lo", "avg_hi", "Jmat", "qd", "rd", "alpha", "res_tol", "Kg", "P_ss", "Gamma",
              "info")

    def __init__(self, abi, c, res_tol=RES_TOL):
        T = len(c["lo"])
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.abi = abi
        self.v = dict(T=T, n_btab=c["Btab"].shape[0], n_tab=c["Btab"].shape[1], xf=f(c["xf"]), Btab=f(c["Btab"]),
                      btab_idx=np.ascontiguousarray(c["bidx"], dtype=np.int32), avg_lo=np.ascontiguousarray(c["lo"], dtype=np.int32),
                      avg_hi=np.ascontiguousarray(c["hi"], dtype=np.int32), Jmat=f(c["Jmat"]), qd=f(c["qd"]), rd=f(c["rd"]),
                      alpha=f(c["alpha"]), res_tol=float(res_tol), Kg=np.full((T, 6, 3), np.nan), P_ss=np.full((T, 6, 6), np.nan),
                      Gamma=np.full((T, 3, 3), np.nan), info=np.zeros(T, dtype=INFO_DTYPE))

    def edit(self, **kw):
        other = type(self).__new__(type(self))
        other.abi, other.v = self.abi, dict(self.v)
        for k, val in kw.items():
            assert k in other.v, k
            other.v[k] = val
        return other

    def c_args(self, names=None):
        out = []
        for n in names or self.FIELDS:
            a = self.v[n]
            if n in ("T", "n_btab"):
                out.append(C.c_int64(a))
            elif n == "n_tab":
                out.append(C.c_int32(a))
            elif n == "res_tol":
                out.append(C.c_double(a))
            elif a is None:
                out.append(None)
            elif n == "info":
                out.append(a.ctypes.data_as(C.c_void_p))
            elif a.dtype == np.int32:
                out.append(self.abi.as_ip(a))
            else:
                out.append(self.abi.as_dp(np.ascontiguousarray(a, dtype=np.float64)))
        return out

    def result(self):
        v = self.v
        return v["Kg"], dict(status=v["info"]["status"], iterations=v["info"]["iterations"], residual=v["info"]["residual"],
                             pivot_min=v["info"]["pivot_min"], P=v["P_ss"], Gamma=v["Gamma"])


def gains_rejections(call):
    """every rejection of tsat_aplqr_gains as (label, edited call, words of the text)"""
    v = call.v
    T = v["T"]
    bad = lambda a, idx, val: (lambda x: (x.__setitem__(idx, val), x)[1])(np.array(a))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return [
        ("T = 0", call.edit(T=0), "bad batch dimensions"), ("n_tab = 0", call.edit(n_tab=0), "bad batch dimensions"),
        ("n_btab = 0", call.edit(n_btab=0), "bad batch dimensions"),
        ("xf NULL", call.edit(xf=None), "null array"), ("Btab NULL", call.edit(Btab=None), "null array"),
        ("Jmat NULL", call.edit(Jmat=None), "null array"), ("qd NULL", call.edit(qd=None), "null array"),
        ("rd NULL", call.edit(rd=None), "null array"), ("alpha NULL", call.edit(alpha=None), "null array"),
        ("Kg NULL", call.edit(Kg=None), "null array"), ("info NULL", call.edit(info=None), "null array"),
        ("avg_lo alone", call.edit(avg_hi=None), "exactly one of avg_lo / avg_hi is NULL"),
        ("avg_hi alone", call.edit(avg_lo=None), "exactly one of avg_lo / avg_hi is NULL"),
        ("btab_idx NULL", call.edit(btab_idx=None), "btab_idx is NULL but n_btab != T"),
        ("btab_idx range", call.edit(btab_idx=i32(np.full(T, 2))), "btab_idx out of range"),
        ("btab_idx negative", call.edit(btab_idx=i32(bad(v["btab_idx"], 1, -1))), "btab_idx out of range"),
        ("empty window", call.edit(avg_hi=i32(bad(v["avg_hi"], 2, v["avg_lo"][2]))), "0 <= avg_lo < avg_hi <= n_tab (t = 2)"),
        ("window past the table", call.edit(avg_hi=i32(bad(v["avg_hi"], 5, v["n_tab"] + 1))), "0 <= avg_lo < avg_hi <= n_tab (t = 5)"),
        ("negative window", call.edit(avg_lo=i32(bad(v["avg_lo"], 0, -1))), "0 <= avg_lo < avg_hi <= n_tab (t = 0)"),
        ("qd zero", call.edit(qd=bad(v["qd"], (1, 4), 0.0)), "qd must be finite and > 0 (t = 1)"),
        ("qd NaN", call.edit(qd=bad(v["qd"], (0, 0), np.nan)), "qd must be finite and > 0 (t = 0)"),
        ("rd negative", call.edit(rd=bad(v["rd"], (3, 2), -1.0)), "rd must be finite and > 0 (t = 3)"),
        ("rd inf", call.edit(rd=bad(v["rd"], (T - 1, 0), np.inf)), f"rd must be finite and > 0 (t = {T - 1})"),
        ("alpha negative", call.edit(alpha=bad(v["alpha"], 2, -0.1)), "alpha must be finite and >= 0 (t = 2)"),
        ("alpha NaN", call.edit(alpha=bad(v["alpha"], 0, np.nan)), "alpha must be finite and >= 0 (t = 0)"),
        ("res_tol zero", call.edit(res_tol=0.0), "res_tol must be > 0"), ("res_tol NaN", call.edit(res_tol=float("nan")), "res_tol must be > 0"),
        ("zero quaternion", call.edit(xf=bad(v["xf"], (1, slice(3, 7)), 0.0)), "non-zero quaternion (t = 1)"),
        ("Jmat NaN", call.edit(Jmat=bad(v["Jmat"], (4, 3), np.nan)), "Jmat must be finite (t = 4)"),
        ("Jmat singular", call.edit(Jmat=bad(v["Jmat"], (2, slice(0, 9)), 0.0)), "Jmat is singular (t = 2)"),
    ]


# ---- the roll-out ---------------------------------------------------------------------------------------------------------------

def law(ol, xr, ur, Kg, rd, w, q, b, us, sign_rule=True):
    """the command of include/tortoise_hip.h before the limit: Kg (6, 3), b the body-frame field; ur None: no feed-forward"""
    qe = ol.qmult(np.r_[xr[3], -xr[4:7]], q)
    s = -1.0 if (sign_rule and qe[0] < 0) else 1.0
    z = np.r_[2.0 * s * qe[1:4], w - xr[:3]]
    v = Kg.T @ z
    m = -(1.0 / rd) * np.cross(b, v)
    return (ur if ur is not None else np.zeros(3)) + m / us


def reference_loop(ol, batch, t, Xr, Ur, Kg, rd, x0, opts, gid, Rtab=None, gm=0.0, plant=None, lo=None, hi=None, limit_mode=0, noisy=True,
                   sign_rule=True):
    """one closed loop of slew t on the true state, as ``reference_rollout.ensemble_loop`` runs the PD law's. Returns X_sim (N, 7)
    zero-filled beyond the horizon, (n_sure, n_maybe), the commands before the limit, the betas (limit_mode 1), the scalar parts e0"""
    NS = batch.N
    N = NS if batch.n_knots is None else int(batch.n_knots[t])
    us, h = float(opts.u_scale), float(batch.dt[t])
    P = rr.plant_of(batch, t, plant)
    Xs, Uc = np.zeros((NS, 7)), np.zeros((NS - 1, 3))
    x = np.array(x0, dtype=np.float64)
    n_sure = n_maybe = 0
    betas, e0s = [], []
    for k in range(N - 1):
        Xs[k] = x
        xr = batch.xf[t] if Xr is None else Xr[k]
        rows = rr.rows_of(batch, t, k)
        b = ol.qrot(x[3:7] / math.sqrt(float(x[3:7] @ x[3:7])), rows[0])
        e0s.append(float(ol.qmult(np.r_[xr[3], -xr[4:7]], x[3:7])[0]))
        u = law(ol, xr, None if Ur is None else Ur[k], Kg, rd, x[:3], x[3:7], b, us, sign_rule)
        Uc[k] = u
        u, (sure, maybe), beta = rr.limit(u, lo, hi, limit_mode)
        n_sure, n_maybe = n_sure + sure, n_maybe + maybe
        if beta is not None:
            betas.append(beta)
        x = rr.plant_step(ol, batch, t, k, x, u, P, us, h, opts, gid, k, noisy, Rtab, gm)
    Xs[N - 1] = x
    return Xs, (n_sure, n_maybe), Uc, betas, e0s


def reference_pairs(ol, abi, batch, x0_sim, Kg, rd, opts, pairs, X=None, U=None, Rtab=None, gm=0.0, plant=None, sat=None, limit_mode=0,
                    x0_nom=None, noise_id0=None, sign_rule=True):
    """``reference_loop`` on the (t, m) pairs; m = -1 is the noise-free MODEL plant from x0_nom[t] (default X[t, 0]). Kg (T, 6, 3),
    rd (T, 3) or (3,). Returns the dict ``dispersed_common.compare`` takes, with U_cmd, betas and e0 per pair."""
    T, M = x0_sim.shape[:2]
    id0 = np.arange(T, dtype=np.int64) * M if noise_id0 is None else np.asarray(noise_id0, dtype=np.int64)
    lo, hi = (None, None) if sat is None else (np.broadcast_to(sat[0], (T, 3)), np.broadcast_to(sat[1], (T, 3)))
    rd = np.broadcast_to(rd, (T, 3))
    ol.load()
    res = []
    for p in pairs:
        t, m = int(p[0]), int(p[1])
        kw = dict(lo=None if lo is None else lo[t], hi=None if hi is None else hi[t], limit_mode=limit_mode, sign_rule=sign_rule)
        Xr, Ur = None if X is None else X[t], None if U is None else U[t]
        if m < 0:
            x0 = x0_nom[t] if x0_nom is not None else X[t, 0]
            res.append(reference_loop(ol, batch, t, Xr, Ur, Kg[t], rd[t], x0, opts, 0, Rtab, gm, None, noisy=False, **kw))
        else:
            res.append(reference_loop(ol, batch, t, Xr, Ur, Kg[t], rd[t], x0_sim[t, m], opts, id0[t] + m, Rtab, gm,
                                      None if plant is None else plant[t, m], **kw))
    pairs = np.asarray(pairs)
    Xs = np.stack([r[0] for r in res])
    nk = ec.horizons(batch)[pairs[:, 0]]
    xf = batch.xf[pairs[:, 0]]
    st = dc.stats_of(abi, Xs, xf, nk, batch.dt[pairs[:, 0]], opts.min_steps, opts.w_tol, opts.angle_tol)
    return dict(X_sim=Xs, stats=st, n_sure=np.array([r[1][0] for r in res]), n_maybe=np.array([r[1][1] for r in res]), xf=xf, n_knots=nk,
                U_cmd=np.stack([r[2] for r in res]), betas=[r[3] for r in res], e0=[r[4] for r in res])


def fixture_gains(ol, batch):
    """the gains of the roll-out fixture, from the numpy restatement of the synthesis over each slew's whole table: Kg (T, 6, 3)"""
    ol.load()
    A = double_integrator()
    Kg = np.zeros((batch.T, 6, 3))
    for t in range(batch.T):
        J = jmat_of(batch, t)
        Gm = gamma_numpy(ol, batch.xf[t], batch.Btab[batch.btab_idx[t]], J, RD)
        P, status, *_ = care_numpy(A, block_g(Gm), np.diag(QD))
        assert status == 0
        Kg[t] = (ALPHA[t] * np.linalg.inv(J) @ P[3:6, :]).T
    return Kg


def moved_by(a, b):
    return float(np.max(np.abs(np.asarray(pc.finals(a)) - np.asarray(pc.finals(b)))))


def diagonal_blocks(Kg):
    """Kg with the off-diagonal entries of its two 3 x 3 blocks dropped: the per-axis law a PD controller is"""
    Kd = np.zeros_like(Kg)
    for c in range(3):
        Kd[:, c, c], Kd[:, 3 + c, c] = Kg[:, c, c], Kg[:, 3 + c, c]
    return Kd


def conditions(ref, ref_zero, ref_diag, ref_nosign, batch, M):
    """the conditions of the roll-out fixture, on references of a REGULATION alone (limit_mode 0, every (t, m) in slew order): the law
    moves the final state by >= 1e-6 against Kg = 0; the sign rule decides on at least two slews (e0 < 0 at every knot, and the
    reference with s = +1 differs); some slews clip at every knot and some never; dropping the off-diagonal entries of the blocks of
    Kg moves it by >= 1e-7"""
    d0, dd, ds = moved_by(ref, ref_zero), moved_by(ref, ref_diag), moved_by(ref, ref_nosign)
    neg = [t for t in range(batch.T) if all(v < 0 for e in ref["e0"][t * M:(t + 1) * M] for v in e)]
    nk = ec.horizons(batch) - 1
    sure, maybe = ref["n_sure"].reshape(batch.T, M), ref["n_maybe"].reshape(batch.T, M)
    always = [t for t in range(batch.T) if np.all(sure[t] == nk[t])]
    never = [t for t in range(batch.T) if not maybe[t].any()]
    print(f"conditions: law on against Kg = 0 {d0:.2e}; diagonal blocks only {dd:.2e}; s = +1 {ds:.2e}; e0 < 0 throughout on slews {neg}; "
          f"clip at every knot on slews {always}, never on {never}")
    assert d0 >= 1e-6 and dd >= 1e-7 and ds >= gc.MOVED
    assert len(neg) >= 2 and len(always) >= 1 and len(never) >= 1


def fixture_conditions(ref_of, kw_of, Kg, batch, M=3):
    """every condition of the roll-out fixture, on references alone: ``ref_of(pairs, kw, Kg=None, **extra)`` is the numpy loop on the
    fixture, ``kw_of(kind, mode)`` its call. ``conditions`` on a regulation with limit_mode 0; then: the law moves the final state when
    tracking, with and without feed-forward; the feed-forward does; the direction-preserving limit is not the clip, and no beta sits
    within 100 bands of 1; the gravity term does"""
    pairs = dc.all_pairs(batch.T, M)
    zero = np.zeros_like(Kg)
    kw = kw_of("regulate", 0)
    ref = ref_of(pairs, kw)
    conditions(ref, ref_of(pairs, kw, Kg=zero), ref_of(pairs, kw, Kg=diagonal_blocks(Kg)), ref_of(pairs, kw, sign_rule=False), batch, M)
    for kind in ("track", "track_ff"):
        kwk = kw_of(kind, 0)
        assert moved_by(ref_of(pairs, kwk), ref_of(pairs, kwk, Kg=zero)) >= 1e-6
    kwf = kw_of("track_ff", 0)
    assert moved_by(ref_of(pairs, kwf), ref_of(pairs, dict(kwf, U=None))) >= gc.MOVED
    for kind in ("track", "track_ff", "regulate"):
        kw1 = kw_of(kind, 1)
        r1 = ref_of(pairs, kw1)
        assert moved_by(r1, ref_of(pairs, dict(kw1, limit_mode=0))) >= gc.MOVED
        near = min(abs(x - 1.0) for bs in r1["betas"] for x in bs)
        assert near > 100 * dc.CLIP_BAND, near
    assert moved_by(ref, ref_of(pairs, dict(kw, gm=0.0))) >= gc.MOVED


FIELDS = tuple("Kg" if f == "kd" else ("rd" if f == "kp" else f) for f in pc.FIELDS)


class Call(pc.Call):
    """the arguments of tsat_aplqr_ensemble after the handle: ``pd_common.Call`` with Kg (T, 6, 3) and rd in the places of kd and kp"""

    def __init__(self, abi, batch, opts, x0_sim, Kg, rd, **kw):
        super().__init__(abi, batch, opts, x0_sim, np.zeros(3), np.zeros(3), **kw)
        del self.v["kd"], self.v["kp"]
        self.v["Kg"] = np.ascontiguousarray(Kg, dtype=np.float64)
        self.v["rd"] = np.ascontiguousarray(np.broadcast_to(rd, (batch.T, 3)), dtype=np.float64)

    def c_args(self, names=FIELDS):
        return super().c_args(names)


def rejections(call, batch, Rtab):
    """every rejection of tsat_aplqr_ensemble: the law's own, then those of ``pd_common.rejections`` that are not about kd / kp"""
    T = batch.T
    bad = lambda a, idx, val: (lambda x: (x.__setitem__(idx, val), x)[1])(np.array(a, dtype=np.float64))
    Kg, rd = call.v["Kg"], call.v["rd"]
    own = [("Kg NULL", call.edit(Kg=None), "null Kg or rd"), ("rd NULL", call.edit(rd=None), "null Kg or rd"),
           ("Kg NaN", call.edit(Kg=bad(Kg, (1, 2, 0), np.nan)), "Kg must be finite (t = 1)"),
           ("Kg inf", call.edit(Kg=bad(Kg, (T - 1, 5, 2), -np.inf)), f"Kg must be finite (t = {T - 1})"),
           ("rd zero", call.edit(rd=bad(rd, (0, 1), 0.0)), "rd must be finite and > 0 (t = 0)"),
           ("rd negative", call.edit(rd=bad(rd, (1, 2), -3.0)), "rd must be finite and > 0 (t = 1)"),
           ("rd NaN", call.edit(rd=bad(rd, (T - 1, 0), np.nan)), f"rd must be finite and > 0 (t = {T - 1})")]
    call.v["kd"] = call.v["kp"] = np.zeros((T, 3))               # what pd_common.rejections edits and this call does not carry
    parents = [r for r in pc.rejections(call, batch, Rtab) if not r[0].startswith(("kd", "kp"))]
    del call.v["kd"], call.v["kp"]
    for _, c, _ in parents:
        c.v.pop("kd", None), c.v.pop("kp", None)
    return own + parents


class Emu:
    """ctypes binding of tests/emu/libtsat_emu_aplqr.so, built here by the emulator's pattern rule"""

    def __init__(self, abi):
        self.lib = helpers.emu_library("libtsat_emu_aplqr.so")
        self.abi = abi

    def care6(self, A, G, Q, res_tol=RES_TOL):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        A, G, Q, P = f(A), f(G), f(Q), np.full((6, 6), np.nan)
        info = np.zeros(1, dtype=INFO_DTYPE)
        d = self.abi.as_dp
        assert self.lib.emu_care6(d(A), d(G), d(Q), C.c_double(res_tol), d(P), info.ctypes.data_as(C.c_void_p)) == 0
        return P, info[0]

    def gains(self, call):
        rc = self.lib.emu_aplqr_gains(*call.c_args())
        if rc != 0:
            raise RuntimeError(f"emu_aplqr_gains rc={rc}")
        return call.result()

    def gains_check(self, call):
        text = C.create_string_buffer(256)
        names = [n for n in GainsCall.FIELDS if n not in ("P_ss", "Gamma")]
        rc = self.lib.emu_aplqr_gains_check(*call.c_args(names), text, C.c_int32(256))
        return rc, text.value.decode()

    def run(self, batch, opts, x0_sim, Kg, rd, **kw):
        call = Call(self.abi, batch, opts, x0_sim, Kg, rd, **kw)
        rc = self.lib.emu_aplqr_ensemble(*call.c_args())
        if rc != 0:
            raise RuntimeError(f"emu_aplqr_ensemble rc={rc}")
        return call.result()

    def check(self, call):
        text = C.create_string_buffer(256)
        names = [n for n in FIELDS if n not in ("noise_id0", "X_sim", "n_clipped")]
        rc = self.lib.emu_aplqr_check(*call.c_args(names), text, C.c_int32(256))
        return rc, text.value.decode()
