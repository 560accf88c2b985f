// tsat_aplqr.hpp — the ASYMPTOTIC PERIODIC LQR on the dispersed plants (tsat_aplqr_gains, tsat_aplqr_ensemble of
// include/tortoise_hip.h): the model-based constant-P regulator the reference's comparison figure plots against the tracked plans,
// flown on the plants, limits, noise, gravity field and statistic of tsat_pd_ensemble. The reference's form of it:
//   magnetic_control_effectiveness, src/comparison/psiaki_dynamics.jl:75-98    the averaged control-effectiveness Gramian
//   Pss_psiaki, src/comparison/psiaki_dynamics.jl:101-125                       ControlSystems.care on the averaged system
//   nominal_input_psiaki, src/comparison/psiaki_dynamics.jl:127-143             u = -alpha inv(R) B' P x and its limit
// Deviations from those scripts (the law below is the one include/tortoise_hip.h defines):
//   - the goal there is fixed in the local-level frame and A carries orbit-rate and gravity-gradient terms; every goal of this ABI
//     is inertial (xf), so A is the double integrator [[0, I], [0, 0]] and the field is averaged in the goal's body frame;
//   - there B~ = sqrt(alpha) is handed to care; only B~ B~' = Gamma enters the equation, so no matrix square root is taken;
//   - the attitude error there is quaternion_euler(q); here the rotation vector to first order, 2 s e[1:4], with the PD law's
//     shortest-rotation sign s;
//   - inv(J) is the full inverse, not 1 / J_ii row scalings;
//   - the limit there scales back against U_max; here limit_mode 0 or 1 is tsat_pd_ensemble's, on the limits of the call.
//
// Synthesis, one wavefront per slew (aplqr_gains_wave):
//   beta_j = qrot(xf[3:7] / |xf[3:7]|, row j),  M = (1/n) sum_j beta_j beta_j'  over the window [avg_lo, avg_hi)
//   Gamma  = (1/n) sum_j B_j diag(1/rd) B_j',  B_j = -inv(J) hat(beta_j)   =   inv(J) S inv(J)',  S = hat(.) diag(1/rd) hat(.)'
//            summed, which is linear in the six entries of M: lanes stride over the rows, six wave_sum
//   P      : A'P + P A - P G P + Q = 0 with G = blockdiag(0, Gamma), Q = diag(qd)   (care6)
//   Kg     = alpha inv(J) P[3:6, 0:6]
// care6 is the matrix sign function of the Hamiltonian [[A, -G], [-Q, -A']]: Z <- (c Z + inv(Z) / c) / 2, c = |det Z|^(-1/12),
// the inverse by Gauss-Jordan with partial pivoting on [Z | I] in LDS, lane = column, |det| from the pivots. A lane finds the
// pivot row by reading the twelve entries of the column itself — broadcast reads, the same row in every lane, no reduction; the
// 1-norms of the stop rule are column sums under wave_max. Then P from [W12; W22 + I] P = -[W11 + I; W21] in the least-squares
// sense by modified Gram-Schmidt, lane = column (not by the normal equations, which square the condition of that matrix: 2.4e-7
// against 4.6e-16 with the 3U inertia), symmetrised, and the relative residual of the equation.
//
// Roll-out, per knot (aplqr_rollout): y, B from the Sensor exactly as pd_rollout takes them, xr the record or xf,
//   dw = y[0:3] - xr[0:3];  e = conj(xr[3:7]) (x) y[3:7];  s = (e0 < 0) ? -1 : 1;  theta = 2 s e[1:4]
//   v = Kg [theta; dw];  m[c] = -(1/rd[c]) (B x v)[c]  (a zero field row gives m = 0 by itself);  u_cmd = (ff ? U_k : 0) + m / u_scale
// and everything after u_cmd is pd_rollout's. The loop restates pd_rollout with the command lines replaced, so that pd_rollout and
// every kernel built on it keep their instruction streams. The launch block is PdArgs with GAIN = [T][AQGW]: Kg row-major (18),
// 1/rd (3), read by scalar loads once per wave.
#pragma once
#include <string>
#include <vector>
#include "tsat_pd.hpp"

#ifdef TSAT_EMU
#include <cmath>
#endif

namespace tsat {

constexpr int AQGW = 24;         // gains of a slew in the roll-out: Kg[3][6] row-major, 1/rd[3], 3 unused
constexpr int AQPW = 28;         // parameters of a slew in the synthesis (AQ_* below)
constexpr int AQ_QF = 0, AQ_JI = 4, AQ_QD = 13, AQ_IRD = 19, AQ_ALPHA = 22, AQ_LO = 23, AQ_HI = 24, AQ_BIDX = 25;
constexpr int CARE_MAX_ITER = 32;

// the LDS of the synthesis, in doubles: the augmented matrix of the eliminations (12 x 24), the scratch of the wave collectives,
// then A, G, Q and P (6 x 6 row-major each) of aplqr_gains_wave. 3968 bytes.
constexpr int AQL_AUG = 0, AQL_RED = 288, AQL_A = 352, AQL_G = 388, AQL_Q = 424, AQL_P = 460, AQL_REALS = 496;
#ifndef TSAT_EMU
__shared__ __align__(16) double tsat_aplqr_smem[AQL_REALS];
#endif
TSAT_DEV double* aplqr_lds() {
#ifdef TSAT_EMU
  return reinterpret_cast<double*>(tsat_emu::lds());
#else
  return tsat_aplqr_smem;
#endif
}
#ifdef TSAT_EMU
TSAT_DEV double aplqr_exp_(double a) { return std::exp(a); }
#else
TSAT_DEV double aplqr_exp_(double a) { return ::exp(a); }
#endif

// what care6 reports: the fields of tsat_aplqr_info
struct CareInfo {
  int status, iterations;
  double residual, pivot_min;
};

// Gauss-Jordan with partial pivoting on the n x w matrix m in LDS (row-major), lane = column: [Z | R] -> [. | inv(Z) R]; only the
// right block is meaningful afterwards. Called by the whole wave, m complete and synchronised; leaves it so. logdet takes the sum
// of log |pivot|, pmin the smallest |pivot|. false: a zero or non-finite pivot (wave-uniform; the matrix is left half reduced).
template <int n, int w>
TSAT_DEV bool gauss_jordan(double* m, double& logdet, double& pmin) {
  const int lane = TSAT_LANE();
  const bool mine = lane < w;
  const int c = mine ? lane : 0;
  TSAT_NO_UNROLL
  for (int p = 0; p < n; ++p) {
    int pr = p;
    double best = fabs_(m[p * w + p]);
    for (int r = 0; r < n; ++r) {
      const double v = fabs_(m[r * w + p]);
      if (r > p && v > best) { best = v; pr = r; }
    }
    if (!(best > 0.0) || !(best < inf_<double>())) return false;
    logdet = logdet + log_(best);
    pmin = best < pmin ? best : pmin;
    TSAT_SYNC_LDS();                                           // column p is read: the swap may write
    if (mine && pr != p) {
      const double a = m[p * w + c], b = m[pr * w + c];
      m[p * w + c] = b; m[pr * w + c] = a;
    }
    TSAT_SYNC_LDS();
    // the columns up to p are not read again after this step and stay as they are: column p keeps the factors while the others use them
    if (mine && c > p) {
      const double pc = m[p * w + c] * rcp_(m[p * w + p]);
      for (int r = 0; r < n; ++r) {
        if (r == p) m[r * w + c] = pc;
        else m[r * w + c] = fma_(-m[r * w + p], pc, m[r * w + c]);
      }
    }
    TSAT_SYNC_LDS();
  }
  return true;
}

// The stabilising solution of A'P + P A - P G P + Q = 0 for 6 x 6 row-major A, G, Q (any memory every lane can read; G and Q
// symmetric), by the whole wave; written for general A. P goes to Pout (6 x 6 row-major, LDS), zero-filled unless status == 0.
// lds: AQL_AUG and AQL_RED are used. status 0 ok; 1 not converged in CARE_MAX_ITER iterations; 2 a zero or non-finite pivot;
// 3 residual > res_tol, residual = |A'P + P A - P G P + Q|_F / (2 |A|_F |P|_F + |G|_F |P|_F^2 + |Q|_F). pivot_min is the smallest
// |pivot| of all eliminations of the call and of the diagonal of the triangular factor P is solved from.
TSAT_DEV CareInfo care6(const double* A, const double* G, const double* Q, double res_tol, double* lds, double* Pout) {
  const int lane = TSAT_LANE();
  double* aug = lds + AQL_AUG;
  double* red = lds + AQL_RED;
  const bool col = lane < 12;
  const int c = col ? lane : 11;
  CareInfo info{0, 0, 0.0, inf_<double>()};
  // column c of the Hamiltonian
  double z[12];
  for (int r = 0; r < 12; ++r) {
    const int i = r < 6 ? r : r - 6, j = c < 6 ? c : c - 6;
    z[r] = r < 6 ? (c < 6 ? A[i * 6 + j] : -G[i * 6 + j]) : (c < 6 ? -Q[i * 6 + j] : -A[j * 6 + i]);
  }
  bool converged = false;
  TSAT_NO_UNROLL
  for (int it = 1; it <= CARE_MAX_ITER; ++it) {
    info.iterations = it;                                      // the iterations begun: a failed elimination is counted
    if (lane < 24)
      for (int r = 0; r < 12; ++r) aug[r * 24 + lane] = col ? z[r] : ((lane - 12 == r) ? 1.0 : 0.0);
    TSAT_SYNC_LDS();
    double logdet = 0.0;
    if (!gauss_jordan<12, 24>(aug, logdet, info.pivot_min)) { info.status = 2; break; }
    const double cs = aplqr_exp_(logdet * (-1.0 / 12.0)), ics = rcp_(cs);
    double sd = 0.0, sz = 0.0;
    for (int r = 0; r < 12; ++r) {
      const double zn = 0.5 * fma_(cs, z[r], aug[r * 24 + 12 + c] * ics);
      sd = sd + fabs_(zn - z[r]);
      sz = sz + fabs_(zn);
      z[r] = zn;
    }
    TSAT_SYNC_LDS();                                           // the inverse is read: the next iteration may overwrite it
    const double nd = wave_max<double>(col ? sd : 0.0, red), nz = wave_max<double>(col ? sz : 0.0, red);
    if (nd <= 1e-14 * nz) { converged = true; break; }
  }
  if (info.status == 0 && !converged) info.status = 1;
  if (info.status == 0) {
    // [W12; W22 + I] P = -[W11 + I; W21] in the least-squares sense. The columns are already in the lanes: lane 6 + j holds column j
    // of M = [W12; W22 + I], lane c < 6 column c of the right side. Modified Gram-Schmidt over the twelve of them, the right side
    // carried along as further columns (which makes it as accurate as a Householder QR of M; the normal equations square the
    // condition of M, 4.5e8 with the 3U inertia), then R P = Q'rhs by back-substitution, a column of P per lane.
    double* qv = aug;                                          // q_j (12), |m_j|^2 at [12]
    double* Rm = aug + 16;                                     // R, 6 x 6 row-major
    double* ne = aug + 64;                                     // P before it is symmetrised, 6 x 6 row-major
    for (int r = 0; r < 12; ++r) {
      const double v = z[r] + ((r == c) ? 1.0 : 0.0);
      z[r] = c < 6 ? -v : v;
    }
    double y[6];
    for (int j = 0; j < 6; ++j) {
      if (lane == 6 + j) {
        double s2 = 0.0;
        for (int r = 0; r < 12; ++r) s2 = fma_(z[r], z[r], s2);
        const double rn = rsqrt_<double>(s2);
        for (int r = 0; r < 12; ++r) qv[r] = z[r] * rn;
        qv[12] = s2;
        Rm[j * 6 + j] = s2 * rn;
      }
      TSAT_SYNC_LDS();
      const double s2 = qv[12];
      if (!(s2 > 0.0) || !(s2 < inf_<double>())) info.status = 2;          // wave-uniform
      double d = 0.0;
      for (int r = 0; r < 12; ++r) d = fma_(qv[r], z[r], d);
      if (col && lane != 6 + j)
        for (int r = 0; r < 12; ++r) z[r] = fma_(-d, qv[r], z[r]);
      y[j] = d;
      if (lane > 6 + j && col) Rm[j * 6 + (lane - 6)] = d;
      TSAT_SYNC_LDS();
    }
    if (info.status == 0) {
      for (int j = 0; j < 6; ++j) {
        const double rjj = Rm[j * 6 + j];
        info.pivot_min = rjj < info.pivot_min ? rjj : info.pivot_min;
      }
      double xs[6];
      for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v = fma_(-Rm[i * 6 + k], xs[k], v);
        xs[i] = v * rcp_(Rm[i * 6 + i]);
      }
      if (lane < 6)
        for (int i = 0; i < 6; ++i) ne[i * 6 + lane] = xs[i];
      TSAT_SYNC_LDS();
    }
    if (info.status == 0) {
      const int e = lane < 36 ? lane : 35, i = e / 6, j = e - 6 * i;
      const double pij = 0.5 * (ne[i * 6 + j] + ne[j * 6 + i]);
      if (lane < 36) Pout[e] = pij;
      TSAT_SYNC_LDS();
      // T1 = P G (at aug: R and the columns of P are read), then R = A'P + P A - T1 P + Q
      double t1 = 0.0;
      for (int k = 0; k < 6; ++k) t1 = fma_(Pout[i * 6 + k], G[k * 6 + j], t1);
      if (lane < 36) aug[e] = t1;
      TSAT_SYNC_LDS();
      double rij = Q[e];
      for (int k = 0; k < 6; ++k) rij = fma_(A[k * 6 + i], Pout[k * 6 + j], rij);
      for (int k = 0; k < 6; ++k) rij = fma_(Pout[i * 6 + k], A[k * 6 + j], rij);
      for (int k = 0; k < 6; ++k) rij = fma_(-aug[i * 6 + k], Pout[k * 6 + j], rij);
      const bool on = lane < 36;
      const double rr = wave_sum<double>(on ? rij * rij : 0.0, red), aa = wave_sum<double>(on ? A[e] * A[e] : 0.0, red);
      const double pp = wave_sum<double>(on ? pij * pij : 0.0, red), gg = wave_sum<double>(on ? G[e] * G[e] : 0.0, red);
      const double qq = wave_sum<double>(on ? Q[e] * Q[e] : 0.0, red);
      info.residual = sqrt_(rr) / (2.0 * sqrt_(aa) * sqrt_(pp) + sqrt_(gg) * pp + sqrt_(qq));
      if (!(info.residual <= res_tol)) info.status = 3;
    }
  }
  if (info.status != 0) {
    TSAT_SYNC_LDS();
    if (lane < 36) Pout[lane] = 0.0;
  }
  TSAT_SYNC_LDS();
  return info;
}

// the launch block of the synthesis
struct AplqrGainArgs {
  const double* GP;      // [T][AQPW]: xf[3:7], inv(J) row-major, qd[6], 1/rd[3], alpha, avg_lo, avg_hi, btab_idx (the integers as doubles)
  const double* B;       // [n_btab][n_tab][3] the field tables as the caller gives them
  int n_tab;
  double res_tol;
  double* Kg;            // [T][18], entry (c, j) at j * 3 + c: 3 x 6 x T of the ABI
  double* Pss;           // [T][36]
  double* Gam;           // [T][9]
  void* info;            // [T] tsat_aplqr_info
};

// one wavefront per slew
TSAT_DEV void aplqr_gains_wave(const AplqrGainArgs& a, int traj) {
  const int lane = TSAT_LANE();
  double* lds = aplqr_lds();
  double* red = lds + AQL_RED;
  const TSAT_CONSTMEM double* gp = (const TSAT_CONSTMEM double*)(a.GP + (size_t)traj * AQPW);
  const int lo = (int)gp[AQ_LO], hi = (int)gp[AQ_HI], n = hi - lo;
  const TSAT_GLOBAL double* bt = (const TSAT_GLOBAL double*)(a.B + (size_t)(int)gp[AQ_BIDX] * a.n_tab * 3);
  double Ji[9], ird[3];
  for (int i = 0; i < 9; ++i) Ji[i] = gp[AQ_JI + i];
  for (int i = 0; i < 3; ++i) ird[i] = gp[AQ_IRD + i];
  // the second moment of the field in the goal's body frame: lanes stride over the window's rows
  double x[7] = {0, 0, 0, gp[AQ_QF], gp[AQ_QF + 1], gp[AQ_QF + 2], gp[AQ_QF + 3]};
  double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0;
  TrueState goal;
  for (int j = lo + lane; j < hi; j += WAVE) {
    const double b0[3] = {bt[(size_t)j * 3], bt[(size_t)j * 3 + 1], bt[(size_t)j * 3 + 2]};
    double b[3];
    goal.field<double>(0, 0, false, x, b0, b);
    m00 = fma_(b[0], b[0], m00); m01 = fma_(b[0], b[1], m01); m02 = fma_(b[0], b[2], m02);
    m11 = fma_(b[1], b[1], m11); m12 = fma_(b[1], b[2], m12); m22 = fma_(b[2], b[2], m22);
  }
  const double in = rcp_((double)n);
  m00 = wave_sum<double>(m00, red) * in; m01 = wave_sum<double>(m01, red) * in; m02 = wave_sum<double>(m02, red) * in;
  m11 = wave_sum<double>(m11, red) * in; m12 = wave_sum<double>(m12, red) * in; m22 = wave_sum<double>(m22, red) * in;
  // S = mean of hat(beta) diag(1/rd) hat(beta)', then Gamma = inv(J) S inv(J)'
  double S[9];
  S[0] = ird[1] * m22 + ird[2] * m11; S[4] = ird[0] * m22 + ird[2] * m00; S[8] = ird[0] * m11 + ird[1] * m00;
  S[1] = S[3] = -(ird[2] * m01); S[2] = S[6] = -(ird[1] * m02); S[5] = S[7] = -(ird[0] * m12);
  double JS[9], Gm[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) JS[3 * i + j] = dot3_(Ji[3 * i], S[j], Ji[3 * i + 1], S[3 + j], Ji[3 * i + 2], S[6 + j]);
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) Gm[3 * i + j] = Gm[3 * j + i] = dot3_(JS[3 * i], Ji[3 * j], JS[3 * i + 1], Ji[3 * j + 1], JS[3 * i + 2], Ji[3 * j + 2]);
  // A, G, Q to LDS
  if (lane < 36) {
    const int i = lane / 6, j = lane - 6 * i;
    lds[AQL_A + lane] = (i < 3 && j == i + 3) ? 1.0 : 0.0;
    double g = 0.0;
    for (int e = 0; e < 9; ++e) g = (i >= 3 && j >= 3 && 3 * (i - 3) + (j - 3) == e) ? Gm[e] : g;
    lds[AQL_G + lane] = g;
    double q = 0.0;
    for (int e = 0; e < 6; ++e) q = (i == j && i == e) ? gp[AQ_QD + e] : q;
    lds[AQL_Q + lane] = q;
  }
  TSAT_SYNC_LDS();
  const CareInfo ci = care6(lds + AQL_A, lds + AQL_G, lds + AQL_Q, a.res_tol, lds, lds + AQL_P);
  // Kg = alpha inv(J) P[3:6, 0:6] (zero with P on a failed solve)
  const double alpha = gp[AQ_ALPHA];
  if (lane < 18) {
    const int cc = lane / 6, j = lane - 6 * cc;
    double v = 0.0;
    for (int r = 0; r < 3; ++r) {                               // every row of inv(J) by a constant index, the lane's own selected
      const double vr = dot3_(Ji[3 * r], lds[AQL_P + 18 + j], Ji[3 * r + 1], lds[AQL_P + 24 + j], Ji[3 * r + 2], lds[AQL_P + 30 + j]);
      v = (cc == r) ? vr : v;
    }
    a.Kg[(size_t)traj * 18 + j * 3 + cc] = alpha * v;
  }
  if (lane < 36) a.Pss[(size_t)traj * 36 + lane] = lds[AQL_P + lane];
  if (lane < 9) {
    double g = Gm[0];
    for (int e = 1; e < 9; ++e) g = (lane == e) ? Gm[e] : g;
    a.Gam[(size_t)traj * 9 + lane] = g;
  }
  if (lane == 0) {
    tsat_aplqr_info* out = reinterpret_cast<tsat_aplqr_info*>(a.info) + traj;
    out->status = ci.status; out->iterations = ci.iterations; out->residual = ci.residual; out->pivot_min = ci.pivot_min;
  }
}

template <typename real, typename Plant, typename Sensor = TrueState>
TSAT_DEV void aplqr_rollout(const PdArgs<real>& pa, Plant& plant, int traj, int wave, Sensor sensor = Sensor()) {
  constexpr int DIAGJ = Plant::DIAGJ;
  const EnsArgs<real>& a = pa.d.e;
  const int lane = TSAT_LANE();
  const int NS = a.N, n_tab = a.n_tab, M = a.M;
  const int N = a.nk ? a.nk[traj] : a.N;                       // own horizon; slabs keep the stride NS
  const int R = M + 1;
  // lanes past the last realisation compute a duplicate of it and store nothing (no divergent exit)
  const int r_own = wave * WAVE + lane;
  const bool live = r_own < R;
  const int r = live ? r_own : R - 1;
  const bool noisy = r < M;
  const TSAT_CONSTMEM real* Pc = (const TSAT_CONSTMEM real*)(a.P + (size_t)traj * PSTRIDE);
  const TSAT_CONSTMEM real* xu = a.XUR ? (const TSAT_CONSTMEM real*)(a.XUR + (size_t)traj * NS * XUW) : nullptr;
  const TSAT_CONSTMEM real* gn = (const TSAT_CONSTMEM real*)(pa.GAIN + (size_t)traj * AQGW);
  const TSAT_CONSTMEM real* bt = (const TSAT_CONSTMEM real*)(a.BT + (size_t)a.bidx[traj] * n_tab * 4);
  const Traj<real> tr = ensemble_traj<real>(Pc, a.us, N, n_tab);
  plant.load(tr, traj, r);
  sensor.load(traj, r);
  const Traj<real>& tp = plant.traj(tr);                       // what dyn_sim_h reads
  const long long gid = (a.nid0 ? a.nid0[traj] : (long long)traj * (long long)M) + (long long)r;
  TSAT_GLOBAL real* xs = (a.XS && live && noisy) ? (TSAT_GLOBAL real*)(a.XS + ((size_t)traj * M + r) * NS * 7) : nullptr;
  real x[7];
  if (noisy) {
    const TSAT_GLOBAL real* x0 = (const TSAT_GLOBAL real*)(a.X0 + ((size_t)traj * M + r) * 7);
    for (int i = 0; i < 7; ++i) x[i] = x0[i];
  } else {
    const TSAT_CONSTMEM real* x0 = (const TSAT_CONSTMEM real*)(pa.X0N + (size_t)traj * 7);
    for (int i = 0; i < 7; ++i) x[i] = x0[i];
  }
  const real cs = control_scale<real, DIAGJ>(tr);
  // the law's constants, once per wave: the gain, 1 / rd, 1 / u_scale, and for limit_mode 1 the reciprocals of the limits
  real kg[18], ird[3], ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};
  for (int i = 0; i < 18; ++i) kg[i] = gn[i];
  for (int c = 0; c < 3; ++c) ird[c] = gn[18 + c];
  const real ius = rcp_(a.us);
  const int ff = pa.feedforward, mode1 = pa.limit_mode;
  if (mode1)
    for (int c = 0; c < 3; ++c) { ilo[c] = rcp_(plant.lo[c]); ihi[c] = rcp_(plant.hi[c]); }
  int first = 0;                                               // the statistic, evaluated while the roll-out runs
  TSAT_NO_UNROLL
  for (int k = 0; k < N - 1; ++k) {
    {  // sample j = k + 1 (1-based): src/monte_carlo.jl:242-262
      const real wj = sqrt_(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      if (first == 0 && k + 1 > a.min_steps && wj < a.w_tol) {
        if (ensemble_angle<real>(tr, x) < a.ang_tol) first = k + 1;
      }
    }
    if (xs)
      for (int i = 0; i < 7; ++i) xs[(size_t)k * 7 + i] = x[i];
    real xr[7], uc[3] = {0, 0, 0};
    if (xu) {
      const TSAT_CONSTMEM real* rec = xu + (size_t)k * XUW;
      for (int i = 0; i < 7; ++i) xr[i] = rec[i];
      if (ff)
        for (int c = 0; c < 3; ++c) uc[c] = rec[7 + c];
    } else {
      for (int i = 0; i < 7; ++i) xr[i] = tr.xf[i];
    }
    // rows at tau, tau + dtau/2, tau + dtau: wave-uniform indices, said so (the clock is fp64 arithmetic on the vector unit)
    const TSAT_CONSTMEM real* p0 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.0)) * 4;
    const TSAT_CONSTMEM real* p1 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.5)) * 4;
    const TSAT_CONSTMEM real* p2 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 1.0)) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    {  // the law, on what the sensor gives of x: y for the errors, B for the body-frame field
      real z[6], v[3], y[7], B[3];
      sensor.state(gid, k, noisy, x, y);
      {
        // e = q_ref^-1 (x) q_sim as pd_rollout forms it; theta = 2 s e[1:4], the rotation vector to first order
        const real s1 = xr[3], a1 = -xr[4], a2 = -xr[5], a3 = -xr[6];
        const real e0 = s1 * y[3] - (a1 * y[4] + a2 * y[5] + a3 * y[6]);
        const real e1 = s1 * y[4] + y[3] * a1 + (a2 * y[6] - a3 * y[5]);
        const real e2 = s1 * y[5] + y[3] * a2 + (a3 * y[4] - a1 * y[6]);
        const real e3 = s1 * y[6] + y[3] * a3 + (a1 * y[5] - a2 * y[4]);
        const bool neg = e0 < 0;                               // shortest rotation
        z[0] = 2 * (neg ? -e1 : e1); z[1] = 2 * (neg ? -e2 : e2); z[2] = 2 * (neg ? -e3 : e3);
        z[3] = y[0] - xr[0]; z[4] = y[1] - xr[1]; z[5] = y[2] - xr[2];
      }
      for (int c = 0; c < 3; ++c) {
        real s = kg[6 * c] * z[0];
        for (int j = 1; j < 6; ++j) s = fma_(kg[6 * c + j], z[j], s);
        v[c] = s;
      }
      sensor.field(gid, k, noisy, x, b0, B);                   // TrueState: qrot(q, b0)
      // m = -diag(1/rd) (B x v): no reciprocal in the knot, a zero row gives no dipole by itself
      uc[0] = uc[0] - (ird[0] * dmm_(B[1], v[2], B[2], v[1])) * ius;
      uc[1] = uc[1] - (ird[1] * dmm_(B[2], v[0], B[0], v[2])) * ius;
      uc[2] = uc[2] - (ird[2] * dmm_(B[0], v[1], B[1], v[0])) * ius;
    }
    real us[3];
    if (mode1) {
      // direction-preserving: the largest ratio of a component to the limit on its side
      real beta = 0;
      for (int c = 0; c < 3; ++c) {
        const real rc = uc[c] > 0 ? uc[c] * ihi[c] : (uc[c] < 0 ? uc[c] * ilo[c] : (real)0);
        beta = rc > beta ? rc : beta;
      }
      if (beta > 1) {
        const real ib = rcp_(beta);
        for (int c = 0; c < 3; ++c) uc[c] = uc[c] * ib;
        plant.hit = 1;
      }
    } else {
      for (int c = 0; c < 3; ++c) uc[c] = plant.command(c, uc[c], cs);
    }
    sensor.commanded(k, uc);                                   // as pd_rollout hands it over
    plant.actuate(uc, cs, us);
    real k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
    for (int i = 0; i < 9; ++i) nz[i] = 0;
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 0, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, x, us, b0, noisy, nz, k1);
    plant.disturb(tr, k, 0.0, x, k1);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 1, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b1, noisy, nz, k2);
    plant.disturb(tr, k, 0.5, t, k2);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 2, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b1, noisy, nz, k3);
    plant.disturb(tr, k, 0.5, t, k3);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 3, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b2, noisy, nz, k4);
    plant.disturb(tr, k, 1.0, t, k4);
    for (int i = 0; i < 7; ++i) x[i] = x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (real)(1.0 / 6.0);
  }
  // last sample j = N
  const real wN = sqrt_(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const real angN = ensemble_angle<real>(tr, x);
  if (first == 0 && N > a.min_steps && wN < a.w_tol && angN < a.ang_tol) first = N;
  if (xs)
    for (int i = 0; i < 7; ++i) xs[(size_t)(N - 1) * 7 + i] = x[i];
  if (live) {
    tsat_tvlqr_stats st;
    st.slew_index = first;
    st.failed = first ? 0 : 1;
    st.slew_time = (double)tr.h * (first ? (double)first : (double)N);
    st.final_w_norm = (double)wN;
    st.final_angle = (double)angN;
    if (noisy) {
      a.stats[(size_t)traj * M + r] = st;
      plant.store((size_t)traj * M + r);
    } else {
      a.stats_nom[traj] = st;
    }
  }
}

// Everything tsat_aplqr_ensemble rejects besides a null handle, before anything is allocated or launched: "" or the reason. The
// checks of tsat_pd_ensemble in check_pd's order (its own gains apart), then the law's own.
inline std::string check_aplqr(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                               const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                               const double* dt, const double* Jmat, const double* Kg, const double* rd, int32_t feedforward,
                               int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int32_t* n_knots, const double* plant,
                               const double* sat_lo, const double* sat_hi, const void* stats, const double* summary,
                               const void* stats_nominal, const double* Rtab, double gm) {
  // check_pd reads its gains only after it has accepted T: zeros of that size stand in for them
  const std::vector<double> zero((T >= 1 && T <= 0x7fffffff) ? 3 * (size_t)T : 0, 0.0);
  const std::string why = check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, zero.data(), zero.data(), feedforward,
                                   limit_mode, x0_sim, x0_nom, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm);
  if (!why.empty()) return why;
  if (!Kg || !rd) return "null Kg or rd";
  for (int64_t i = 0; i < 18 * T; ++i)
    if (!std::isfinite(Kg[i])) return "Kg must be finite (t = " + std::to_string(i / 18) + ")";
  for (int64_t i = 0; i < 3 * T; ++i)
    if (!std::isfinite(rd[i]) || !(rd[i] > 0.0)) return "rd must be finite and > 0 (t = " + std::to_string(i / 3) + ")";
  return "";
}

// ... and tsat_aplqr_gains
inline std::string check_aplqr_gains(int64_t T, int64_t n_btab, int32_t n_tab, const double* xf, const double* Btab, const int32_t* btab_idx,
                                     const int32_t* avg_lo, const int32_t* avg_hi, const double* Jmat, const double* qd, const double* rd,
                                     const double* alpha, double res_tol, const double* Kg, const void* info) {
  if (T < 1 || T > 0x7fffffff || n_btab < 1 || n_tab < 1) return "bad batch dimensions";
  if (!xf || !Btab || !Jmat || !qd || !rd || !alpha || !Kg || !info) return "null array";
  if ((avg_lo == nullptr) != (avg_hi == nullptr)) return "exactly one of avg_lo / avg_hi is NULL";
  if (!btab_idx && n_btab != T) return "btab_idx is NULL but n_btab != T";
  if (!(res_tol > 0.0)) return "res_tol must be > 0";
  for (int64_t t = 0; t < T; ++t) {
    const std::string at = " (t = " + std::to_string(t) + ")";
    const int64_t v = btab_idx ? btab_idx[t] : t;
    if (v < 0 || v >= n_btab) return "btab_idx out of range";
    if (avg_lo && !(avg_lo[t] >= 0 && avg_lo[t] < avg_hi[t] && avg_hi[t] <= n_tab))
      return "the averaging window must satisfy 0 <= avg_lo < avg_hi <= n_tab" + at;
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(qd[6 * t + i]) || !(qd[6 * t + i] > 0.0)) return "qd must be finite and > 0" + at;
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(rd[3 * t + i]) || !(rd[3 * t + i] > 0.0)) return "rd must be finite and > 0" + at;
    if (!std::isfinite(alpha[t]) || alpha[t] < 0.0) return "alpha must be finite and >= 0" + at;
    const double* q = xf + 7 * t + 3;
    const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!std::isfinite(qq) || !(qq > 0.0)) return "xf[3:7] must be a finite, non-zero quaternion" + at;
    const double* J = Jmat + 9 * t;
    double nrm = 0;
    for (int i = 0; i < 9; ++i) {
      if (!std::isfinite(J[i])) return "Jmat must be finite" + at;
      nrm = std::fmax(nrm, std::fabs(J[i]));
    }
    const double det = J[0] * (J[4] * J[8] - J[7] * J[5]) - J[3] * (J[1] * J[8] - J[7] * J[2]) + J[6] * (J[1] * J[5] - J[4] * J[2]);
    if (!(std::fabs(det) > 1e-12 * nrm * nrm * nrm)) return "Jmat is singular" + at;
  }
  return "";
}

// the parameter records of the synthesis, [T][AQPW]
inline std::vector<double> pack_aplqr_gains(int64_t T, int32_t n_tab, const double* xf, const int32_t* btab_idx, const int32_t* avg_lo,
                                            const int32_t* avg_hi, const double* Jmat, const double* qd, const double* rd,
                                            const double* alpha) {
  std::vector<double> gp((size_t)T * AQPW, 0.0);
  for (int64_t t = 0; t < T; ++t) {
    double* p = gp.data() + (size_t)t * AQPW;
    double Jr[9];
    for (int i = 0; i < 4; ++i) p[AQ_QF + i] = xf[7 * t + 3 + i];
    inertia_inverse_rm(Jmat + 9 * t, Jr, p + AQ_JI);
    for (int i = 0; i < 6; ++i) p[AQ_QD + i] = qd[6 * t + i];
    for (int i = 0; i < 3; ++i) p[AQ_IRD + i] = 1.0 / rd[3 * t + i];
    p[AQ_ALPHA] = alpha[t];
    p[AQ_LO] = avg_lo ? (double)avg_lo[t] : 0.0;
    p[AQ_HI] = avg_hi ? (double)avg_hi[t] : (double)n_tab;
    p[AQ_BIDX] = btab_idx ? (double)btab_idx[t] : (double)t;
  }
  return gp;
}

// the gain records of the roll-out, [T][AQGW], from the ABI's Kg 3 x 6 x T and rd 3 x T
inline std::vector<double> pack_aplqr_law(int64_t T, const double* Kg, const double* rd) {
  std::vector<double> g((size_t)T * AQGW, 0.0);
  for (int64_t t = 0; t < T; ++t) {
    for (int c = 0; c < 3; ++c) {
      for (int j = 0; j < 6; ++j) g[(size_t)t * AQGW + 6 * c + j] = Kg[18 * t + 3 * j + c];
      g[(size_t)t * AQGW + 18 + c] = 1.0 / rd[3 * t + c];
    }
  }
  return g;
}

// Rtab == null at the call: the plants of tsat_tvlqr_ensemble_dispersed ...
template <typename real>
TSAT_DEV void aplqr_wave(const PdArgs<real>& pa, int traj, int wave) {
  DispersedPlant<real> plant(pa.d);
  aplqr_rollout<real>(pa, plant, traj, wave);
}

// ... otherwise those of tsat_tvlqr_ensemble_gg, whatever gm is
template <typename real>
TSAT_DEV void aplqr_gg_wave(const PdArgs<real>& pa, int traj, int wave) {
  const GgEnsArgs<real> g{pa.d, pa.GT};
  GgPlant<real> plant(g);
  aplqr_rollout<real>(pa, plant, traj, wave);
}

}  // namespace tsat

// the launchers (tsat_kernels_aplqr.hip), called by the host code of the entry points (tsat_kernels_ensemble.hip)
#ifndef TSAT_EMU
hipError_t tsat_launch_aplqr_gains(const tsat::AplqrGainArgs& a, int64_t T, hipStream_t stream);
hipError_t tsat_launch_aplqr(const tsat::PdArgs<double>& a, int waves, hipStream_t stream);
#endif
