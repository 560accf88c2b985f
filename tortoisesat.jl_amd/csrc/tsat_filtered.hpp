// tsat_filtered.hpp — a multiplicative EKF between sensor and law in the ensembles (tsat_tvlqr_ensemble_filtered,
// tsat_pd_ensemble_filtered, include/tortoise_hip.h): the calls of tsat_sensed.hpp with the standard six-state filter — attitude
// error and gyro bias, propagated by the gyro, updated by the attitude measurement — between the measurement and the command.
//
// WHAT IT REMOVES AND WHAT IT DOES NOT. The filter removes attitude-sensor noise and estimates the gyro bias.
// It does NOT smooth white gyro noise: the rate the law sees is w_m - b^, the gyro sample itself less the bias estimate, so its
// error stays that of one gyro sample (a numpy run of the recursion at dt = 0.2 s, sigma_gyro = 0.38 deg/s, sigma_att = 1 deg, a 2e-3 rad/s bias, 400
// knots: attitude error 1.74 deg raw -> 0.48 deg filtered, bias error 3.5e-3 -> 0.7e-3 rad/s, rate error 1.20e-2 -> 1.15e-2 rad/s).
//
// Filtered is the third `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState and Sensed:
// it OWNS a Sensed, runs over the samples m_j = (w_m, q_m) that Sensed::state produces, and hands the law its estimate. `field`
// passes through to the inner Sensed: the PD law's magnetometer reading is not filtered. The loops, the plants, the limit rules
// and the statistic stay the parents' own code; neither roll-out is edited. The sensor type knows (traj, r, k), so it writes its
// own outputs — X_hat row k and, at the last knot that commands, filt_final — from inside state(), for realisations r < M.
//
// State of a lane: q^ (4, unit, scalar first), b^ (3), w^ (3) and the 6 x 6 covariance as blocks A (theta theta), B (theta b),
// D (b b), A and D as upper triangles (00 01 02 11 12 22): 6 + 9 + 6 = 21 values, P symmetric by construction. One flat record of
// FLW = 31 values (FilterState) with load / save, which the held re-planning loop carries between launches (tsat_mpc_filtered.hpp).
//
// h is the trajectory's dt from the parameter record (as ensemble_traj reads it), dq(.) the rotation-vector quaternion of
// tsat_sensed.hpp including its th == 0 select, (x) the quaternion product in the operand order of Sensed::state.
//   first sample m_0:  q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I
//   step on sample m_j, j >= 1:
//     1. phi = h w^, d = dq(phi), q- = q^ (x) d;  C = I + 2 d0 [v]x + 2 [v]x^2 with v = d[1:4];  Phi = C^T
//     2. A- = Phi A Phi^T - h (Phi B + (Phi B)^T) + h^2 D + (sigma_v h)^2 I;  B- = Phi B - h D;  D- = D + sigma_u^2 I
//     3. e = conj(q-) (x) (q_m / |q_m|);  s = (e0 < 0 ? -1 : 1);  z = 2 s e[1:4]
//     4. S = A- + sigma_a^2 I (3 x 3, positive definite; inverted by cofactors and one reciprocal);
//        Ktheta = A- S^-1, Kb = B-^T S^-1;  dtheta = Ktheta z, db = Kb z
//     5. q^ = (q- (x) [1; dtheta / 2]) normalised;  b^ <- b^ + db;  w^ = w_m - b^
//     6. P <- P- - K S K^T by blocks, the upper triangles of A and D only
//   what the law sees at knot k — latency 0: the filter is at sample k, y_k = (w^_k, q^_k). Latency 1: y_0 = (w^_0, q^_0); for
//   k >= 1 the filter is at sample k - 1 and y_k = (w^_{k-1}, q^_{k-1} (x) dq(h w^_{k-1})), the estimate predicted across the delay
//   (step 1's q- of the next step). The inner Sensed at latency 1 hands m_0 over twice, at k = 0 and k = 1: the second makes no step.
// The noise-free realisation (slot M) flies the ideal sensor through the same filter. Latency stays a uniform branch, as do
// k == 0 and the skipped step (k is the loop counter); nothing asks whether a sigma is zero.
#pragma once
#include <string>
#include "tsat_sensed.hpp"

namespace tsat {

constexpr int FLW = 31;          // the filter's state of a lane: q^[4], b^[3], w^[3], A[6], B[9], D[6]
constexpr int FFW = TSAT_FILTER_W;   // filt_final of a realisation: b^[3], sqrt(diag A)[3], sqrt(diag D)[3]

template <typename real>
struct FiltArgs {
  SensArgs<real> s;      // the inner sensor's block
  const real* P;         // [T][PSTRIDE] parameter records: h = P[P_DT]
  const int* nk;         // [T] per-slew knot counts or null (all N)
  int M, N;              // realisations of a slew; slab stride of XH
  real sv, su, sa;       // sigma_v, sigma_u, sigma_a
  real p0a, p0b;         // p0_att, p0_bias
  real* XH;              // [T][M][N][7] what the law saw, or null
  real* FF;              // [T][M][FFW] b^, sqrt(diag A), sqrt(diag D) after the last sample processed, or null
};

template <typename real>
struct FilteredTvArgs {
  GgEnsArgs<real> g;     // as SensedTvArgs
  FiltArgs<real> f;
};

template <typename real>
struct FilteredPdArgs {
  PdArgs<real> p;        // as SensedPdArgs
  FiltArgs<real> f;
};

// the launch block of the filter around that of its sensor (host)
inline FiltArgs<double> filt_args(const tsat_filter_options& f, const SensArgs<double>& sa, const EnsArgs<double>& e, double* XH, double* FF) {
  FiltArgs<double> a;
  a.s = sa; a.P = e.P; a.nk = e.nk; a.M = e.M; a.N = e.N;
  a.sv = f.sigma_v; a.su = f.sigma_u; a.sa = f.sigma_a; a.p0a = f.p0_att; a.p0b = f.p0_bias;
  a.XH = XH; a.FF = FF;
  return a;
}

// the flat record
template <typename real>
struct FilterState {
  real q[4], b[3], w[3], A[6], B[9], D[6];
  TSAT_DEV void load(const real* p, size_t stride = 1) {
    int o = 0;
    for (int i = 0; i < 4; ++i) q[i] = p[(size_t)(o++) * stride];
    for (int i = 0; i < 3; ++i) b[i] = p[(size_t)(o++) * stride];
    for (int i = 0; i < 3; ++i) w[i] = p[(size_t)(o++) * stride];
    for (int i = 0; i < 6; ++i) A[i] = p[(size_t)(o++) * stride];
    for (int i = 0; i < 9; ++i) B[i] = p[(size_t)(o++) * stride];
    for (int i = 0; i < 6; ++i) D[i] = p[(size_t)(o++) * stride];
  }
  TSAT_DEV void save(real* p, size_t stride = 1) const {
    int o = 0;
    for (int i = 0; i < 4; ++i) p[(size_t)(o++) * stride] = q[i];
    for (int i = 0; i < 3; ++i) p[(size_t)(o++) * stride] = b[i];
    for (int i = 0; i < 3; ++i) p[(size_t)(o++) * stride] = w[i];
    for (int i = 0; i < 6; ++i) p[(size_t)(o++) * stride] = A[i];
    for (int i = 0; i < 9; ++i) p[(size_t)(o++) * stride] = B[i];
    for (int i = 0; i < 6; ++i) p[(size_t)(o++) * stride] = D[i];
  }
};

// qmult(a, b), the form of Sensed::state
template <typename real>
TSAT_DEV void filt_qmult(const real a[4], const real b[4], real r[4]) {
  r[0] = a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]);
  r[1] = a[0] * b[1] + b[0] * a[1] + (a[2] * b[3] - a[3] * b[2]);
  r[2] = a[0] * b[2] + b[0] * a[2] + (a[3] * b[1] - a[1] * b[3]);
  r[3] = a[0] * b[3] + b[0] * a[3] + (a[1] * b[2] - a[2] * b[1]);
}

// dq(phi) of tsat_sensed.hpp
template <typename real>
TSAT_DEV void filt_dq(const real phi[3], real d[4]) {
  const real th = sqrt_(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
  const real sr = sin_((real)0.5 * th) / th;
  const real sh = (th == 0) ? (real)0.5 : sr;
  d[0] = cos_((real)0.5 * th);
  d[1] = phi[0] * sh; d[2] = phi[1] * sh; d[3] = phi[2] * sh;
}

// upper triangle (00 01 02 11 12 22) <-> full symmetric 3 x 3, row-major
template <typename real>
TSAT_DEV void filt_sym(const real u[6], real m[9]) {
  m[0] = u[0]; m[1] = u[1]; m[2] = u[2];
  m[3] = u[1]; m[4] = u[3]; m[5] = u[4];
  m[6] = u[2]; m[7] = u[4]; m[8] = u[5];
}

template <typename real>
struct Filtered {
  const FiltArgs<real>& f;
  Sensed<real> in;
  FilterState<real> st;
  real h;
  int nt;                                                      // the slew's own knot count
  TSAT_GLOBAL real* xh;                                        // this realisation's rows of XH / record of FF, or null
  TSAT_GLOBAL real* ff;
  TSAT_DEV explicit Filtered(const FiltArgs<real>& f_) : f(f_), in(f_.s) {}
  TSAT_DEV void load(int traj, int r) {
    in.load(traj, r);
    const TSAT_CONSTMEM real* Pc = (const TSAT_CONSTMEM real*)(f.P + (size_t)traj * PSTRIDE);
    h = Pc[P_DT];
    nt = f.nk ? f.nk[traj] : f.N;
    const bool own = r < f.M;
    xh = (f.XH && own) ? (TSAT_GLOBAL real*)(f.XH + ((size_t)traj * f.M + r) * f.N * 7) : nullptr;
    ff = (f.FF && own) ? (TSAT_GLOBAL real*)(f.FF + ((size_t)traj * f.M + r) * FFW) : nullptr;
    for (int i = 0; i < 4; ++i) st.q[i] = 0;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = 0; }
    for (int i = 0; i < 6; ++i) { st.A[i] = 0; st.D[i] = 0; }
    for (int i = 0; i < 9; ++i) st.B[i] = 0;
  }
  TSAT_DEV void commanded(int, const real*) {}                 // the gyro propagates this filter, not the model
  TSAT_DEV void first(const real m[7]) {
    const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
    for (int i = 0; i < 4; ++i) st.q[i] = m[3 + i] * rn;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = m[i]; }
    const real a0 = f.p0a * f.p0a, d0 = f.p0b * f.p0b;
    st.A[0] = a0; st.A[1] = 0; st.A[2] = 0; st.A[3] = a0; st.A[4] = 0; st.A[5] = a0;
    st.D[0] = d0; st.D[1] = 0; st.D[2] = 0; st.D[3] = d0; st.D[4] = 0; st.D[5] = d0;
    for (int i = 0; i < 9; ++i) st.B[i] = 0;
  }
  TSAT_DEV void step(const real m[7]) {
    // 1. propagate the attitude by the gyro; Phi = C^T = I - 2 d0 [v]x + 2 (v v^T - |v|^2 I)
    real phi[3], d[4], qm[4];
    for (int i = 0; i < 3; ++i) phi[i] = h * st.w[i];
    filt_dq<real>(phi, d);
    filt_qmult<real>(st.q, d, qm);
    real Ph[9];
    {
      const real v1 = d[1], v2 = d[2], v3 = d[3], vv = v1 * v1 + v2 * v2 + v3 * v3, c = 2 * d[0];
      Ph[0] = 1 + 2 * (v1 * v1 - vv); Ph[1] = 2 * v1 * v2 + c * v3;    Ph[2] = 2 * v1 * v3 - c * v2;
      Ph[3] = 2 * v1 * v2 - c * v3;   Ph[4] = 1 + 2 * (v2 * v2 - vv);  Ph[5] = 2 * v2 * v3 + c * v1;
      Ph[6] = 2 * v1 * v3 + c * v2;   Ph[7] = 2 * v2 * v3 - c * v1;    Ph[8] = 1 + 2 * (v3 * v3 - vv);
    }
    // 2. the covariance; Am, Bm, Dm are A-, B-, D-
    real Af[9], Df[9], PA[9], PB[9], Am[9], Bm[9], Dm[6];
    filt_sym<real>(st.A, Af);
    filt_sym<real>(st.D, Df);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        PA[3 * i + j] = Ph[3 * i] * Af[j] + Ph[3 * i + 1] * Af[3 + j] + Ph[3 * i + 2] * Af[6 + j];
        PB[3 * i + j] = Ph[3 * i] * st.B[j] + Ph[3 * i + 1] * st.B[3 + j] + Ph[3 * i + 2] * st.B[6 + j];
      }
    const real qv = (f.sv * h) * (f.sv * h), hh = h * h;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) {
        const real pap = PA[3 * i] * Ph[3 * j] + PA[3 * i + 1] * Ph[3 * j + 1] + PA[3 * i + 2] * Ph[3 * j + 2];
        const real a = pap - h * (PB[3 * i + j] + PB[3 * j + i]) + hh * Df[3 * i + j] + (i == j ? qv : (real)0);
        Am[3 * i + j] = a; Am[3 * j + i] = a;
      }
    for (int i = 0; i < 9; ++i) Bm[i] = PB[i] - h * Df[i];
    {
      const real qu = f.su * f.su;
      Dm[0] = st.D[0] + qu; Dm[1] = st.D[1]; Dm[2] = st.D[2]; Dm[3] = st.D[3] + qu; Dm[4] = st.D[4]; Dm[5] = st.D[5] + qu;
    }
    // 3. the residual
    real z[3];
    {
      const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
      const real qn[4] = {m[3] * rn, m[4] * rn, m[5] * rn, m[6] * rn}, qc[4] = {qm[0], -qm[1], -qm[2], -qm[3]};
      real e[4];
      filt_qmult<real>(qc, qn, e);
      const real s2 = (e[0] < 0) ? (real)-2 : (real)2;
      for (int i = 0; i < 3; ++i) z[i] = s2 * e[1 + i];
    }
    // 4. S, its inverse by cofactors (symmetric), the gains and the correction
    real S[9], Si[9], Kt[9], Kb[9], dth[3], db[3];
    {
      const real ra = f.sa * f.sa;
      for (int i = 0; i < 9; ++i) S[i] = Am[i];
      S[0] += ra; S[4] += ra; S[8] += ra;
      const real c00 = S[4] * S[8] - S[5] * S[5], c01 = S[2] * S[5] - S[1] * S[8], c02 = S[1] * S[5] - S[2] * S[4];
      const real c11 = S[0] * S[8] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[5], c22 = S[0] * S[4] - S[1] * S[1];
      const real id = (real)1 / (S[0] * c00 + S[1] * c01 + S[2] * c02);
      Si[0] = c00 * id; Si[1] = c01 * id; Si[2] = c02 * id;
      Si[3] = Si[1];    Si[4] = c11 * id; Si[5] = c12 * id;
      Si[6] = Si[2];    Si[7] = Si[5];    Si[8] = c22 * id;
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Kt[3 * i + j] = Am[3 * i] * Si[j] + Am[3 * i + 1] * Si[3 + j] + Am[3 * i + 2] * Si[6 + j];
        Kb[3 * i + j] = Bm[i] * Si[j] + Bm[3 + i] * Si[3 + j] + Bm[6 + i] * Si[6 + j];      // B-^T S^-1
      }
    for (int i = 0; i < 3; ++i) {
      dth[i] = Kt[3 * i] * z[0] + Kt[3 * i + 1] * z[1] + Kt[3 * i + 2] * z[2];
      db[i] = Kb[3 * i] * z[0] + Kb[3 * i + 1] * z[1] + Kb[3 * i + 2] * z[2];
    }
    // 5. the state
    {
      const real dl[4] = {1, (real)0.5 * dth[0], (real)0.5 * dth[1], (real)0.5 * dth[2]};
      real qp[4];
      filt_qmult<real>(qm, dl, qp);
      const real rn = rsqrt_<real>(qp[0] * qp[0] + qp[1] * qp[1] + qp[2] * qp[2] + qp[3] * qp[3]);
      for (int i = 0; i < 4; ++i) st.q[i] = qp[i] * rn;
      for (int i = 0; i < 3; ++i) { st.b[i] = st.b[i] + db[i]; st.w[i] = m[i] - st.b[i]; }
    }
    // 6. P <- P- - K S K^T: Wt = Ktheta S, Wb = Kb S
    real Wt[9], Wb[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Wt[3 * i + j] = Kt[3 * i] * S[j] + Kt[3 * i + 1] * S[3 + j] + Kt[3 * i + 2] * S[6 + j];
        Wb[3 * i + j] = Kb[3 * i] * S[j] + Kb[3 * i + 1] * S[3 + j] + Kb[3 * i + 2] * S[6 + j];
      }
    {
      int u = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++u) {
          st.A[u] = Am[3 * i + j] - (Wt[3 * i] * Kt[3 * j] + Wt[3 * i + 1] * Kt[3 * j + 1] + Wt[3 * i + 2] * Kt[3 * j + 2]);
          st.D[u] = Dm[u] - (Wb[3 * i] * Kb[3 * j] + Wb[3 * i + 1] * Kb[3 * j + 1] + Wb[3 * i + 2] * Kb[3 * j + 2]);
        }
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        st.B[3 * i + j] = Bm[3 * i + j] - (Wt[3 * i] * Kb[3 * j] + Wt[3 * i + 1] * Kb[3 * j + 1] + Wt[3 * i + 2] * Kb[3 * j + 2]);
  }
  // y: the estimate as it stands, (w^, q^), or — `ahead` — with the attitude predicted across one step of delay
  TSAT_DEV void estimate(bool ahead, real y[7]) const {
    for (int i = 0; i < 3; ++i) y[i] = st.w[i];
    if (ahead) {
      real phi[3], d[4], qp[4];
      for (int i = 0; i < 3; ++i) phi[i] = h * st.w[i];
      filt_dq<real>(phi, d);
      filt_qmult<real>(st.q, d, qp);
      for (int i = 0; i < 4; ++i) y[3 + i] = qp[i];
    } else {
      for (int i = 0; i < 4; ++i) y[3 + i] = st.q[i];
    }
  }
  // y: the estimate the law sees at knot k
  TSAT_DEV void state(long long gid, int k, bool noisy, const real x[7], real y[7]) {
    real m[7];
    in.state(gid, k, noisy, x, m);                             // m_k, or m_max(k-1, 0)
    const int lat = f.s.latency;
    if (k == 0) first(m);
    else if (!(lat && k == 1)) step(m);
    estimate(lat && k > 0, y);                                 // predicted across the delay
    if (xh)
      for (int i = 0; i < 7; ++i) xh[(size_t)k * 7 + i] = y[i];
    if (ff && k == nt - 2) {                                   // the last knot that commands
      for (int i = 0; i < 3; ++i) ff[i] = st.b[i];
      ff[3] = sqrt_(st.A[0]); ff[4] = sqrt_(st.A[3]); ff[5] = sqrt_(st.A[5]);
      ff[6] = sqrt_(st.D[0]); ff[7] = sqrt_(st.D[3]); ff[8] = sqrt_(st.D[5]);
    }
  }
  TSAT_DEV void field(long long gid, int k, bool noisy, const real x[7], const real b0[3], real B[3]) {
    in.field(gid, k, noisy, x, b0, B);
  }
};

// What the filtered entry points reject besides what their sensed parents reject: "" or the reason
inline std::string check_filter(const tsat_filter_options* f) {
  if (!f) return "null filter options";
  const double v[5] = {f->sigma_v, f->sigma_u, f->sigma_a, f->p0_att, f->p0_bias};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return "filter sigma_v, sigma_u, sigma_a, p0_att and p0_bias must be finite and >= 0";
  if (f->sigma_a == 0.0) return "filter sigma_a must be > 0: S = A- + sigma_a^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void filtered_tv_wave(const FilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, Filtered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void filtered_tv_gg_wave(const FilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, Filtered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void filtered_pd_wave(const FilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, Filtered<real>(a.f));
}

template <typename real>
TSAT_DEV void filtered_pd_gg_wave(const FilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, Filtered<real>(a.f));
}

}  // namespace tsat
