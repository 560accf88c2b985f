// tsat_mag_filtered.hpp — a MAGNETOMETER-updated attitude filter between sensor and law in the ensembles
// (tsat_tvlqr_ensemble_mag_filtered, tsat_pd_ensemble_mag_filtered, include/tortoise_hip.h): the calls of tsat_filtered.hpp with the
// attitude update replaced by a magnetometer update. The satellite of the reference carries a gyro and a magnetometer and no sensor
// that hands over a quaternion; this filter takes ONE attitude fix, at knot 0, and from then on corrects the gyro-propagated attitude
// by the measured body field against the slew's own field table. The field fixes two of the three attitude angles at a knot; the third
// comes from the field's turning along the orbit and from the rate, so the estimate is much coarser than the six-state filter's.
//
// MagFiltered is the fifth `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState, Sensed,
// Filtered and ModelFiltered: it OWNS a Sensed and a FilterState (the 31-value record of tsat_filtered.hpp), runs over the samples
// m_j = (w_m, q_m, b_m) — the first two from Sensed::state, the third from Sensed::field — and hands the law its estimate. The slew's
// table pointer and clock are read as ModelFiltered::load reads them; r_j, the stage-0 field row of knot j (the row the roll-out hands
// `field` at that knot), is fetched through brow_index(tm, j, 0.0) with a wave-uniform index.
//
// THE MAGNETOMETER IS SAMPLED ONCE PER KNOT: state() calls the inner Sensed::field itself, with the row of knot k, and keeps the three
// values; field() hands the PD law those three and does not call the inner field again (a second call at latency 1 would push the
// one-knot buffer hb twice). Under the TVLQR law nobody calls field(): the TVLQR kernels of this unit draw n_m, their sensed and
// filtered parents do not.
//
// h, dq(.) and (x) are those of tsat_filtered.hpp; steps 1, 2, 5 and 6 and the cofactor inverse are Filtered::step's, operation for
// operation, in free functions below (filt_propagate, filt_inv_sym, filt_correct).
//   first sample m_0:  as Filtered::first — q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I. The one
//     attitude fix; q_m of every later sample is ignored, and no magnetometer update is made at the first sample
//   step on sample m_j, j >= 1:
//     1., 2. as Filtered::step: q-, A-, B-, D-
//     3. n = q- / |q-|;  b^ = qrot(n, r_j) as TrueState::field computes it;  z = b_m - b^;
//        H = -C(n) [r_j]x, C(n) = I + 2 n0 [v]x + 2 [v]x^2 with v = n[1:4]: qrot(n, v) = C(n) v, and H is the derivative of
//        qrot(q- (x) [1; dtheta / 2], r_j) in dtheta at 0
//     4. G = A- H^T, Gb = B-^T H^T;  S = H G + sigma_m^2 I (3 x 3; its upper triangle, mirrored; positive definite because
//        sigma_m > 0);  Ktheta = G S^-1, Kb = Gb S^-1;  dtheta = Ktheta z, db = Kb z
//     5., 6. as Filtered::step, with these K and S
//   A zero field row gives H = 0 and K = 0: an update that changes nothing, without a branch (the last row of a magnetic_simulation
//   table is such a row). Nothing asks whether a sigma is zero.
//   what the law sees at knot k is the six-state filter's rule: latency 0 — the filter is at sample k; latency 1 — y_0 from the first
//   sample, m_0 handed over twice makes no step the second time, and for k >= 1 the estimate is predicted across the delay by
//   q^ (x) dq(h w^). At latency 1 the sample that arrives at knot k is knot k - 1's and is updated against r_{k-1}, not r_k.
#pragma once
#include <string>
#include "tsat_filtered.hpp"

namespace tsat {

template <typename real>
struct MagFiltArgs {
  SensArgs<real> s;      // the inner sensor's block
  const real* P;         // [T][PSTRIDE] parameter records: h and the table clock
  const real* BT;        // [n_btab][n_tab][4] field rows
  const int* bidx;       // [T]
  const int* nk;         // [T] per-slew knot counts or null (all N)
  int M, N, n_tab;       // realisations of a slew; slab stride of XH; rows of a field table
  real us;               // u_scale (ensemble_traj takes it)
  real sv, su, sm;       // sigma_v, sigma_u, sigma_m
  real p0a, p0b;         // p0_att, p0_bias
  real* XH;              // [T][M][N][7] what the law saw, or null
  real* FF;              // [T][M][FFW] b^, sqrt(diag A), sqrt(diag D) after the last sample processed, or null
};

template <typename real>
struct MagFilteredTvArgs {
  GgEnsArgs<real> g;     // as SensedTvArgs
  MagFiltArgs<real> f;
};

template <typename real>
struct MagFilteredPdArgs {
  PdArgs<real> p;        // as SensedPdArgs
  MagFiltArgs<real> f;
};

// the launch block of the filter around that of its sensor (host); it reads the slew's clock and field rows itself
inline MagFiltArgs<double> mag_filt_args(const tsat_mag_filter_options& f, const SensArgs<double>& sa, const EnsArgs<double>& e, double* XH,
                                         double* FF) {
  MagFiltArgs<double> a;
  a.s = sa; a.P = e.P; a.BT = e.BT; a.bidx = e.bidx; a.nk = e.nk; a.M = e.M; a.N = e.N; a.n_tab = e.n_tab; a.us = e.us;
  a.sv = f.sigma_v; a.su = f.sigma_u; a.sm = f.sigma_m; a.p0a = f.p0_att; a.p0b = f.p0_bias;
  a.XH = XH; a.FF = FF;
  return a;
}

// The arithmetic this filter shares with Filtered::step, as free functions that only this header uses. Filtered::step keeps its own
// text: calling these from it was tried and changed the instruction streams of all nine kernels that hold it (the compiler simplifies
// a function on its own before it inlines it; profiles/builds/mag_filtered_isa_identity.txt), and no existing kernel may change.

// steps 1 and 2 of the recursion on the record `st`: qm = q-, Am = A- (full), Bm = B-, Dm = D- (upper triangle); st is not changed
template <typename real>
TSAT_DEV void filt_propagate(const FilterState<real>& st, real h, real sv, real su, real qm[4], real Am[9], real Bm[9], real Dm[6]) {
  // 1. propagate the attitude by the gyro; Phi = C^T = I - 2 d0 [v]x + 2 (v v^T - |v|^2 I)
  real phi[3], d[4];
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
  // 2. the covariance
  real Af[9], Df[9], PA[9], PB[9];
  filt_sym<real>(st.A, Af);
  filt_sym<real>(st.D, Df);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      PA[3 * i + j] = Ph[3 * i] * Af[j] + Ph[3 * i + 1] * Af[3 + j] + Ph[3 * i + 2] * Af[6 + j];
      PB[3 * i + j] = Ph[3 * i] * st.B[j] + Ph[3 * i + 1] * st.B[3 + j] + Ph[3 * i + 2] * st.B[6 + j];
    }
  const real qv = (sv * h) * (sv * h), hh = h * h;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const real pap = PA[3 * i] * Ph[3 * j] + PA[3 * i + 1] * Ph[3 * j + 1] + PA[3 * i + 2] * Ph[3 * j + 2];
      const real a = pap - h * (PB[3 * i + j] + PB[3 * j + i]) + hh * Df[3 * i + j] + (i == j ? qv : (real)0);
      Am[3 * i + j] = a; Am[3 * j + i] = a;
    }
  for (int i = 0; i < 9; ++i) Bm[i] = PB[i] - h * Df[i];
  {
    const real qu = su * su;
    Dm[0] = st.D[0] + qu; Dm[1] = st.D[1]; Dm[2] = st.D[2]; Dm[3] = st.D[3] + qu; Dm[4] = st.D[4]; Dm[5] = st.D[5] + qu;
  }
}

// the inverse of a symmetric positive definite 3 x 3 by cofactors and one reciprocal (reads the upper triangle)
template <typename real>
TSAT_DEV void filt_inv_sym(const real S[9], real Si[9]) {
  const real c00 = S[4] * S[8] - S[5] * S[5], c01 = S[2] * S[5] - S[1] * S[8], c02 = S[1] * S[5] - S[2] * S[4];
  const real c11 = S[0] * S[8] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[5], c22 = S[0] * S[4] - S[1] * S[1];
  const real id = (real)1 / (S[0] * c00 + S[1] * c01 + S[2] * c02);
  Si[0] = c00 * id; Si[1] = c01 * id; Si[2] = c02 * id;
  Si[3] = Si[1];    Si[4] = c11 * id; Si[5] = c12 * id;
  Si[6] = Si[2];    Si[7] = Si[5];    Si[8] = c22 * id;
}

// the correction of the recursion with the gains Kt, Kb and the innovation covariance S: dtheta = Kt z, db = Kb z, then steps 5
// and 6 on the prior (qm, Am, Bm, Dm); wm is the gyro sample
template <typename real>
TSAT_DEV void filt_correct(FilterState<real>& st, const real wm[3], const real qm[4], const real Am[9], const real Bm[9], const real Dm[6],
                           const real S[9], const real Kt[9], const real Kb[9], const real z[3]) {
  real dth[3], db[3];
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
    for (int i = 0; i < 3; ++i) { st.b[i] = st.b[i] + db[i]; st.w[i] = wm[i] - st.b[i]; }
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

template <typename real>
struct MagFiltered {
  const MagFiltArgs<real>& f;
  Sensed<real> in;
  FilterState<real> st;
  Traj<real> tm;                                               // the slew's clock and h
  const TSAT_CONSTMEM real* bt;                                // the slew's field table
  real bmag[3];                                                // b_m of this knot's sample: the one magnetometer reading of the knot
  int nt;                                                      // the slew's own knot count
  TSAT_GLOBAL real* xh;                                        // this realisation's rows of XH / record of FF, or null
  TSAT_GLOBAL real* ff;
  TSAT_DEV explicit MagFiltered(const MagFiltArgs<real>& f_) : f(f_), in(f_.s) {}
  TSAT_DEV void load(int traj, int r) {
    in.load(traj, r);
    nt = f.nk ? f.nk[traj] : f.N;
    tm = ensemble_traj<real>((const TSAT_CONSTMEM real*)(f.P + (size_t)traj * PSTRIDE), f.us, nt, f.n_tab);
    bt = (const TSAT_CONSTMEM real*)(f.BT + (size_t)f.bidx[traj] * f.n_tab * 4);
    const bool own = r < f.M;
    xh = (f.XH && own) ? (TSAT_GLOBAL real*)(f.XH + ((size_t)traj * f.M + r) * f.N * 7) : nullptr;
    ff = (f.FF && own) ? (TSAT_GLOBAL real*)(f.FF + ((size_t)traj * f.M + r) * FFW) : nullptr;
    for (int i = 0; i < 4; ++i) st.q[i] = 0;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = 0; bmag[i] = 0; }
    for (int i = 0; i < 6; ++i) { st.A[i] = 0; st.D[i] = 0; }
    for (int i = 0; i < 9; ++i) st.B[i] = 0;
  }
  TSAT_DEV void commanded(int, const real*) {}                 // the gyro propagates this filter, not the model
  TSAT_DEV void flown(const real*, const real*, const real*, const real*) {}
  TSAT_DEV void first(const real m[7]) {
    const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
    for (int i = 0; i < 4; ++i) st.q[i] = m[3 + i] * rn;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = m[i]; }
    const real a0 = f.p0a * f.p0a, d0 = f.p0b * f.p0b;
    st.A[0] = a0; st.A[1] = 0; st.A[2] = 0; st.A[3] = a0; st.A[4] = 0; st.A[5] = a0;
    st.D[0] = d0; st.D[1] = 0; st.D[2] = 0; st.D[3] = d0; st.D[4] = 0; st.D[5] = d0;
    for (int i = 0; i < 9; ++i) st.B[i] = 0;
  }
  // on the gyro sample wm and the field sample bs of knot j, rj the stage-0 field row of that knot
  TSAT_DEV void step(const real wm[3], const real bs[3], const real rj[3]) {
    // 1. and 2. q-, A-, B-, D-
    real qm[4], Am[9], Bm[9], Dm[6];
    filt_propagate<real>(st, tm.h, f.sv, f.su, qm, Am, Bm, Dm);
    // 3. the predicted field, the residual and H = -C(n) [r]x
    real z[3], H[9];
    {
      const real rn = rsqrt_<real>(qm[0] * qm[0] + qm[1] * qm[1] + qm[2] * qm[2] + qm[3] * qm[3]);
      const real xq[7] = {0, 0, 0, qm[0], qm[1], qm[2], qm[3]};
      real bh[3];
      TrueState().field<real>(0, 0, false, xq, rj, bh);
      for (int i = 0; i < 3; ++i) z[i] = bs[i] - bh[i];
      const real n0 = qm[0] * rn, v1 = qm[1] * rn, v2 = qm[2] * rn, v3 = qm[3] * rn, vv = v1 * v1 + v2 * v2 + v3 * v3, c = 2 * n0;
      real Cn[9];
      Cn[0] = 1 + 2 * (v1 * v1 - vv); Cn[1] = 2 * v1 * v2 - c * v3;    Cn[2] = 2 * v1 * v3 + c * v2;
      Cn[3] = 2 * v1 * v2 + c * v3;   Cn[4] = 1 + 2 * (v2 * v2 - vv);  Cn[5] = 2 * v2 * v3 - c * v1;
      Cn[6] = 2 * v1 * v3 - c * v2;   Cn[7] = 2 * v2 * v3 + c * v1;    Cn[8] = 1 + 2 * (v3 * v3 - vv);
      for (int i = 0; i < 3; ++i) {
        H[3 * i] = Cn[3 * i + 2] * rj[1] - Cn[3 * i + 1] * rj[2];
        H[3 * i + 1] = Cn[3 * i] * rj[2] - Cn[3 * i + 2] * rj[0];
        H[3 * i + 2] = Cn[3 * i + 1] * rj[0] - Cn[3 * i] * rj[1];
      }
    }
    // 4. G = A- H^T, Gb = B-^T H^T, S = H G + sigma_m^2 I, the gains
    real G[9], Gb[9], S[9], Si[9], Kt[9], Kb[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        G[3 * i + j] = Am[3 * i] * H[3 * j] + Am[3 * i + 1] * H[3 * j + 1] + Am[3 * i + 2] * H[3 * j + 2];
        Gb[3 * i + j] = Bm[i] * H[3 * j] + Bm[3 + i] * H[3 * j + 1] + Bm[6 + i] * H[3 * j + 2];
      }
    {
      const real rm = f.sm * f.sm;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
          const real v = H[3 * i] * G[j] + H[3 * i + 1] * G[3 + j] + H[3 * i + 2] * G[6 + j] + (i == j ? rm : (real)0);
          S[3 * i + j] = v; S[3 * j + i] = v;
        }
    }
    filt_inv_sym<real>(S, Si);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Kt[3 * i + j] = G[3 * i] * Si[j] + G[3 * i + 1] * Si[3 + j] + G[3 * i + 2] * Si[6 + j];
        Kb[3 * i + j] = Gb[3 * i] * Si[j] + Gb[3 * i + 1] * Si[3 + j] + Gb[3 * i + 2] * Si[6 + j];
      }
    // the correction, 5. and 6.
    filt_correct<real>(st, wm, qm, Am, Bm, Dm, S, Kt, Kb, z);
  }
  // y: the estimate as it stands, (w^, q^), or — `ahead` — with the attitude predicted across one step of delay
  TSAT_DEV void estimate(bool ahead, real y[7]) const {
    for (int i = 0; i < 3; ++i) y[i] = st.w[i];
    if (ahead) {
      real phi[3], d[4], qp[4];
      for (int i = 0; i < 3; ++i) phi[i] = tm.h * st.w[i];
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
    in.state(gid, k, noisy, x, m);                             // (w_m, q_m) of knot k, or of knot max(k - 1, 0)
    const int lat = f.s.latency;
    {
      const TSAT_CONSTMEM real* p = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tm, k, 0.0)) * 4;
      const real rk[3] = {p[0], p[1], p[2]};
      in.field(gid, k, noisy, x, rk, bmag);                    // b_m likewise: the one magnetometer sample of the knot
    }
    if (k == 0) {
      first(m);
    } else if (!(lat && k == 1)) {
      const TSAT_CONSTMEM real* p = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tm, lat ? k - 1 : k, 0.0)) * 4;   // the sample's own knot
      const real rj[3] = {p[0], p[1], p[2]};
      step(m, bmag, rj);
    }
    estimate(lat && k > 0, y);                                 // predicted across the delay
    if (xh)
      for (int i = 0; i < 7; ++i) xh[(size_t)k * 7 + i] = y[i];
    if (ff && k == nt - 2) {                                   // the last knot that commands
      for (int i = 0; i < 3; ++i) ff[i] = st.b[i];
      ff[3] = sqrt_(st.A[0]); ff[4] = sqrt_(st.A[3]); ff[5] = sqrt_(st.A[5]);
      ff[6] = sqrt_(st.D[0]); ff[7] = sqrt_(st.D[3]); ff[8] = sqrt_(st.D[5]);
    }
  }
  // B: the reading state() took at this knot
  TSAT_DEV void field(long long, int, bool, const real*, const real*, real B[3]) {
    for (int i = 0; i < 3; ++i) B[i] = bmag[i];
  }
};

// What the mag-filtered entry points reject besides what their sensed parents reject: "" or the reason
inline std::string check_mag_filter(const tsat_mag_filter_options* f) {
  if (!f) return "null filter options";
  const double v[5] = {f->sigma_v, f->sigma_u, f->sigma_m, f->p0_att, f->p0_bias};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return "filter sigma_v, sigma_u, sigma_m, p0_att and p0_bias must be finite and >= 0";
  if (f->sigma_m == 0.0) return "filter sigma_m must be > 0: S = H A- H^T + sigma_m^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void mag_filtered_tv_wave(const MagFilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, MagFiltered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void mag_filtered_tv_gg_wave(const MagFilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, MagFiltered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void mag_filtered_pd_wave(const MagFilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, MagFiltered<real>(a.f));
}

template <typename real>
TSAT_DEV void mag_filtered_pd_gg_wave(const MagFilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, MagFiltered<real>(a.f));
}

}  // namespace tsat
