// tsat_mag_bias_filtered.hpp — the magnetometer-updated attitude filter of tsat_mag_filtered.hpp with the MAGNETOMETER BIAS as a state
// (tsat_tvlqr_ensemble_mag_bias_filtered, tsat_pd_ensemble_mag_bias_filtered, include/tortoise_hip.h). On a magnetorquer-only
// satellite the magnetometer sits next to the torquers and a constant bias of several percent of the field is the normal case; the
// six-state mag filter lets it enter z unmodelled. This one carries nine error states — attitude error theta, gyro bias b,
// magnetometer bias c — and the measurement matrix [H 0 I].
//
// MagBiasFiltered is the sixth `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState, Sensed,
// Filtered, ModelFiltered and MagFiltered: it OWNS a Sensed, a FilterState (the 31-value record of tsat_filtered.hpp: q^, b^, w^, A, B,
// D) and the 27 values the new state adds — c^ 3, E (theta c) and F (b c) row-major 3 x 3, M (c c) as an upper triangle: 58 values a
// lane. Samples m_j = (w_m, q_m, b_m), rows r_j (brow_index(tm, j, 0.0), wave-uniform), h, dq(.), (x), the cofactor inverse and the
// latency rule are the mag filter's, word for word, and so is THE MAGNETOMETER IS SAMPLED ONCE PER KNOT: state() calls the inner
// Sensed::field itself and keeps the three values, field() hands the PD law those three — the raw reading the filter used, not
// corrected by c^.
//
// filt_propagate, filt_inv_sym and filt_correct of tsat_mag_filtered.hpp are used as they stand; the three new blocks have free
// functions of their own below. F and M need no propagation arithmetic (F- = F, M- = M + sigma_c^2 I).
//   first sample m_0:  as MagFiltered::first — q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I — and
//     c^ = 0, M = p0_mag^2 I, E = F = 0. The one attitude fix; no magnetometer update is made at the first sample
//   step on sample m_j, j >= 1:
//     1. q- and Phi as the mag filter
//     2. A-, B-, D- as the mag filter;  E- = Phi E - h F;  F- = F;  M- = M + sigma_c^2 I
//     3. n = q- / |q-|;  b^f = qrot(n, r_j) as TrueState::field computes it;  z = b_m - c^ - b^f;  H = -C(n) [r_j]x;
//        the measurement matrix is [H 0 I]
//     4. Gtheta = A- H^T + E-;  Gb = B-^T H^T + F-;  Gc = E-^T H^T + M-;  S = H Gtheta + Gc + sigma_m^2 I (3 x 3; its upper
//        triangle, mirrored; positive definite because sigma_m > 0);  K. = G. S^-1 for theta, b and c;  dtheta, db, dc = K. z
//     5. q^, b^ and w^ as the mag filter;  c^ <- c^ + dc
//     6. P <- P- - K S K^T by blocks, W. = K. S: the triangles of A, D and M;  B -= Wtheta Kb^T;  E -= Wtheta Kc^T;  F -= Wb Kc^T
//   A ZERO FIELD ROW IS NO LONGER A NO-OP: H = 0 leaves z = b_m - c^, which observes c directly — and rightly so, the plant's field
//   is zero there too, so the reading is bias plus noise (the last row of a magnetic_simulation table is such a row). Still no
//   branch, and nothing asks whether a sigma is zero. With p0_mag = sigma_c = 0 the blocks E, F, M and c^ stay zero and the
//   recursion is the mag filter's.
//   what the law sees at knot k is the mag filter's rule: latency 0 — the filter is at sample k; latency 1 — y_0 from the first
//   sample, m_0 handed over twice makes no step the second time, and for k >= 1 the estimate is predicted across the delay by
//   q^ (x) dq(h w^). At latency 1 the sample that arrives at knot k is knot k - 1's and is updated against r_{k-1}, not r_k.
#pragma once
#include <string>
#include "tsat_mag_filtered.hpp"

namespace tsat {

constexpr int MBFFW = TSAT_MAG_BIAS_FILTER_W;   // b^ 3, sqrt diag A 3, sqrt diag D 3, c^ 3, sqrt diag M 3

template <typename real>
struct MagBiasFiltArgs {
  MagFiltArgs<real> m;   // the mag filter's block: sensor, clock, tables, sigma_v, sigma_u, sigma_m, p0_att, p0_bias, XH; FF is [T][M][MBFFW]
  real sc, p0m;          // sigma_c, p0_mag
};

template <typename real>
struct MagBiasFilteredTvArgs {
  GgEnsArgs<real> g;     // as SensedTvArgs
  MagBiasFiltArgs<real> f;
};

template <typename real>
struct MagBiasFilteredPdArgs {
  PdArgs<real> p;        // as SensedPdArgs
  MagBiasFiltArgs<real> f;
};

// the launch block of the filter around that of its sensor (host)
inline MagBiasFiltArgs<double> mag_bias_filt_args(const tsat_mag_bias_filter_options& f, const SensArgs<double>& sa, const EnsArgs<double>& e,
                                                  double* XH, double* FF) {
  tsat_mag_filter_options g;
  g.sigma_v = f.sigma_v; g.sigma_u = f.sigma_u; g.sigma_m = f.sigma_m; g.p0_att = f.p0_att; g.p0_bias = f.p0_bias; g.reserved = 0;
  MagBiasFiltArgs<double> a;
  a.m = mag_filt_args(g, sa, e, XH, FF);
  a.sc = f.sigma_c; a.p0m = f.p0_mag;
  return a;
}

// step 2 for the block E: Em = Phi E - h F, Phi the matrix filt_propagate forms from the same record (the same operations, so that
// the compiler can share them)
template <typename real>
TSAT_DEV void magb_propagate_e(const FilterState<real>& st, real h, const real E[9], const real F[9], real Em[9]) {
  real phi[3], d[4], Ph[9];
  for (int i = 0; i < 3; ++i) phi[i] = h * st.w[i];
  filt_dq<real>(phi, d);
  {
    const real v1 = d[1], v2 = d[2], v3 = d[3], vv = v1 * v1 + v2 * v2 + v3 * v3, c = 2 * d[0];
    Ph[0] = 1 + 2 * (v1 * v1 - vv); Ph[1] = 2 * v1 * v2 + c * v3;    Ph[2] = 2 * v1 * v3 - c * v2;
    Ph[3] = 2 * v1 * v2 - c * v3;   Ph[4] = 1 + 2 * (v2 * v2 - vv);  Ph[5] = 2 * v2 * v3 + c * v1;
    Ph[6] = 2 * v1 * v3 + c * v2;   Ph[7] = 2 * v2 * v3 - c * v1;    Ph[8] = 1 + 2 * (v3 * v3 - vv);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      Em[3 * i + j] = (Ph[3 * i] * E[j] + Ph[3 * i + 1] * E[3 + j] + Ph[3 * i + 2] * E[6 + j]) - h * F[3 * i + j];
}

// step 4: G = X H^T + Y for a row-major X (`transposed`: X^T H^T + Y)
template <typename real, bool transposed>
TSAT_DEV void magb_gain_block(const real X[9], const real H[9], const real Y[9], real G[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const real x0 = transposed ? X[i] : X[3 * i], x1 = transposed ? X[3 + i] : X[3 * i + 1], x2 = transposed ? X[6 + i] : X[3 * i + 2];
      G[3 * i + j] = (x0 * H[3 * j] + x1 * H[3 * j + 1] + x2 * H[3 * j + 2]) + Y[3 * i + j];
    }
}

// K = G S^-1 and W = K S, one block at a time
template <typename real>
TSAT_DEV void magb_mul(const real G[9], const real Si[9], real K[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K[3 * i + j] = G[3 * i] * Si[j] + G[3 * i + 1] * Si[3 + j] + G[3 * i + 2] * Si[6 + j];
}

// steps 5 and 6 for what the new state adds, on the priors Em, F (= F-), Mm (full): c^ += Kc z; E = E- - Wtheta Kc^T;
// F -= Wb Kc^T; the triangle of M = M- - Wc Kc^T
template <typename real>
TSAT_DEV void magb_correct_c(real c[3], real E[9], real F[9], real Mc[6], const real Em[9], const real Mm[9], const real S[9],
                             const real Kt[9], const real Kb[9], const real Kc[9], const real z[3]) {
  for (int i = 0; i < 3; ++i) c[i] = c[i] + (Kc[3 * i] * z[0] + Kc[3 * i + 1] * z[1] + Kc[3 * i + 2] * z[2]);
  real W[9];
  magb_mul<real>(Kt, S, W);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      E[3 * i + j] = Em[3 * i + j] - (W[3 * i] * Kc[3 * j] + W[3 * i + 1] * Kc[3 * j + 1] + W[3 * i + 2] * Kc[3 * j + 2]);
  magb_mul<real>(Kb, S, W);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      F[3 * i + j] = F[3 * i + j] - (W[3 * i] * Kc[3 * j] + W[3 * i + 1] * Kc[3 * j + 1] + W[3 * i + 2] * Kc[3 * j + 2]);
  magb_mul<real>(Kc, S, W);
  int u = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++u)
      Mc[u] = Mm[3 * i + j] - (W[3 * i] * Kc[3 * j] + W[3 * i + 1] * Kc[3 * j + 1] + W[3 * i + 2] * Kc[3 * j + 2]);
}

template <typename real>
struct MagBiasFiltered {
  const MagBiasFiltArgs<real>& fb;
  const MagFiltArgs<real>& f;
  Sensed<real> in;
  FilterState<real> st;
  real c[3], E[9], F[9], Mc[6];                                // c^ and the blocks theta c, b c (row-major), c c (upper triangle)
  Traj<real> tm;                                               // the slew's clock and h
  const TSAT_CONSTMEM real* bt;                                // the slew's field table
  real bmag[3];                                                // b_m of this knot's sample: the one magnetometer reading of the knot
  int nt;                                                      // the slew's own knot count
  TSAT_GLOBAL real* xh;                                        // this realisation's rows of XH / record of FF, or null
  TSAT_GLOBAL real* ff;
  TSAT_DEV explicit MagBiasFiltered(const MagBiasFiltArgs<real>& f_) : fb(f_), f(f_.m), in(f_.m.s) {}
  TSAT_DEV void load(int traj, int r) {
    in.load(traj, r);
    nt = f.nk ? f.nk[traj] : f.N;
    tm = ensemble_traj<real>((const TSAT_CONSTMEM real*)(f.P + (size_t)traj * PSTRIDE), f.us, nt, f.n_tab);
    bt = (const TSAT_CONSTMEM real*)(f.BT + (size_t)f.bidx[traj] * f.n_tab * 4);
    const bool own = r < f.M;
    xh = (f.XH && own) ? (TSAT_GLOBAL real*)(f.XH + ((size_t)traj * f.M + r) * f.N * 7) : nullptr;
    ff = (f.FF && own) ? (TSAT_GLOBAL real*)(f.FF + ((size_t)traj * f.M + r) * MBFFW) : nullptr;
    for (int i = 0; i < 4; ++i) st.q[i] = 0;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = 0; bmag[i] = 0; c[i] = 0; }
    for (int i = 0; i < 6; ++i) { st.A[i] = 0; st.D[i] = 0; Mc[i] = 0; }
    for (int i = 0; i < 9; ++i) { st.B[i] = 0; E[i] = 0; F[i] = 0; }
  }
  TSAT_DEV void commanded(int, const real*) {}                 // the gyro propagates this filter, not the model
  TSAT_DEV void flown(const real*, const real*, const real*, const real*) {}
  TSAT_DEV void first(const real m[7]) {
    const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
    for (int i = 0; i < 4; ++i) st.q[i] = m[3 + i] * rn;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = m[i]; c[i] = 0; }
    const real a0 = f.p0a * f.p0a, d0 = f.p0b * f.p0b, m0 = fb.p0m * fb.p0m;
    st.A[0] = a0; st.A[1] = 0; st.A[2] = 0; st.A[3] = a0; st.A[4] = 0; st.A[5] = a0;
    st.D[0] = d0; st.D[1] = 0; st.D[2] = 0; st.D[3] = d0; st.D[4] = 0; st.D[5] = d0;
    Mc[0] = m0; Mc[1] = 0; Mc[2] = 0; Mc[3] = m0; Mc[4] = 0; Mc[5] = m0;
    for (int i = 0; i < 9; ++i) { st.B[i] = 0; E[i] = 0; F[i] = 0; }
  }
  // on the gyro sample wm and the field sample bs of knot j, rj the stage-0 field row of that knot
  TSAT_DEV void step(const real wm[3], const real bs[3], const real rj[3]) {
    // 1. and 2. q-, A-, B-, D-, E-, M- (F- = F)
    real qm[4], Am[9], Bm[9], Dm[6], Em[9], Mm[9];
    filt_propagate<real>(st, tm.h, f.sv, f.su, qm, Am, Bm, Dm);
    magb_propagate_e<real>(st, tm.h, E, F, Em);
    {
      const real qc = fb.sc * fb.sc;
      Mm[0] = Mc[0] + qc; Mm[1] = Mc[1]; Mm[2] = Mc[2];
      Mm[3] = Mc[1];      Mm[4] = Mc[3] + qc; Mm[5] = Mc[4];
      Mm[6] = Mc[2];      Mm[7] = Mc[4];      Mm[8] = Mc[5] + qc;
    }
    // 3. the predicted field, the residual and H = -C(n) [r]x
    real z[3], H[9];
    {
      const real rn = rsqrt_<real>(qm[0] * qm[0] + qm[1] * qm[1] + qm[2] * qm[2] + qm[3] * qm[3]);
      const real xq[7] = {0, 0, 0, qm[0], qm[1], qm[2], qm[3]};
      real bh[3];
      TrueState().field<real>(0, 0, false, xq, rj, bh);
      for (int i = 0; i < 3; ++i) z[i] = (bs[i] - c[i]) - bh[i];
      const real n0 = qm[0] * rn, v1 = qm[1] * rn, v2 = qm[2] * rn, v3 = qm[3] * rn, vv = v1 * v1 + v2 * v2 + v3 * v3, cc = 2 * n0;
      real Cn[9];
      Cn[0] = 1 + 2 * (v1 * v1 - vv); Cn[1] = 2 * v1 * v2 - cc * v3;   Cn[2] = 2 * v1 * v3 + cc * v2;
      Cn[3] = 2 * v1 * v2 + cc * v3;  Cn[4] = 1 + 2 * (v2 * v2 - vv);  Cn[5] = 2 * v2 * v3 - cc * v1;
      Cn[6] = 2 * v1 * v3 - cc * v2;  Cn[7] = 2 * v2 * v3 + cc * v1;   Cn[8] = 1 + 2 * (v3 * v3 - vv);
      for (int i = 0; i < 3; ++i) {
        H[3 * i] = Cn[3 * i + 2] * rj[1] - Cn[3 * i + 1] * rj[2];
        H[3 * i + 1] = Cn[3 * i] * rj[2] - Cn[3 * i + 2] * rj[0];
        H[3 * i + 2] = Cn[3 * i + 1] * rj[0] - Cn[3 * i] * rj[1];
      }
    }
    // 4. the three G blocks, S = H Gtheta + Gc + sigma_m^2 I, the gains
    real G[9], Gc[9], S[9], Si[9], Kt[9], Kb[9], Kc[9];
    magb_gain_block<real, false>(Am, H, Em, G);
    magb_gain_block<real, true>(Em, H, Mm, Gc);
    {
      const real rm = f.sm * f.sm;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
          const real v = (H[3 * i] * G[j] + H[3 * i + 1] * G[3 + j] + H[3 * i + 2] * G[6 + j]) + Gc[3 * i + j] + (i == j ? rm : (real)0);
          S[3 * i + j] = v; S[3 * j + i] = v;
        }
    }
    filt_inv_sym<real>(S, Si);
    magb_mul<real>(G, Si, Kt);
    magb_mul<real>(Gc, Si, Kc);
    magb_gain_block<real, true>(Bm, H, F, G);
    magb_mul<real>(G, Si, Kb);
    // the correction, 5. and 6.: the mag filter's for q^, b^, w^, A, B, D, then the new state's
    filt_correct<real>(st, wm, qm, Am, Bm, Dm, S, Kt, Kb, z);
    magb_correct_c<real>(c, E, F, Mc, Em, Mm, S, Kt, Kb, Kc, z);
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
      for (int i = 0; i < 3; ++i) { ff[i] = st.b[i]; ff[9 + i] = c[i]; }
      ff[3] = sqrt_(st.A[0]); ff[4] = sqrt_(st.A[3]); ff[5] = sqrt_(st.A[5]);
      ff[6] = sqrt_(st.D[0]); ff[7] = sqrt_(st.D[3]); ff[8] = sqrt_(st.D[5]);
      ff[12] = sqrt_(Mc[0]); ff[13] = sqrt_(Mc[3]); ff[14] = sqrt_(Mc[5]);
    }
  }
  // B: the reading state() took at this knot
  TSAT_DEV void field(long long, int, bool, const real*, const real*, real B[3]) {
    for (int i = 0; i < 3; ++i) B[i] = bmag[i];
  }
};

// What the mag-bias-filtered entry points reject besides what their sensed parents reject: "" or the reason
inline std::string check_mag_bias_filter(const tsat_mag_bias_filter_options* f) {
  if (!f) return "null filter options";
  const double v[7] = {f->sigma_v, f->sigma_u, f->sigma_m, f->sigma_c, f->p0_att, f->p0_bias, f->p0_mag};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return "filter sigma_v, sigma_u, sigma_m, sigma_c, p0_att, p0_bias and p0_mag must be finite and >= 0";
  if (f->sigma_m == 0.0) return "filter sigma_m must be > 0: S = H Gtheta + Gc + sigma_m^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void mag_bias_filtered_tv_wave(const MagBiasFilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, MagBiasFiltered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void mag_bias_filtered_tv_gg_wave(const MagBiasFilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, MagBiasFiltered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void mag_bias_filtered_pd_wave(const MagBiasFilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, MagBiasFiltered<real>(a.f));
}

template <typename real>
TSAT_DEV void mag_bias_filtered_pd_gg_wave(const MagBiasFilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, MagBiasFiltered<real>(a.f));
}

}  // namespace tsat
