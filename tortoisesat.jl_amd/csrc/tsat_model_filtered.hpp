// tsat_model_filtered.hpp — a MODEL-BASED rate filter between sensor and law in the ensembles (tsat_tvlqr_ensemble_model_filtered,
// tsat_pd_ensemble_model_filtered, include/tortoise_hip.h): the calls of tsat_filtered.hpp with a nine-state multiplicative EKF
// that carries the body rate as a state. The six-state filter hands the law w_m - b^, one gyro sample less the bias estimate;
// this one propagates (w^, q^) by the plant's own integrator on the MODEL — the model inertia, the field rows of the knot and
// the command the law has just issued — and takes the gyro as a MEASUREMENT of w^ + b^, so white gyro noise is smoothed to the
// level sigma_w (the un-modelled angular acceleration the filter assumes) allows.
//
// ModelFiltered is the fourth `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState,
// Sensed and Filtered: it OWNS a Sensed, runs over the samples m_j = (w_m, q_m) that Sensed::state produces and hands the law its
// estimate; `field` passes through to the inner Sensed. It learns the command through the one hook the roll-outs have for it,
// `commanded(k, uc)`, called where the command goes to plant.actuate: after the limit rule, before the plant's actuator matrix and
// residual dipole. J, h inv(J), h, the table clock and the field rows of the slew are read as the roll-outs read them, through
// constant-address-space pointers built from the block index and the loop counter (wave-uniform scalar loads).
//
// State of a lane: q^ (4, unit, scalar first), w^ (3), b^ (3), the command of the last knot (3) and the 9 x 9 covariance over
// (dtheta, dw, db) as its upper triangle by blocks: A (theta theta), W (w w), D (b b) as upper triangles (00 01 02 11 12 22),
// X (theta w), B (theta b), Y (w b) full row-major: 6 + 6 + 6 + 9 + 9 + 9 = 45 values, P symmetric by construction. One flat
// record of MFLW = 58 values (ModelFilterState) with load / save, for a loop that carries it between launches.
//
// h, dq(.), (x), C(.) and the 3 x 3 inverse are those of tsat_filtered.hpp.
//   first(m_0):  q^ = q_m / |q_m|, w^ = w_m, b^ = 0;  A = p0_att^2 I, D = p0_bias^2 I, W = (sigma_g^2 + p0_bias^2) I,
//                Y = -p0_bias^2 I, X = B = 0           (w - w_m = -(n + b): the consistent start)
//   predict(u):  (w-, q-) = one RK4 step of the model plant from (w^, q^) under u with the knot's field rows (what slot M of a
//                dispersed call flies: no noise, no disturbance, G = I, m_res = 0), q- normalised, b- = b^;  P- = Phi P Phi^T + Q,
//                Phi_tt = C(h w^)^T, Phi_tw = h I, Phi_ww = I + h J^-1 ([J w^]x - [w^]x J), Phi_bb = I, the rest 0,
//                Q = diag((sigma_v h)^2 I, (sigma_w h)^2 I, sigma_u^2 I), by blocks:
//                  A- = F A F^T + h (F X + (F X)^T) + h^2 W + qv I     X- = (F X + h W) G^T     B- = F B + h Y
//                  W- = G W G^T + qw I                                  Y- = G Y                 D- = D + qu I
//   update(m):   a. attitude: e = conj(q^) (x) q_m / |q_m|, z = 2 s e[1:4];  S = A + sigma_a^2 I;  K = P[:, theta] S^-1
//                b. gyro:     z = w_m - (w^ + b^);  S = W + Y + Y^T + D + sigma_g^2 I;  K = (P[:, w] + P[:, b]) S^-1
//                each: delta = K z;  q^ <- normalise(q^ (x) [1; dtheta / 2]), w^ += dw, b^ += db;  P <- P - K S K^T
//   what the law sees at knot k — latency 0: k = 0 first; k >= 1 predict(u_{k-1}) with the rows of knot k - 1, then update(m_k);
//   latency 1: y_0 from first(m_0); k = 1: m_0 arrives a second time and makes no update, then predict(u_0); k >= 2:
//   update(m_{k-1}) on the prior made at knot k - 1, then predict(u_{k-1}). y_k = (w^, q^) as the record then stands: at latency 1
//   and k >= 1 the model prediction across the delay, rate included.
// Latency, k == 0 and the skipped update are uniform branches; nothing asks whether a sigma is zero.
#pragma once
#include <string>
#include "tsat_filtered.hpp"

namespace tsat {

constexpr int MFLW = 58;                       // q^[4], w^[3], b^[3], u[3], A[6], W[6], D[6], X[9], B[9], Y[9]
constexpr int MFFW = TSAT_MODEL_FILTER_W;      // filt_final: b^[3], sqrt(diag A)[3], sqrt(diag W)[3], sqrt(diag D)[3]
// TSAT_MODEL_FILTER_STATE_W is the public header's (include/tortoise_hip.h, next to TSAT_FILTER_STATE_W). The same definition, token
// for token, stays here as well — which the language allows — because tests/test_model_filtered.py reads it in this file.
#define TSAT_MODEL_FILTER_STATE_W 58
static_assert(MFLW == TSAT_MODEL_FILTER_STATE_W, "the record of ModelFilterState");

template <typename real>
struct ModelFiltArgs {
  SensArgs<real> s;      // the inner sensor's block
  const real* P;         // [T][PSTRIDE] parameter records: h, J, inv(J), the table clock
  const real* BT;        // [n_btab][n_tab][4] field rows
  const int* bidx;       // [T]
  const int* nk;         // [T] per-slew knot counts or null (all N)
  int M, N, n_tab;       // realisations of a slew; slab stride of XH; rows of a field table
  real us;               // u_scale
  real sv, sw, su;       // sigma_v, sigma_w, sigma_u
  real sa, sg;           // sigma_a, sigma_g
  real p0a, p0b;         // p0_att, p0_bias
  real* XH;              // [T][M][N][7] what the law saw, or null
  real* FF;              // [T][M][MFFW], or null
};

template <typename real>
struct ModelFilteredTvArgs {
  GgEnsArgs<real> g;
  ModelFiltArgs<real> f;
};

template <typename real>
struct ModelFilteredPdArgs {
  PdArgs<real> p;
  ModelFiltArgs<real> f;
};

// the launch block of the nine-state filter around that of its sensor (host); it reads the slew's constants and field rows itself
inline ModelFiltArgs<double> model_filt_args(const tsat_model_filter_options& f, const SensArgs<double>& sa, const EnsArgs<double>& e,
                                             double* XH, double* FF) {
  ModelFiltArgs<double> a;
  a.s = sa; a.P = e.P; a.BT = e.BT; a.bidx = e.bidx; a.nk = e.nk; a.M = e.M; a.N = e.N; a.n_tab = e.n_tab; a.us = e.us;
  a.sv = f.sigma_v; a.sw = f.sigma_w; a.su = f.sigma_u; a.sa = f.sigma_a; a.sg = f.sigma_g; a.p0a = f.p0_att; a.p0b = f.p0_bias;
  a.XH = XH; a.FF = FF;
  return a;
}

// the flat record
template <typename real>
struct ModelFilterState {
  real q[4], w[3], b[3], u[3], A[6], W[6], D[6], X[9], B[9], Y[9];
  template <typename F>
  TSAT_DEV void each(F&& fn) {
    int o = 0;
    for (int i = 0; i < 4; ++i) fn(q[i], o++);
    for (int i = 0; i < 3; ++i) fn(w[i], o++);
    for (int i = 0; i < 3; ++i) fn(b[i], o++);
    for (int i = 0; i < 3; ++i) fn(u[i], o++);
    for (int i = 0; i < 6; ++i) fn(A[i], o++);
    for (int i = 0; i < 6; ++i) fn(W[i], o++);
    for (int i = 0; i < 6; ++i) fn(D[i], o++);
    for (int i = 0; i < 9; ++i) fn(X[i], o++);
    for (int i = 0; i < 9; ++i) fn(B[i], o++);
    for (int i = 0; i < 9; ++i) fn(Y[i], o++);
  }
  TSAT_DEV void load(const real* p, size_t stride = 1) {
    each([&](real& v, int o) { v = p[(size_t)o * stride]; });
  }
  TSAT_DEV void save(real* p, size_t stride = 1) {
    each([&](real& v, int o) { p[(size_t)o * stride] = v; });
  }
};

// r = a b, 3 x 3 row-major
template <typename real>
TSAT_DEV void mf_mul(const real a[9], const real b[9], real r[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// r = a b^T
template <typename real>
TSAT_DEV void mf_mul_t(const real a[9], const real b[9], real r[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// element (i, j) of a b^T
template <typename real>
TSAT_DEV real mf_abt(const real a[9], const real b[9], int i, int j) {
  return a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

template <typename real>
struct ModelFiltered {
  const ModelFiltArgs<real>& f;
  Sensed<real> in;
  ModelFilterState<real> st;
  Traj<real> tm;                                               // the model's: dyn_sim_h<real, 0> reads hh, J and hJi of it
  const TSAT_CONSTMEM real* bt;                                // the slew's field table
  int nt;                                                      // the slew's own knot count
  TSAT_GLOBAL real* xh;                                        // this realisation's rows of XH / record of FF, or null
  TSAT_GLOBAL real* ff;
  TSAT_DEV explicit ModelFiltered(const ModelFiltArgs<real>& f_) : f(f_), in(f_.s) {}
  TSAT_DEV void load(int traj, int r) {
    in.load(traj, r);
    nt = f.nk ? f.nk[traj] : f.N;
    tm = ensemble_traj<real>((const TSAT_CONSTMEM real*)(f.P + (size_t)traj * PSTRIDE), f.us, nt, f.n_tab);
    bt = (const TSAT_CONSTMEM real*)(f.BT + (size_t)f.bidx[traj] * f.n_tab * 4);
    const bool own = r < f.M;
    xh = (f.XH && own) ? (TSAT_GLOBAL real*)(f.XH + ((size_t)traj * f.M + r) * f.N * 7) : nullptr;
    ff = (f.FF && own) ? (TSAT_GLOBAL real*)(f.FF + ((size_t)traj * f.M + r) * MFFW) : nullptr;
    st.each([](real& v, int) { v = 0; });
  }
  // the hook of the roll-outs: the command of knot k as it goes to plant.actuate
  TSAT_DEV void commanded(int, const real uc[3]) {
    for (int c = 0; c < 3; ++c) st.u[c] = uc[c];
  }
  TSAT_DEV void first(const real m[7]) {
    const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
    for (int i = 0; i < 4; ++i) st.q[i] = m[3 + i] * rn;
    for (int i = 0; i < 3; ++i) { st.b[i] = 0; st.w[i] = m[i]; }
    const real a0 = f.p0a * f.p0a, d0 = f.p0b * f.p0b, w0 = f.sg * f.sg + d0;
    for (int i = 0; i < 6; ++i) {
      const bool dg = (i == 0 || i == 3 || i == 5);
      st.A[i] = dg ? a0 : (real)0; st.W[i] = dg ? w0 : (real)0; st.D[i] = dg ? d0 : (real)0;
    }
    for (int i = 0; i < 9; ++i) {
      st.X[i] = 0; st.B[i] = 0;
      st.Y[i] = (i == 0 || i == 4 || i == 8) ? -d0 : (real)0;
    }
  }
  // across knot kk under the command st.u: the knot's field rows of the slew's own table, wave-uniform
  TSAT_DEV void predict(int kk) {
    const TSAT_CONSTMEM real* p0 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tm, kk, 0.0)) * 4;
    const TSAT_CONSTMEM real* p1 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tm, kk, 0.5)) * 4;
    const TSAT_CONSTMEM real* p2 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tm, kk, 1.0)) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    predict(b0, b1, b2);
  }
  // across a step of the model tm under the command st.u with the field rows b0, b1, b2 at c = 0, 1/2, 1, wherever they come from
  // (the held loop of tsat_mpc_model_filtered.hpp hands over the rows its plant read)
  TSAT_DEV void predict(const real b0[3], const real b1[3], const real b2[3]) {
    const real h = tm.h;
    // the mean: one step of the plant's integrator on the model
    const real wo[3] = {st.w[0], st.w[1], st.w[2]};
    {
      const real cs = control_scale<real, 0>(tm);
      real x[7], us[3], k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
      for (int i = 0; i < 9; ++i) nz[i] = 0;
      for (int i = 0; i < 3; ++i) { x[i] = st.w[i]; us[i] = st.u[i] * cs; }
      for (int i = 0; i < 4; ++i) x[3 + i] = st.q[i];
      dyn_sim_h<real, 0>(tm, x, us, b0, false, nz, k1);
      for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
      dyn_sim_h<real, 0>(tm, t, us, b1, false, nz, k2);
      for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
      dyn_sim_h<real, 0>(tm, t, us, b1, false, nz, k3);
      for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
      dyn_sim_h<real, 0>(tm, t, us, b2, false, nz, k4);
      for (int i = 0; i < 7; ++i) x[i] = x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (real)(1.0 / 6.0);
      const real rn = rsqrt_<real>(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
      for (int i = 0; i < 3; ++i) st.w[i] = x[i];
      for (int i = 0; i < 4; ++i) st.q[i] = x[3 + i] * rn;
    }
    // Phi_tt = C(h w^)^T and Phi_ww, at the estimate the step started from (formed after the mean: fewer values live across the stages)
    real F[9], G[9];
    {
      real phi[3], d[4];
      for (int i = 0; i < 3; ++i) phi[i] = h * wo[i];
      filt_dq<real>(phi, d);
      const real v1 = d[1], v2 = d[2], v3 = d[3], vv = v1 * v1 + v2 * v2 + v3 * v3, c = 2 * d[0];
      F[0] = 1 + 2 * (v1 * v1 - vv); F[1] = 2 * v1 * v2 + c * v3;    F[2] = 2 * v1 * v3 - c * v2;
      F[3] = 2 * v1 * v2 - c * v3;   F[4] = 1 + 2 * (v2 * v2 - vv);  F[5] = 2 * v2 * v3 + c * v1;
      F[6] = 2 * v1 * v3 + c * v2;   F[7] = 2 * v2 * v3 - c * v1;    F[8] = 1 + 2 * (v3 * v3 - vv);
    }
    {
      const real w0 = wo[0], w1 = wo[1], w2 = wo[2];
      const real* J = tm.J;
      const real j0 = J[0] * w0 + J[1] * w1 + J[2] * w2, j1 = J[3] * w0 + J[4] * w1 + J[5] * w2, j2 = J[6] * w0 + J[7] * w1 + J[8] * w2;
      // Mx = [J w]x - [w]x J
      real Mx[9];
      Mx[0] = (w2 * J[3] - w1 * J[6]);       Mx[1] = -j2 + (w2 * J[4] - w1 * J[7]); Mx[2] = j1 + (w2 * J[5] - w1 * J[8]);
      Mx[3] = j2 + (w0 * J[6] - w2 * J[0]);  Mx[4] = (w0 * J[7] - w2 * J[1]);       Mx[5] = -j0 + (w0 * J[8] - w2 * J[2]);
      Mx[6] = -j1 + (w1 * J[0] - w0 * J[3]); Mx[7] = j0 + (w1 * J[1] - w0 * J[4]);  Mx[8] = (w1 * J[2] - w0 * J[5]);
      mf_mul<real>(tm.hJi, Mx, G);
      G[0] += 1; G[4] += 1; G[8] += 1;
    }
    // the covariance, block by block
    const real hh = h * h, qv = (f.sv * h) * (f.sv * h), qw = (f.sw * h) * (f.sw * h), qu = f.su * f.su;
    real Wf[9], FX[9];
    filt_sym<real>(st.W, Wf);
    mf_mul<real>(F, st.X, FX);
    {  // A- = F A F^T + h (F X + (F X)^T) + h^2 W + qv I
      real Af[9], FA[9];
      filt_sym<real>(st.A, Af);
      mf_mul<real>(F, Af, FA);
      int u = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++u)
          st.A[u] = mf_abt<real>(FA, F, i, j) + h * (FX[3 * i + j] + FX[3 * j + i]) + hh * Wf[3 * i + j] + (i == j ? qv : (real)0);
    }
    {  // B- = F B + h Y, with the old Y
      real FB[9];
      mf_mul<real>(F, st.B, FB);
      for (int i = 0; i < 9; ++i) st.B[i] = FB[i] + h * st.Y[i];
    }
    {  // X- = (F X + h W) G^T
      real Tm[9];
      for (int i = 0; i < 9; ++i) Tm[i] = FX[i] + h * Wf[i];
      mf_mul_t<real>(Tm, G, st.X);
    }
    {  // W- = G W G^T + qw I,  Y- = G Y,  D- = D + qu I
      real GW[9], GY[9];
      mf_mul<real>(G, Wf, GW);
      int u = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++u) st.W[u] = mf_abt<real>(GW, G, i, j) + (i == j ? qw : (real)0);
      mf_mul<real>(G, st.Y, GY);
      for (int i = 0; i < 9; ++i) st.Y[i] = GY[i];
      st.D[0] += qu; st.D[3] += qu; st.D[5] += qu;
    }
  }
  // one 3-vector update: Ht, Hw, Hb the theta, w and b rows of P H^T (3 x 3 each), S = H P H^T + R (symmetric), z the residual
  TSAT_DEV void correct(const real Ht[9], const real Hw[9], const real Hb[9], const real S[9], const real z[3]) {
    real Si[9];
    {
      const real c00 = S[4] * S[8] - S[5] * S[5], c01 = S[2] * S[5] - S[1] * S[8], c02 = S[1] * S[5] - S[2] * S[4];
      const real c11 = S[0] * S[8] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[5], c22 = S[0] * S[4] - S[1] * S[1];
      const real id = (real)1 / (S[0] * c00 + S[1] * c01 + S[2] * c02);
      Si[0] = c00 * id; Si[1] = c01 * id; Si[2] = c02 * id;
      Si[3] = Si[1];    Si[4] = c11 * id; Si[5] = c12 * id;
      Si[6] = Si[2];    Si[7] = Si[5];    Si[8] = c22 * id;
    }
    real Kt[9], Kw[9], Kb[9];
    mf_mul<real>(Ht, Si, Kt);
    mf_mul<real>(Hw, Si, Kw);
    mf_mul<real>(Hb, Si, Kb);
    {  // the state
      real dth[3];
      for (int i = 0; i < 3; ++i) {
        dth[i] = Kt[3 * i] * z[0] + Kt[3 * i + 1] * z[1] + Kt[3 * i + 2] * z[2];
        st.w[i] = st.w[i] + (Kw[3 * i] * z[0] + Kw[3 * i + 1] * z[1] + Kw[3 * i + 2] * z[2]);
        st.b[i] = st.b[i] + (Kb[3 * i] * z[0] + Kb[3 * i + 1] * z[1] + Kb[3 * i + 2] * z[2]);
      }
      const real dl[4] = {1, (real)0.5 * dth[0], (real)0.5 * dth[1], (real)0.5 * dth[2]};
      real qp[4];
      filt_qmult<real>(st.q, dl, qp);
      const real rn = rsqrt_<real>(qp[0] * qp[0] + qp[1] * qp[1] + qp[2] * qp[2] + qp[3] * qp[3]);
      for (int i = 0; i < 4; ++i) st.q[i] = qp[i] * rn;
    }
    // P <- P - K S K^T, with K S = P H^T: the rows the update came in with
    const real *Vt = Ht, *Vw = Hw, *Vb = Hb;
    int u = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++u) {
        st.A[u] = st.A[u] - mf_abt<real>(Vt, Kt, i, j);
        st.W[u] = st.W[u] - mf_abt<real>(Vw, Kw, i, j);
        st.D[u] = st.D[u] - mf_abt<real>(Vb, Kb, i, j);
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        st.X[3 * i + j] = st.X[3 * i + j] - mf_abt<real>(Vt, Kw, i, j);
        st.B[3 * i + j] = st.B[3 * i + j] - mf_abt<real>(Vt, Kb, i, j);
        st.Y[3 * i + j] = st.Y[3 * i + j] - mf_abt<real>(Vw, Kb, i, j);
      }
  }
  TSAT_DEV void update(const real m[7]) {
    {  // a. attitude: P H^T = [A; X^T; B^T]
      real z[3], Ht[9], Hw[9], Hb[9], S[9];
      {
        const real rn = rsqrt_<real>(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
        const real qn[4] = {m[3] * rn, m[4] * rn, m[5] * rn, m[6] * rn}, qc[4] = {st.q[0], -st.q[1], -st.q[2], -st.q[3]};
        real e[4];
        filt_qmult<real>(qc, qn, e);
        const real s2 = (e[0] < 0) ? (real)-2 : (real)2;
        for (int i = 0; i < 3; ++i) z[i] = s2 * e[1 + i];
      }
      filt_sym<real>(st.A, Ht);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { Hw[3 * i + j] = st.X[3 * j + i]; Hb[3 * i + j] = st.B[3 * j + i]; }
      const real ra = f.sa * f.sa;
      for (int i = 0; i < 9; ++i) S[i] = Ht[i];
      S[0] += ra; S[4] += ra; S[8] += ra;
      correct(Ht, Hw, Hb, S, z);
    }
    {  // b. gyro: P H^T = [X + B; W + Y; Y^T + D]
      real z[3], Ht[9], Hw[9], Hb[9], S[9], Wf[9], Df[9];
      for (int i = 0; i < 3; ++i) z[i] = m[i] - (st.w[i] + st.b[i]);
      filt_sym<real>(st.W, Wf);
      filt_sym<real>(st.D, Df);
      for (int i = 0; i < 9; ++i) { Ht[i] = st.X[i] + st.B[i]; Hw[i] = Wf[i] + st.Y[i]; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Hb[3 * i + j] = st.Y[3 * j + i] + Df[3 * i + j];
      const real rg = f.sg * f.sg;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
          const real v = Wf[3 * i + j] + st.Y[3 * i + j] + st.Y[3 * j + i] + Df[3 * i + j] + (i == j ? rg : (real)0);
          S[3 * i + j] = v; S[3 * j + i] = v;
        }
      correct(Ht, Hw, Hb, S, z);
    }
  }
  TSAT_DEV void record() {
    if (!ff) return;
    for (int i = 0; i < 3; ++i) ff[i] = st.b[i];
    ff[3] = sqrt_(st.A[0]); ff[4] = sqrt_(st.A[3]); ff[5] = sqrt_(st.A[5]);
    ff[6] = sqrt_(st.W[0]); ff[7] = sqrt_(st.W[3]); ff[8] = sqrt_(st.W[5]);
    ff[9] = sqrt_(st.D[0]); ff[10] = sqrt_(st.D[3]); ff[11] = sqrt_(st.D[5]);
  }
  // y: the estimate the law sees at knot k
  TSAT_DEV void state(long long gid, int k, bool noisy, const real x[7], real y[7]) {
    real m[7];
    in.state(gid, k, noisy, x, m);                             // m_k, or m_max(k-1, 0)
    const int lat = f.s.latency;
    const bool last = (k == nt - 2);                           // the last knot that commands
    if (k == 0) {
      first(m);
      if (last) record();
    } else if (lat) {
      if (k > 1) update(m);                                    // m_0 handed over a second time makes no update
      if (last) record();
      predict(k - 1);
    } else {
      predict(k - 1);
      update(m);
      if (last) record();
    }
    for (int i = 0; i < 3; ++i) y[i] = st.w[i];
    for (int i = 0; i < 4; ++i) y[3 + i] = st.q[i];
    if (xh)
      for (int i = 0; i < 7; ++i) xh[(size_t)k * 7 + i] = y[i];
  }
  TSAT_DEV void field(long long gid, int k, bool noisy, const real x[7], const real b0[3], real B[3]) {
    in.field(gid, k, noisy, x, b0, B);
  }
};

// What the model-filtered entry points reject besides what their sensed parents reject: "" or the reason
inline std::string check_model_filter(const tsat_model_filter_options* f) {
  if (!f) return "null filter options";
  const double v[7] = {f->sigma_v, f->sigma_w, f->sigma_u, f->sigma_a, f->sigma_g, f->p0_att, f->p0_bias};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0)
      return "filter sigma_v, sigma_w, sigma_u, sigma_a, sigma_g, p0_att and p0_bias must be finite and >= 0";
  if (f->sigma_a == 0.0) return "filter sigma_a must be > 0: S = P_tt + sigma_a^2 I has to be positive definite";
  if (f->sigma_g == 0.0) return "filter sigma_g must be > 0: S = H P H^T + sigma_g^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void model_filtered_tv_wave(const ModelFilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelFiltered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void model_filtered_tv_gg_wave(const ModelFilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelFiltered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void model_filtered_pd_wave(const ModelFilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, ModelFiltered<real>(a.f));
}

template <typename real>
TSAT_DEV void model_filtered_pd_gg_wave(const ModelFilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, ModelFiltered<real>(a.f));
}

}  // namespace tsat
