// tsat_model_mag_filtered.hpp — the MODEL-BASED rate filter of tsat_model_filtered.hpp UPDATED BY THE MAGNETOMETER
// (tsat_tvlqr_ensemble_model_mag_filtered, tsat_pd_ensemble_model_mag_filtered, include/tortoise_hip.h): the nine-state
// multiplicative EKF over (dtheta, dw, db) with its attitude update a. replaced by the magnetometer update of
// tsat_mag_filtered.hpp. The satellite of the reference carries a gyro, a magnetometer and no sensor that hands over a quaternion:
// this filter takes ONE attitude fix, at knot 0, propagates (w^, q^) on the model under the command just issued, corrects the
// attitude by the measured body field against the slew's own table and smooths the gyro as a measurement of w^ + b^.
//
// ModelMagFiltered is the seventh `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState,
// Sensed, Filtered, ModelFiltered, MagFiltered and MagBiasFiltered: it OWNS a ModelFiltered — and through it the inner Sensed, the
// 58-value record ModelFilterState, the model's Traj and the slew's table pointer — and calls its load, commanded, first,
// predict(kk), correct and record AS THEY STAND. The record's layout is the parent's exactly, so a loop that carries it between
// launches can carry this filter's. New here are the magnetometer block and `bmag`; gyro block b. is restated, operation for
// operation, because ModelFiltered::update holds a. and b. in one function and no existing device header is edited.
//
// THE MAGNETOMETER IS SAMPLED ONCE PER KNOT, as MagFiltered samples it: state() calls the inner Sensed::field itself, with the row
// of knot k, and keeps the three values; field() hands the PD law those three and does not call the inner field again. Under the
// TVLQR law nobody calls field(): the TVLQR kernels of this unit draw n_m, their sensed and model-filtered parents do not.
//
//   first(m_0):  the parent's — the one attitude fix; q_m of every later sample is ignored, no magnetometer update at sample 0
//   predict(u):  the parent's, with the rows of the knot being crossed
//   update(m_j), j >= 1, r_j the stage-0 field row of the sample's own knot (brow_index(tm, j, 0.0), wave-uniform):
//     a. magnetometer: n = q^ / |q^|;  z = b_m - qrot(n, r_j) as TrueState::field computes it;  Hm = -C(n) [r_j]x (the mag filter's
//        H);  P H^T = [A Hm^T; X^T Hm^T; B^T Hm^T];  S = Hm A Hm^T + sigma_m^2 I (its upper triangle, mirrored)
//     b. gyro:         z = w_m - (w^ + b^);  S = W + Y + Y^T + D + sigma_g^2 I;  P H^T = [X + B; W + Y; Y^T + D]
//     each applies its whole 9-vector K z and P <- P - K S K^T through ModelFiltered::correct. a. is formed in a scope of its own,
//     so nothing of it is live across b.
//   A zero field row gives Hm = 0 and K = 0 in a.: an update that changes nothing, without a branch. Nothing asks whether a sigma
//   is zero.
//   what the law sees at knot k is the parent's rule — latency 0: k = 0 first; k >= 1 predict(u_{k-1}), update(m_k) against r_k;
//   latency 1: y_0 from first(m_0); k = 1: m_0 arrives a second time and makes no update, then predict(u_0); k >= 2:
//   update(m_{k-1}) against r_{k-1}, then predict(u_{k-1}). filt_final is the parent's 12 values after the last update made up to
//   and including k = n_knots - 2.
#pragma once
#include <string>
#include "tsat_model_filtered.hpp"

namespace tsat {

template <typename real>
struct ModelMagFiltArgs {
  ModelFiltArgs<real> m;   // the model filter's block: sensor, constants, tables, sigma_v, sigma_w, sigma_u, sigma_g, p0s, XH, FF (sa unused)
  real sm;                 // sigma_m
};

template <typename real>
struct ModelMagFilteredTvArgs {
  GgEnsArgs<real> g;
  ModelMagFiltArgs<real> f;
};

template <typename real>
struct ModelMagFilteredPdArgs {
  PdArgs<real> p;
  ModelMagFiltArgs<real> f;
};

// the launch block of the filter around that of its sensor (host)
inline ModelMagFiltArgs<double> model_mag_filt_args(const tsat_model_mag_filter_options& f, const SensArgs<double>& sa,
                                                    const EnsArgs<double>& e, double* XH, double* FF) {
  tsat_model_filter_options g;
  g.sigma_v = f.sigma_v; g.sigma_w = f.sigma_w; g.sigma_u = f.sigma_u; g.sigma_a = 0.0; g.sigma_g = f.sigma_g;
  g.p0_att = f.p0_att; g.p0_bias = f.p0_bias; g.reserved = 0;
  ModelMagFiltArgs<double> a;
  a.m = model_filt_args(g, sa, e, XH, FF);
  a.sm = f.sigma_m;
  return a;
}

template <typename real>
struct ModelMagFiltered {
  const ModelMagFiltArgs<real>& fm;
  ModelFiltered<real> mf;
  real bmag[3];                                                // b_m of this knot's sample: the one magnetometer reading of the knot
  TSAT_DEV explicit ModelMagFiltered(const ModelMagFiltArgs<real>& f_) : fm(f_), mf(f_.m) {}
  TSAT_DEV void load(int traj, int r) {
    mf.load(traj, r);
    for (int i = 0; i < 3; ++i) bmag[i] = 0;
  }
  TSAT_DEV void commanded(int k, const real uc[3]) { mf.commanded(k, uc); }
  // on the gyro sample wm and the field sample bs of knot j, rj the stage-0 field row of that knot
  TSAT_DEV void update(const real wm[3], const real bs[3], const real rj[3]) {
    ModelFilterState<real>& st = mf.st;
    {  // a. magnetometer: P H^T = [A Hm^T; X^T Hm^T; B^T Hm^T]
      real z[3], Ht[9], Hw[9], Hb[9], S[9];
      {
        real H[9];
        {
          const real* q = st.q;
          const real rn = rsqrt_<real>(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
          const real xq[7] = {0, 0, 0, q[0], q[1], q[2], q[3]};
          real bh[3];
          TrueState().field<real>(0, 0, false, xq, rj, bh);
          for (int i = 0; i < 3; ++i) z[i] = bs[i] - bh[i];
          const real n0 = q[0] * rn, v1 = q[1] * rn, v2 = q[2] * rn, v3 = q[3] * rn, vv = v1 * v1 + v2 * v2 + v3 * v3, c = 2 * n0;
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
        real Af[9];
        filt_sym<real>(st.A, Af);
        mf_mul_t<real>(Af, H, Ht);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            Hw[3 * i + j] = st.X[i] * H[3 * j] + st.X[3 + i] * H[3 * j + 1] + st.X[6 + i] * H[3 * j + 2];
            Hb[3 * i + j] = st.B[i] * H[3 * j] + st.B[3 + i] * H[3 * j + 1] + st.B[6 + i] * H[3 * j + 2];
          }
        const real rm = fm.sm * fm.sm;
        for (int i = 0; i < 3; ++i)
          for (int j = i; j < 3; ++j) {
            const real v = H[3 * i] * Ht[j] + H[3 * i + 1] * Ht[3 + j] + H[3 * i + 2] * Ht[6 + j] + (i == j ? rm : (real)0);
            S[3 * i + j] = v; S[3 * j + i] = v;
          }
      }
      mf.correct(Ht, Hw, Hb, S, z);
    }
    {  // b. gyro: P H^T = [X + B; W + Y; Y^T + D] — ModelFiltered::update's b., operation for operation
      real z[3], Ht[9], Hw[9], Hb[9], S[9], Wf[9], Df[9];
      for (int i = 0; i < 3; ++i) z[i] = wm[i] - (st.w[i] + st.b[i]);
      filt_sym<real>(st.W, Wf);
      filt_sym<real>(st.D, Df);
      for (int i = 0; i < 9; ++i) { Ht[i] = st.X[i] + st.B[i]; Hw[i] = Wf[i] + st.Y[i]; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Hb[3 * i + j] = st.Y[3 * j + i] + Df[3 * i + j];
      const real rg = mf.f.sg * mf.f.sg;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
          const real v = Wf[3 * i + j] + st.Y[3 * i + j] + st.Y[3 * j + i] + Df[3 * i + j] + (i == j ? rg : (real)0);
          S[3 * i + j] = v; S[3 * j + i] = v;
        }
      mf.correct(Ht, Hw, Hb, S, z);
    }
  }
  // y: the estimate the law sees at knot k
  TSAT_DEV void state(long long gid, int k, bool noisy, const real x[7], real y[7]) {
    real m[7];
    mf.in.state(gid, k, noisy, x, m);                          // (w_m, q_m) of knot k, or of knot max(k - 1, 0)
    const int lat = mf.f.s.latency;
    {
      const TSAT_CONSTMEM real* p = mf.bt + (size_t)TSAT_UNIFORM_INT(brow_index(mf.tm, k, 0.0)) * 4;
      const real rk[3] = {p[0], p[1], p[2]};
      mf.in.field(gid, k, noisy, x, rk, bmag);                 // b_m likewise: the one magnetometer sample of the knot
    }
    const bool last = (k == mf.nt - 2);                        // the last knot that commands
    if (k == 0) {
      mf.first(m);
      if (last) mf.record();
    } else if (lat) {
      if (k > 1) {                                             // m_0 handed over a second time makes no update
        const TSAT_CONSTMEM real* p = mf.bt + (size_t)TSAT_UNIFORM_INT(brow_index(mf.tm, k - 1, 0.0)) * 4;   // the sample's own knot
        const real rj[3] = {p[0], p[1], p[2]};
        update(m, bmag, rj);
      }
      if (last) mf.record();
      mf.predict(k - 1);
    } else {
      mf.predict(k - 1);
      const TSAT_CONSTMEM real* p = mf.bt + (size_t)TSAT_UNIFORM_INT(brow_index(mf.tm, k, 0.0)) * 4;
      const real rj[3] = {p[0], p[1], p[2]};
      update(m, bmag, rj);
      if (last) mf.record();
    }
    for (int i = 0; i < 3; ++i) y[i] = mf.st.w[i];
    for (int i = 0; i < 4; ++i) y[3 + i] = mf.st.q[i];
    if (mf.xh)
      for (int i = 0; i < 7; ++i) mf.xh[(size_t)k * 7 + i] = y[i];
  }
  // B: the reading state() took at this knot
  TSAT_DEV void field(long long, int, bool, const real*, const real*, real B[3]) {
    for (int i = 0; i < 3; ++i) B[i] = bmag[i];
  }
};

// What the model-mag-filtered entry points reject besides what their sensed parents reject: "" or the reason
inline std::string check_model_mag_filter(const tsat_model_mag_filter_options* f) {
  if (!f) return "null filter options";
  const double v[7] = {f->sigma_v, f->sigma_w, f->sigma_u, f->sigma_g, f->sigma_m, f->p0_att, f->p0_bias};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0)
      return "filter sigma_v, sigma_w, sigma_u, sigma_g, sigma_m, p0_att and p0_bias must be finite and >= 0";
  if (f->sigma_g == 0.0) return "filter sigma_g must be > 0: S = H P H^T + sigma_g^2 I has to be positive definite";
  if (f->sigma_m == 0.0) return "filter sigma_m must be > 0: S = Hm A Hm^T + sigma_m^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void model_mag_filtered_tv_wave(const ModelMagFilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelMagFiltered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void model_mag_filtered_tv_gg_wave(const ModelMagFilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelMagFiltered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void model_mag_filtered_pd_wave(const ModelMagFilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, ModelMagFiltered<real>(a.f));
}

template <typename real>
TSAT_DEV void model_mag_filtered_pd_gg_wave(const ModelMagFilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, ModelMagFiltered<real>(a.f));
}

}  // namespace tsat
