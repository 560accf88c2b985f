// tsat_model_mag_sun_filtered.hpp — the magnetometer-updated model filter of tsat_model_mag_filtered.hpp WITH A SUN SENSOR
// (tsat_tvlqr_ensemble_model_mag_sun_filtered, tsat_pd_ensemble_model_mag_sun_filtered, include/tortoise_hip.h): a second body
// vector, measured against a per-slew sun table, closes the rotation about the field that one field vector does not observe. The
// sensor is blind in eclipse: a row of the sun table that is exactly (0, 0, 0) is a knot in the Earth's shadow.
//
// ModelMagSunFiltered is the eighth `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), after TrueState,
// Sensed, Filtered, ModelFiltered, MagFiltered, MagBiasFiltered and ModelMagFiltered: it OWNS a ModelMagFiltered — and through it the
// ModelFiltered, the inner Sensed, the 58-value record, the model's Traj and the slew's field table — and calls its load, commanded,
// update and field, and the ModelFiltered's first, predict(kk), correct and record, AS THEY STAND. No existing device header is
// edited; state() is restated, as the parent restated its parent's, because the sun sample is drawn in it.
//
// THE SUN TABLE has the shape and the indexing of the field table: [n_btab][n_tab][4] packed rows, the slew's table chosen by
// bidx, the row of knot j the stage-0 row brow_index(tm, j, 0.0) on the same clock. A row is the sun direction in ECI (a unit
// vector in the intended use) or exactly zero. It is read by scalar loads and is wave-uniform: ECLIPSE IS A UNIFORM BRANCH.
//
// THE SUN SENSOR IS SAMPLED ONCE PER KNOT, inside state() beside the magnetometer sample:
//   s_m = qrot(x[3:7] / |x[3:7]|, s_k) + sigma_sun n_s            formed as TrueState::field forms the body field
// n_s the gyro triple of stage index 6 of the documented draw layout: Philox counter 24 of (gid, k), which nothing else uses.
// sigma_sun >= 0 is launch-uniform and dimensionless (radians for small angles). THERE IS NO PER-REALISATION SUN-SENSOR BIAS.
// Where the row is zero no block is generated and no sample exists. At latency 1 the sensor keeps the last sample (three values,
// as Sensed::hb keeps the field's) and pairs it with ITS OWN row s_{k-1}, not s_k. The noise-free realisation draws nothing.
//
//   first(m_0), predict(u), correct, record: the parent's
//   update(m_j), j >= 1:
//     a. magnetometer, b. gyro: ModelMagFiltered::update(w_m, b_m, r_j) as it stands
//     c. sun, only if s_j != 0 (uniform): n = q^ / |q^|;  z = s_m - qrot(n, s_j);  Hs = -C(n) [s_j]x;
//        P H^T = [A Hs^T; X^T Hs^T; B^T Hs^T];  S = Hs A Hs^T + sigma_s^2 I (its upper triangle, mirrored);  then correct.
//        It is block a. with (s_j, s_m, sigma_s) in the places of (r_j, b_m, sigma_m): vector_update below states that block once
//        as a function of (row, sample, sigma); it cannot be lifted out of the parent without editing the parent. It is formed in a
//        scope of its own, so nothing of it is live across correct.
//   c. is skipped BY BRANCH and not by K = 0: correct renormalises q^, and a dark knot must leave the parent's bits.
//   what the law sees at knot k is the parent's rule; no sun update at sample 0 and none at k = 1 of latency 1, as for the
//   magnetometer. X_hat and filt_final are the parent's (7 per knot; 12 values, TSAT_MODEL_FILTER_W).
#pragma once
#include <string>
#include "tsat_model_mag_filtered.hpp"

namespace tsat {

template <typename real>
struct ModelMagSunFiltArgs {
  ModelMagFiltArgs<real> g;   // the parent's block
  const real* ST;             // [n_btab][n_tab][4] sun rows, laid out like the field rows
  real ss;                    // sigma_s: what the filter assumes
  real ssun;                  // sigma_sun: what the sensor draws
};

template <typename real>
struct ModelMagSunFilteredTvArgs {
  GgEnsArgs<real> g;
  ModelMagSunFiltArgs<real> f;
};

template <typename real>
struct ModelMagSunFilteredPdArgs {
  PdArgs<real> p;
  ModelMagSunFiltArgs<real> f;
};

// the seven options the parent shares with this filter
inline tsat_model_mag_filter_options model_mag_options_of(const tsat_model_mag_sun_filter_options& f) {
  tsat_model_mag_filter_options g;
  g.sigma_v = f.sigma_v; g.sigma_w = f.sigma_w; g.sigma_u = f.sigma_u; g.sigma_g = f.sigma_g; g.sigma_m = f.sigma_m;
  g.p0_att = f.p0_att; g.p0_bias = f.p0_bias; g.reserved = f.reserved;
  return g;
}

// the launch block of the filter around that of its parent (host); ST the packed sun rows
inline ModelMagSunFiltArgs<double> model_mag_sun_filt_args(const tsat_model_mag_sun_filter_options& f, const SensArgs<double>& sa,
                                                            const EnsArgs<double>& e, double* XH, double* FF, const double* ST,
                                                            double sigma_sun) {
  ModelMagSunFiltArgs<double> a;
  a.g = model_mag_filt_args(model_mag_options_of(f), sa, e, XH, FF);
  a.ST = ST; a.ss = f.sigma_s; a.ssun = sigma_sun;
  return a;
}

template <typename real>
struct ModelMagSunFiltered {
  const ModelMagSunFiltArgs<real>& fs;
  ModelMagFiltered<real> mm;
  const TSAT_CONSTMEM real* sun;                               // the slew's sun table
  real smag[3];                                                // s_m the filter is handed at this knot
  real hs[3];                                                  // the sample of the last knot (latency = 1)
  TSAT_DEV explicit ModelMagSunFiltered(const ModelMagSunFiltArgs<real>& f_) : fs(f_), mm(f_.g) {}
  TSAT_DEV void load(int traj, int r) {
    mm.load(traj, r);
    sun = (const TSAT_CONSTMEM real*)(fs.ST + (size_t)mm.mf.f.bidx[traj] * mm.mf.f.n_tab * 4);
    for (int i = 0; i < 3; ++i) { smag[i] = 0; hs[i] = 0; }
  }
  TSAT_DEV void commanded(int k, const real uc[3]) { mm.commanded(k, uc); }
  // the update of a body vector measured against its inertial row: block a. of ModelMagFiltered::update, operation for operation,
  // as a function of (row, sample, sigma)
  TSAT_DEV void vector_update(const real rj[3], const real bs[3], real sigma) {
    ModelFiltered<real>& mf = mm.mf;
    ModelFilterState<real>& st = mf.st;
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
      const real rm = sigma * sigma;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
          const real v = H[3 * i] * Ht[j] + H[3 * i + 1] * Ht[3 + j] + H[3 * i + 2] * Ht[6 + j] + (i == j ? rm : (real)0);
          S[3 * i + j] = v; S[3 * j + i] = v;
        }
    }
    mf.correct(Ht, Hw, Hb, S, z);
  }
  // on the gyro sample wm, the field sample bs and the sun sample sm of knot j: jj the stage-0 row index of that knot in both tables
  TSAT_DEV void update(const real wm[3], const real bs[3], const real sm[3], int jj) {
    {
      const TSAT_CONSTMEM real* p = mm.mf.bt + (size_t)jj * 4;
      const real rj[3] = {p[0], p[1], p[2]};
      mm.update(wm, bs, rj);                                   // a. magnetometer and b. gyro: the parent's
    }
    const TSAT_CONSTMEM real* p = sun + (size_t)jj * 4;
    const real sj[3] = {p[0], p[1], p[2]};
    if (sj[0] != 0 || sj[1] != 0 || sj[2] != 0) {              // c. sun; wave-uniform: the row came by scalar loads
      vector_update(sj, sm, fs.ss);
    }
  }
  // y: the estimate the law sees at knot k
  TSAT_DEV void state(long long gid, int k, bool noisy, const real x[7], real y[7]) {
    ModelFiltered<real>& mf = mm.mf;
    real m[7];
    mf.in.state(gid, k, noisy, x, m);                          // (w_m, q_m) of knot k, or of knot max(k - 1, 0)
    const int lat = mf.f.s.latency;
    const int jk = TSAT_UNIFORM_INT(brow_index(mf.tm, k, 0.0));
    {
      const TSAT_CONSTMEM real* p = mf.bt + (size_t)jk * 4;
      const real rk[3] = {p[0], p[1], p[2]};
      mf.in.field(gid, k, noisy, x, rk, mm.bmag);              // b_m likewise: the one magnetometer sample of the knot
    }
    {
      const TSAT_CONSTMEM real* p = sun + (size_t)jk * 4;
      const real sk[3] = {p[0], p[1], p[2]};
      real sm[3] = {0, 0, 0};
      if (sk[0] != 0 || sk[1] != 0 || sk[2] != 0) {            // lit: the one sun sample of the knot; dark: none exists
        real ns[3] = {0, 0, 0};
        if (noisy) {
          unsigned w0[4];
          const unsigned ilo = (unsigned)((unsigned long long)gid & 0xFFFFFFFFull), ihi = (unsigned)((unsigned long long)gid >> 32);
          philox4x32_10(mf.f.s.k0, mf.f.s.k1, ilo, ihi, (unsigned)k, 24u, w0);
          real z[4];
          box_muller<real>(w0[0], w0[1], z[0], z[1]);
          box_muller<real>(w0[2], w0[3], z[2], z[3]);
          for (int i = 0; i < 3; ++i) ns[i] = fs.ssun * z[i];
        }
        real t[3];
        TrueState().field<real>(gid, k, noisy, x, sk, t);
        for (int i = 0; i < 3; ++i) sm[i] = t[i] + ns[i];
      }
      if (lat) {
        const bool old = k > 0;
        for (int i = 0; i < 3; ++i) { smag[i] = old ? hs[i] : sm[i]; hs[i] = sm[i]; }
      } else {
        for (int i = 0; i < 3; ++i) smag[i] = sm[i];
      }
    }
    const bool last = (k == mf.nt - 2);                        // the last knot that commands
    if (k == 0) {
      mf.first(m);
      if (last) mf.record();
    } else if (lat) {
      // m_0 handed over a second time makes no update; later samples go against the rows of their own knot
      if (k > 1) update(m, mm.bmag, smag, TSAT_UNIFORM_INT(brow_index(mf.tm, k - 1, 0.0)));
      if (last) mf.record();
      mf.predict(k - 1);
    } else {
      mf.predict(k - 1);
      update(m, mm.bmag, smag, jk);
      if (last) mf.record();
    }
    for (int i = 0; i < 3; ++i) y[i] = mf.st.w[i];
    for (int i = 0; i < 4; ++i) y[3 + i] = mf.st.q[i];
    if (mf.xh)
      for (int i = 0; i < 7; ++i) mf.xh[(size_t)k * 7 + i] = y[i];
  }
  // B: the magnetometer reading state() took at this knot
  TSAT_DEV void field(long long, int, bool, const real*, const real*, real B[3]) {
    for (int i = 0; i < 3; ++i) B[i] = mm.bmag[i];
  }
};

// What the entry points ask of the sun arguments before they dispatch — f == NULL is the sensed call and Stab == NULL the
// model-mag-filtered one, neither of which has a sun sensor: "" or the reason
inline std::string check_sun_arguments(bool has_f, const double* Stab, double sigma_sun) {
  if (!has_f && Stab) return "f is NULL (the sensed call): Stab must be NULL and sigma_sun 0";
  if (!Stab && !(sigma_sun == 0.0)) return "Stab is NULL (no sun sensor): sigma_sun must be 0";
  return "";
}

// What the model-mag-sun-filtered entry points reject besides what their sensed parents reject, with a sun table of `rows` rows of
// three: "" or the reason
inline std::string check_model_mag_sun_filter(const tsat_model_mag_sun_filter_options* f, const double* Stab, double sigma_sun,
                                              int64_t rows) {
  if (!f) return "null filter options";
  if (!Stab) return "null sun table";
  const double v[8] = {f->sigma_v, f->sigma_w, f->sigma_u, f->sigma_g, f->sigma_m, f->sigma_s, f->p0_att, f->p0_bias};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0)
      return "filter sigma_v, sigma_w, sigma_u, sigma_g, sigma_m, sigma_s, p0_att and p0_bias must be finite and >= 0";
  if (f->sigma_g == 0.0) return "filter sigma_g must be > 0: S = H P H^T + sigma_g^2 I has to be positive definite";
  if (f->sigma_m == 0.0) return "filter sigma_m must be > 0: S = Hm A Hm^T + sigma_m^2 I has to be positive definite";
  if (f->sigma_s == 0.0) return "filter sigma_s must be > 0: S = Hs A Hs^T + sigma_s^2 I has to be positive definite";
  if (f->reserved != 0) return "filter reserved must be 0";
  if (!std::isfinite(sigma_sun) || sigma_sun < 0.0) return "sigma_sun must be finite and >= 0";
  for (int64_t e = 0; e < rows * 3; ++e)
    if (!std::isfinite(Stab[e])) return "non-finite Stab entry in row " + std::to_string(e / 3);
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void model_mag_sun_filtered_tv_wave(const ModelMagSunFilteredTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelMagSunFiltered<real>(a.f));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void model_mag_sun_filtered_tv_gg_wave(const ModelMagSunFilteredTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, ModelMagSunFiltered<real>(a.f));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void model_mag_sun_filtered_pd_wave(const ModelMagSunFilteredPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, ModelMagSunFiltered<real>(a.f));
}

template <typename real>
TSAT_DEV void model_mag_sun_filtered_pd_gg_wave(const ModelMagSunFilteredPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, ModelMagSunFiltered<real>(a.f));
}

}  // namespace tsat
