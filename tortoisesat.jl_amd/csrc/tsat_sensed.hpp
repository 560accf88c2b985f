// tsat_sensed.hpp — the ensemble controllers fed MEASUREMENTS (tsat_tvlqr_ensemble_sensed, tsat_pd_ensemble_sensed,
// include/tortoise_hip.h): the TVLQR feedback of tsat_tvlqr_ensemble_gg and the projection PD law of tsat_pd_ensemble on the same
// plants, but commanding from a biased, noisy, optionally one-knot-old measurement of the lane's state instead of the state itself.
//
// Per knot k of realisation (t, m), x the TRUE state, (bw, ba, bm) the realisation's nine biases:
//   w_m = x[0:3] + bw + n_w
//   phi = ba + n_a;  th = |phi|;  dq = [cos(th/2); phi * (th == 0 ? 1/2 : sin(th/2)/th)]       (a select, not a branch)
//   q_m = x[3:7] (x) dq                                        not normalised: the TVLQR feedback uses x[3:7] raw
//   b_m = qrot(x[3:7] / |x[3:7]|, b0) + bm + n_m               b0: the stage-0 field row of knot k; the TRUE body field
// with n_w, n_a the gyro and attitude triples of stage index 4 of the documented draw layout (Philox counters 16 and 17 of
// (gid, k)) at levels sigma_gyro, sigma_att of the SENSOR options, n_m the gyro triple of stage index 5 (counter 20) at sigma_mag.
// The plant never uses those stages. Words nobody reads are not generated: two blocks for (n_w, n_a), one for n_m, and the
// TVLQR kernels draw no n_m at all. latency = 1: the command of knot k is computed from the measurement of knot max(k - 1, 0),
// the reference record stays that of knot k.
//
// Sensed is the `Sensor` of ensemble_rollout (tsat_ensemble.hpp) and pd_rollout (tsat_pd.hpp), as GgPlant is their `Plant`:
// the loops, the plants, the limit rules and the statistic are the parents' own code. The nine biases of a lane are one record,
// stored component-major [T][SNW][Mp] like the plant records (one coalesced 512-byte access per component), slot M and the
// padding zero; the lane holds them and the measurement of the last knot (7, and 3 more under the PD law) in registers. The
// sigmas and latency are launch-uniform; latency is a uniform branch, and nothing asks whether a sigma is zero. The noise-free
// realisation (slot M) draws nothing and has zero biases: the ideal sensor at the call's latency.
#pragma once
#include <string>
#include "tsat_pd.hpp"

namespace tsat {

constexpr int SNW = 9;           // biases of a realisation: bw[3], ba[3], bm[3]

template <typename real>
struct SensArgs {
  const real* SN;        // [T][SNW][Mp] packed biases, slot M = 0
  int Mp;                // 64 * ensemble_waves(M)
  real sgy, sat, smg;    // sigma_gyro, sigma_att, sigma_mag of the sensor
  int latency;           // 0 | 1
  unsigned k0, k1;       // generator key (that of the plant noise)
};

template <typename real>
struct SensedTvArgs {
  GgEnsArgs<real> g;     // the gravity ensemble's block; g.GT null: the plants of the dispersed call
  SensArgs<real> s;
};

template <typename real>
struct SensedPdArgs {
  PdArgs<real> p;        // the PD call's block, as it is
  SensArgs<real> s;
};

// the launch block of the sensor from the options of both calls (host)
inline SensArgs<double> sens_args(const tsat_sensor_options& s, const tsat_tvlqr_options& o, const double* SN, int Mp) {
  SensArgs<double> a;
  a.SN = SN; a.Mp = Mp; a.sgy = s.sigma_gyro; a.sat = s.sigma_att; a.smg = s.sigma_mag; a.latency = s.latency;
  a.k0 = (unsigned)(o.noise_seed & 0xFFFFFFFFull); a.k1 = (unsigned)(o.noise_seed >> 32);
  return a;
}

// sensor biases 9 x M x T (or null: zeros) -> [T][SNW][Mp]; thread e of the pack grid: slot e % Mp of slew e / Mp
template <typename real>
TSAT_DEV void sensed_pack(const real* sensor, real* SN, int64_t T, int M, int Mp, int64_t e) {
  if (e >= T * (int64_t)Mp) return;
  const int64_t t = e / Mp;
  const int m = (int)(e - t * Mp);
  const TSAT_GLOBAL real* in = (sensor && m < M) ? (const TSAT_GLOBAL real*)(sensor + ((size_t)t * M + m) * SNW) : nullptr;
  TSAT_GLOBAL real* out = (TSAT_GLOBAL real*)(SN + (size_t)t * SNW * Mp + m);
  for (int i = 0; i < SNW; ++i) out[(size_t)i * Mp] = in ? in[i] : (real)0;
}

template <typename real>
struct Sensed {
  const SensArgs<real>& s;
  real bw[3], ba[3], bm[3];
  real hy[7], hb[3];                                           // the measurement of the last knot (latency = 1)
  TSAT_DEV explicit Sensed(const SensArgs<real>& s_) : s(s_) {}
  TSAT_DEV void load(int traj, int r) {
    const TSAT_GLOBAL real* p = (const TSAT_GLOBAL real*)(s.SN + (size_t)traj * SNW * s.Mp + r);
    const size_t ps = (size_t)s.Mp;
    for (int i = 0; i < 3; ++i) { bw[i] = p[(size_t)i * ps]; ba[i] = p[(size_t)(3 + i) * ps]; bm[i] = p[(size_t)(6 + i) * ps]; }
    for (int i = 0; i < 7; ++i) hy[i] = 0;
    for (int i = 0; i < 3; ++i) hb[i] = 0;
  }
  TSAT_DEV void commanded(int, const real*) {}                 // a measurement does not depend on the command
  TSAT_DEV void flown(const real*, const real*, const real*, const real*) {}   // nor on the rows the plant read
  // y: (w_m, q_m) of knot k, or of knot max(k - 1, 0)
  TSAT_DEV void state(long long gid, int k, bool noisy, const real x[7], real y[7]) {
    real nw[3] = {0, 0, 0}, na[3] = {0, 0, 0};
    if (noisy) {
      unsigned w0[4], w1[4];
      const unsigned ilo = (unsigned)((unsigned long long)gid & 0xFFFFFFFFull), ihi = (unsigned)((unsigned long long)gid >> 32);
      philox4x32_10(s.k0, s.k1, ilo, ihi, (unsigned)k, 16u, w0);
      philox4x32_10(s.k0, s.k1, ilo, ihi, (unsigned)k, 17u, w1);
      real z[6];
      box_muller<real>(w0[0], w0[1], z[0], z[1]);
      box_muller<real>(w0[2], w0[3], z[2], z[3]);
      box_muller<real>(w1[0], w1[1], z[4], z[5]);
      for (int i = 0; i < 3; ++i) { nw[i] = s.sgy * z[i]; na[i] = s.sat * z[3 + i]; }
    }
    real m[7];
    for (int i = 0; i < 3; ++i) {
      const real v = x[i] + bw[i];
      m[i] = v + nw[i];
    }
    real phi[3];
    for (int i = 0; i < 3; ++i) phi[i] = ba[i] + na[i];
    const real th = sqrt_(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    const real sr = sin_((real)0.5 * th) / th;
    const real sh = (th == 0) ? (real)0.5 : sr;
    const real ch = cos_((real)0.5 * th);
    const real d1 = phi[0] * sh, d2 = phi[1] * sh, d3 = phi[2] * sh;
    const real q0 = x[3], q1 = x[4], q2 = x[5], q3 = x[6];
    m[3] = q0 * ch - (q1 * d1 + q2 * d2 + q3 * d3);           // qmult(q, dq), the form of dyn_sim_h
    m[4] = q0 * d1 + ch * q1 + (q2 * d3 - q3 * d2);
    m[5] = q0 * d2 + ch * q2 + (q3 * d1 - q1 * d3);
    m[6] = q0 * d3 + ch * q3 + (q1 * d2 - q2 * d1);
    if (s.latency) {
      const bool old = k > 0;
      for (int i = 0; i < 7; ++i) { y[i] = old ? hy[i] : m[i]; hy[i] = m[i]; }
    } else {
      for (int i = 0; i < 7; ++i) y[i] = m[i];
    }
  }
  // B: b_m of knot k, or of knot max(k - 1, 0)
  TSAT_DEV void field(long long gid, int k, bool noisy, const real x[7], const real b0[3], real B[3]) {
    real nm[3] = {0, 0, 0};
    if (noisy) {
      unsigned w0[4];
      const unsigned ilo = (unsigned)((unsigned long long)gid & 0xFFFFFFFFull), ihi = (unsigned)((unsigned long long)gid >> 32);
      philox4x32_10(s.k0, s.k1, ilo, ihi, (unsigned)k, 20u, w0);
      real z[4];
      box_muller<real>(w0[0], w0[1], z[0], z[1]);
      box_muller<real>(w0[2], w0[3], z[2], z[3]);
      for (int i = 0; i < 3; ++i) nm[i] = s.smg * z[i];
    }
    real t[3], m[3];
    TrueState().field<real>(gid, k, noisy, x, b0, t);
    for (int i = 0; i < 3; ++i) {
      const real v = t[i] + bm[i];
      m[i] = v + nm[i];
    }
    if (s.latency) {
      const bool old = k > 0;
      for (int i = 0; i < 3; ++i) { B[i] = old ? hb[i] : m[i]; hb[i] = m[i]; }
    } else {
      for (int i = 0; i < 3; ++i) B[i] = m[i];
    }
  }
};

// What the sensed entry points reject besides what their parents reject, before anything is allocated or launched: "" or the
// reason, a non-finite bias with its (t, m)
inline std::string check_sensor(const tsat_sensor_options* s, const double* sensor, int64_t T, int32_t M) {
  if (!s) return "null sensor options";
  if (!std::isfinite(s->sigma_gyro) || !std::isfinite(s->sigma_att) || !std::isfinite(s->sigma_mag) || s->sigma_gyro < 0.0 ||
      s->sigma_att < 0.0 || s->sigma_mag < 0.0)
    return "sensor sigma_gyro, sigma_att and sigma_mag must be finite and >= 0";
  if (s->latency != 0 && s->latency != 1) return "sensor latency must be 0 (this knot's measurement) or 1 (the last knot's)";
  if (sensor)
    for (int64_t t = 0; t < T; ++t)
      for (int m = 0; m < M; ++m)
        for (int i = 0; i < SNW; ++i)
          if (!std::isfinite(sensor[((size_t)t * M + m) * SNW + i]))
            return "non-finite sensor entry at (t, m) = (" + std::to_string(t) + ", " + std::to_string(m) + ")";
  return "";
}

// TVLQR feedback on the plants of the dispersed call ...
template <typename real>
TSAT_DEV void sensed_tv_wave(const SensedTvArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.g.d);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, Sensed<real>(a.s));
}

// ... and of the gravity call, whatever gm is
template <typename real>
TSAT_DEV void sensed_tv_gg_wave(const SensedTvArgs<real>& a, int traj, int wave) {
  GgPlant<real> plant(a.g);
  ensemble_rollout<real>(a.g.d.e, plant, traj, wave, Sensed<real>(a.s));
}

// the PD law, likewise
template <typename real>
TSAT_DEV void sensed_pd_wave(const SensedPdArgs<real>& a, int traj, int wave) {
  DispersedPlant<real> plant(a.p.d);
  pd_rollout<real>(a.p, plant, traj, wave, Sensed<real>(a.s));
}

template <typename real>
TSAT_DEV void sensed_pd_gg_wave(const SensedPdArgs<real>& a, int traj, int wave) {
  const GgEnsArgs<real> g{a.p.d, a.p.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(a.p, plant, traj, wave, Sensed<real>(a.s));
}

}  // namespace tsat
