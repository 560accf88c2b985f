// tsat_dispersed.hpp — closed-loop tracking of a solved slew under an ensemble of DISPERSED PLANTS
// (tsat_tvlqr_ensemble_dispersed, include/tortoise_hip.h): the ensemble of tsat_ensemble.hpp in which every realisation has
// an inertia, an actuator matrix and a residual dipole of its own, and the feedback command is limited to a box.
//
// Lane = realisation, as in ensemble_wave. What is the same for a slew — reference record, gain rows, field rows, the limits —
// stays wave-uniform (scalar loads); what belongs to the realisation is one packed record of PLW doubles per lane:
//   [0..5]   Jp, upper triangle (00 01 02 11 12 22)          [6..11]  h inv(Jp), the same six
//   [12..20] G, row-major                                    [21..23] m_res / u_scale
// stored component-major, [T][PLW][Mp] with Mp = 64 * waves per slew: a wave's load of one component is one coalesced 512-byte
// access. Slot M of every slew holds the MODEL plant (Jmat, G = I, m_res = 0) for the noise-free realisation. The records are
// made on the device (dispersed_pack_record: closed-form adjugate inverse, one thread per realisation).
//
// The plant, the generator and the table clock are the device functions the nominal kernel uses: dyn_sim_h<real, 0> reads from
// its Traj only hh (wave-uniform), J and hJi, so a per-lane Traj with the full-inertia instantiation reuses them unchanged.
// Per knot: u_cmd = U - K dX, u_sat = clip(u_cmd, lo, hi), applied dipole (units of u_scale) = G u_sat + m_res / u_scale for
// all four stages.
#pragma once
#include "tsat_ensemble.hpp"

namespace tsat {

constexpr int PLW = 24;          // doubles of a packed per-lane plant record
constexpr int SATW = 6;          // limits of a slew: lo[3], hi[3] (+-inf when the call gives none)

template <typename real>
struct DispArgs {
  EnsArgs<real> e;
  const real* PL;    // [T][PLW][Mp]   packed plants, slot M = the model's
  int Mp;            // 64 * ensemble_waves(M)
  const real* SAT;   // [T][SATW]
  int* nclip;        // [T][M] clipped knots of every realisation, or null
};

// one packed record from a realisation's 21 doubles (Jp 9 column-major, G 9 column-major, m_res 3), or — pl == null — the
// model's plant from the slew's parameter record. `out` is the record's first component, `stride` the distance between components.
template <typename real>
TSAT_DEV void dispersed_pack_record(const TSAT_GLOBAL real* pl, const TSAT_GLOBAL real* p, real us, TSAT_GLOBAL real* out, size_t stride) {
  const real h = p[P_DT];
  real v[PLW];
  if (pl) {
    const real a = pl[0], b = pl[3], c = pl[6], d = pl[4], e = pl[7], f = pl[8];      // upper triangle of the symmetric Jp
    const real A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d;
    const real A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
    const real det = a * A00 + (b * A01 + c * A02);
    v[0] = a; v[1] = b; v[2] = c; v[3] = d; v[4] = e; v[5] = f;
    v[6] = h * (A00 / det); v[7] = h * (A01 / det); v[8] = h * (A02 / det);
    v[9] = h * (A11 / det); v[10] = h * (A12 / det); v[11] = h * (A22 / det);
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) v[12 + 3 * r + cc] = pl[9 + 3 * cc + r];
    for (int i = 0; i < 3; ++i) v[21 + i] = pl[18 + i] / us;
  } else {
    const int tri[6] = {0, 1, 2, 4, 5, 8};
    for (int i = 0; i < 6; ++i) { v[i] = p[P_J + tri[i]]; v[6 + i] = h * p[P_JI + tri[i]]; }
    for (int i = 0; i < 9; ++i) v[12 + i] = (i == 0 || i == 4 || i == 8) ? (real)1 : (real)0;
    for (int i = 0; i < 3; ++i) v[21 + i] = 0;
  }
  for (int i = 0; i < PLW; ++i) out[(size_t)i * stride] = v[i];
}

// thread e of the pack grid: realisation e % (M + 1) of slew e / (M + 1); the last one of a slew is the model's plant
template <typename real>
TSAT_DEV void dispersed_pack(const real* plant, const real* P, real us, real* PL, int64_t T, int M, int Mp, int64_t e) {
  if (e >= T * (int64_t)(M + 1)) return;
  const int64_t t = e / (M + 1);
  const int m = (int)(e - t * (M + 1));
  const TSAT_GLOBAL real* pl = (m < M) ? (const TSAT_GLOBAL real*)(plant + ((size_t)t * M + m) * TSAT_PLANT_W) : nullptr;
  dispersed_pack_record<real>(pl, (const TSAT_GLOBAL real*)(P + (size_t)t * PSTRIDE), us,
                              (TSAT_GLOBAL real*)(PL + (size_t)t * PLW * Mp + m), (size_t)Mp);
}

template <typename real>
TSAT_DEV void dispersed_wave(const DispArgs<real>& d, int traj, int wave) {
  const EnsArgs<real>& a = d.e;
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
  const TSAT_CONSTMEM real* xu = (const TSAT_CONSTMEM real*)(a.XUR + (size_t)traj * NS * XUW);
  const TSAT_CONSTMEM real* kdg = (const TSAT_CONSTMEM real*)(a.KD + (size_t)traj * (NS - 1) * KDW);
  const TSAT_CONSTMEM real* bt = (const TSAT_CONSTMEM real*)(a.BT + (size_t)a.bidx[traj] * n_tab * 4);
  const TSAT_CONSTMEM real* sat = (const TSAT_CONSTMEM real*)(d.SAT + (size_t)traj * SATW);
  const Traj<real> tr = ensemble_traj<real>(Pc, a.us, N, n_tab);
  const real lo[3] = {sat[0], sat[1], sat[2]}, hi[3] = {sat[3], sat[4], sat[5]};
  // the lane's own plant: one coalesced load per component, held for the whole roll-out
  const TSAT_GLOBAL real* pl = (const TSAT_GLOBAL real*)(d.PL + (size_t)traj * PLW * d.Mp + r);
  const size_t ps = (size_t)d.Mp;
  Traj<real> tl = tr;                                          // dyn_sim_h<real, 0> reads hh, J and hJi of it
  {
    const real j0 = pl[0], j1 = pl[ps], j2 = pl[2 * ps], j3 = pl[3 * ps], j4 = pl[4 * ps], j5 = pl[5 * ps];
    const real i0 = pl[6 * ps], i1 = pl[7 * ps], i2 = pl[8 * ps], i3 = pl[9 * ps], i4 = pl[10 * ps], i5 = pl[11 * ps];
    tl.J[0] = j0; tl.J[1] = j1; tl.J[2] = j2; tl.J[3] = j1; tl.J[4] = j3; tl.J[5] = j4; tl.J[6] = j2; tl.J[7] = j4; tl.J[8] = j5;
    tl.hJi[0] = i0; tl.hJi[1] = i1; tl.hJi[2] = i2; tl.hJi[3] = i1; tl.hJi[4] = i3; tl.hJi[5] = i4; tl.hJi[6] = i2; tl.hJi[7] = i4;
    tl.hJi[8] = i5;
  }
  real G[9], mr[3];
  for (int i = 0; i < 9; ++i) G[i] = pl[(size_t)(12 + i) * ps];
  for (int i = 0; i < 3; ++i) mr[i] = pl[(size_t)(21 + i) * ps];
  const long long gid = (a.nid0 ? a.nid0[traj] : (long long)traj * (long long)M) + (long long)r;
  TSAT_GLOBAL real* xs = (a.XS && live && noisy) ? (TSAT_GLOBAL real*)(a.XS + ((size_t)traj * M + r) * NS * 7) : nullptr;
  real x[7];
  if (noisy) {
    const TSAT_GLOBAL real* x0 = (const TSAT_GLOBAL real*)(a.X0 + ((size_t)traj * M + r) * 7);
    for (int i = 0; i < 7; ++i) x[i] = x0[i];
  } else {
    for (int i = 0; i < 7; ++i) x[i] = xu[i];
  }
  const real cs = control_scale<real, 0>(tr);
  int first = 0;                                               // the statistic, evaluated while the roll-out runs
  int clipped = 0;                                             // knots at which the limits changed the command
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
    const TSAT_CONSTMEM real* xr = xu + (size_t)k * XUW;
    const TSAT_CONSTMEM real* kd = kdg + (size_t)k * KDW;
    real dX[6];
    for (int i = 0; i < 3; ++i) dX[i] = x[i] - xr[i];
    {  // vector part of q_ref^-1 (x) q_sim  (src/attitude_controller.jl:42)
      const real s1 = xr[3], a1 = -xr[4], a2 = -xr[5], a3 = -xr[6];
      dX[3] = s1 * x[4] + x[3] * a1 + (a2 * x[6] - a3 * x[5]);
      dX[4] = s1 * x[5] + x[3] * a2 + (a3 * x[4] - a1 * x[6]);
      dX[5] = s1 * x[6] + x[3] * a3 + (a1 * x[5] - a2 * x[4]);
    }
    real uc[3];
    int hit = 0;
    for (int c = 0; c < 3; ++c) {
      real v = xr[7 + c];
      for (int j = 0; j < 6; ++j) v += kd[c * 7 + j] * dX[j];   // kd = -K_lqr
      const real s = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);   // the actuator's box
      hit |= (s != v) ? 1 : 0;
      uc[c] = s;
    }
    clipped += hit;
    real us[3];
    for (int c = 0; c < 3; ++c) us[c] = (G[3 * c] * uc[0] + G[3 * c + 1] * uc[1] + G[3 * c + 2] * uc[2] + mr[c]) * cs;
    // rows at tau, tau + dtau/2, tau + dtau: wave-uniform indices, said so (the clock is fp64 arithmetic on the vector unit)
    const TSAT_CONSTMEM real* p0 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.0)) * 4;
    const TSAT_CONSTMEM real* p1 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.5)) * 4;
    const TSAT_CONSTMEM real* p2 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 1.0)) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    real k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
    for (int i = 0; i < 9; ++i) nz[i] = 0;
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 0, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, 0>(tl, x, us, b0, noisy, nz, k1);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 1, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, 0>(tl, t, us, b1, noisy, nz, k2);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 2, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, 0>(tl, t, us, b1, noisy, nz, k3);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 3, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, 0>(tl, t, us, b2, noisy, nz, k4);
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
      if (d.nclip) d.nclip[(size_t)traj * M + r] = clipped;
    } else {
      a.stats_nom[traj] = st;
    }
  }
}

}  // namespace tsat
