// tsat_dispersed.hpp — closed-loop tracking of a solved slew under an ensemble of DISPERSED PLANTS
// (tsat_tvlqr_ensemble_dispersed, include/tortoise_hip.h): the ensemble of tsat_ensemble.hpp in which every realisation has
// an inertia, an actuator matrix and a residual dipole of its own, and the feedback command is limited to a box.
//
// Lane = realisation, and the closed loop is ensemble_rollout of tsat_ensemble.hpp: this file holds what is the dispersed call's
// own — the record layout, the pack functions and DispersedPlant, the plant type that roll-out is instantiated with. What is the
// same for a slew — reference record, gain rows, field rows, the limits — stays wave-uniform (scalar loads); what belongs to
// the realisation is one packed record of PLW doubles per lane:
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

// The plant of a dispersed realisation for ensemble_rollout (tsat_ensemble.hpp; ModelPlant there says what each member answers).
template <typename real>
struct DispersedPlant {
  static constexpr int DIAGJ = 0;                              // the full-inertia instantiation, whatever the model's class
  const DispArgs<real>& d;
  Traj<real> tl;                                               // dyn_sim_h<real, 0> reads hh, J and hJi of it
  real lo[3], hi[3], G[9], mr[3];
  int hit = 0;
  int clipped = 0;                                             // knots at which the limits changed the command
  TSAT_DEV explicit DispersedPlant(const DispArgs<real>& d_) : d(d_) {}
  TSAT_DEV void load(const Traj<real>& tr, int traj, int r) {
    const TSAT_CONSTMEM real* sat = (const TSAT_CONSTMEM real*)(d.SAT + (size_t)traj * SATW);
    for (int c = 0; c < 3; ++c) { lo[c] = sat[c]; hi[c] = sat[3 + c]; }
    // the lane's own plant: one coalesced load per component, held for the whole roll-out
    const TSAT_GLOBAL real* pl = (const TSAT_GLOBAL real*)(d.PL + (size_t)traj * PLW * d.Mp + r);
    const size_t ps = (size_t)d.Mp;
    tl = tr;
    {
      const real j0 = pl[0], j1 = pl[ps], j2 = pl[2 * ps], j3 = pl[3 * ps], j4 = pl[4 * ps], j5 = pl[5 * ps];
      const real i0 = pl[6 * ps], i1 = pl[7 * ps], i2 = pl[8 * ps], i3 = pl[9 * ps], i4 = pl[10 * ps], i5 = pl[11 * ps];
      tl.J[0] = j0; tl.J[1] = j1; tl.J[2] = j2; tl.J[3] = j1; tl.J[4] = j3; tl.J[5] = j4; tl.J[6] = j2; tl.J[7] = j4; tl.J[8] = j5;
      tl.hJi[0] = i0; tl.hJi[1] = i1; tl.hJi[2] = i2; tl.hJi[3] = i1; tl.hJi[4] = i3; tl.hJi[5] = i4; tl.hJi[6] = i2; tl.hJi[7] = i4;
      tl.hJi[8] = i5;
    }
    for (int i = 0; i < 9; ++i) G[i] = pl[(size_t)(12 + i) * ps];
    for (int i = 0; i < 3; ++i) mr[i] = pl[(size_t)(21 + i) * ps];
  }
  TSAT_DEV const Traj<real>& traj(const Traj<real>&) const { return tl; }
  TSAT_DEV real command(int c, real v, real) {
    const real s = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);   // the actuator's box
    hit |= (s != v) ? 1 : 0;
    return s;
  }
  TSAT_DEV void actuate(const real uc[3], real cs, real us[3]) {
    clipped += hit;
    hit = 0;
    for (int c = 0; c < 3; ++c) us[c] = (G[3 * c] * uc[0] + G[3 * c + 1] * uc[1] + G[3 * c + 2] * uc[2] + mr[c]) * cs;
  }
  TSAT_DEV void disturb(const Traj<real>&, int, double, const real*, real*) const {}
  TSAT_DEV void store(size_t i) const {
    if (d.nclip) d.nclip[i] = clipped;
  }
};

template <typename real>
TSAT_DEV void dispersed_wave(const DispArgs<real>& d, int traj, int wave) {
  DispersedPlant<real> plant(d);
  ensemble_rollout<real>(d.e, plant, traj, wave);
}

}  // namespace tsat
