// tsat_gg.hpp — the dispersed ensemble and the held loop under GRAVITY-GRADIENT TORQUE (tsat_tvlqr_ensemble_gg,
// tsat_mpc_run_held_gg, include/tortoise_hip.h): the one external disturbance the plants of tsat_dispersed.hpp and
// tsat_mpc_held.hpp do not feel. The solver's model and the gains stay as they are — the torque is unmodelled on purpose.
//
// The orbit table Rtab (km, ECI) is indexed exactly like the field table: same btab_idx, same row floor(fma(c, dtau, tau))
// clamped. A pack launch (gg_pack_row, one thread per row) turns every row into four doubles [r^ (3), g = 3 gm / |r|^3], the row
// width of the field rows. In every RK4 stage of a plant step, after dyn_sim_h has produced the stage's increment k from the stage
// state x (as integrated, before the noise injection):
//   r_b  = qrot(x[3:7] / |x[3:7]|, r^)        the rotation dyn_h gives the field row
//   tau  = g (r_b x (Jp r_b))                  Jp: the realisation's inertia
//   k[0:3] += (h inv(Jp)) tau
// (gg_stage). It is additive and placed after dyn_sim_h so that dyn_h, dyn_sim_h and every kernel built on them stay untouched;
// g = 0 adds a zero to each of the three components, so gm = 0 repeats the parent kernel's states bit for bit.
//
// Ensemble (lane = realisation): GgPlant is DispersedPlant with the `disturb` hook of ensemble_rollout filled in. The gravity
// rows of a slew are wave-uniform like its field rows — scalar loads through TSAT_UNIFORM_INT(brow_index(...)), one row where
// its stage uses it, none held across the step. Hold (lane = trajectory): GgEnv is the `env` of mpc_held_block; the rows are
// the lane's own vector loads beside its field rows, at the indices the field rows were read at.
#pragma once
#include "tsat_mpc_held.hpp"

namespace tsat {

template <typename real>
struct GgEnsArgs {
  DispArgs<real> d;      // the dispersed ensemble's block, as it is
  const real* GT;        // [n_btab][n_tab][4]   packed gravity rows
};

template <typename real>
struct MpcHeldGgArgs {
  MpcHeldArgs<real> h;   // the held loop's block, as it is
  const real* GT;        // [n_btab][n_tab][4]   packed gravity rows, beside h.s.m.BT
};

// thread e of the pack grid: orbit row e (3 doubles, km) -> [r^, 3 gm / |r|^3]
template <typename real>
TSAT_DEV void gg_pack_row(const real* R, real gm, real* GT, int64_t rows, int64_t e) {
  if (e >= rows) return;
  const TSAT_GLOBAL real* r = (const TSAT_GLOBAL real*)(R + (size_t)e * 3);
  TSAT_GLOBAL real* o = (TSAT_GLOBAL real*)(GT + (size_t)e * 4);
  const real x = r[0], y = r[1], z = r[2];
  const real n2 = x * x + y * y + z * z;
  const real n = sqrt_(n2);
  o[0] = x / n; o[1] = y / n; o[2] = z / n;
  o[3] = ((real)3 * gm) / (n2 * n);
}

// the gravity-gradient increment of one RK4 stage: x the stage state, g its packed row (scalar or vector loads: Row is the
// pointer type), k the increment dyn_sim_h has just written. Reads J and hJi of the plant's Traj, like dyn_h<real, 0>.
template <typename real, typename Row>
TSAT_DEV void gg_stage(const Traj<real>& tp, const real x[7], Row g, real k[7]) {
  const real rn = rsqrt_<real>(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
  const real q0 = x[3] * rn, q1 = x[4] * rn, q2 = x[5] * rn, q3 = x[6] * rn;
  const real a0 = g[0], a1 = g[1], a2 = g[2], gg = g[3];
  // r_b = qrot(q, r^) = r^ + 2 v x (v x r^ + s r^), as dyn_h rotates b
  const real c0 = (q2 * a2 - q3 * a1) + q0 * a0;
  const real c1 = (q3 * a0 - q1 * a2) + q0 * a1;
  const real c2 = (q1 * a1 - q2 * a0) + q0 * a2;
  const real r0 = a0 + 2 * (q2 * c2 - q3 * c1);
  const real r1 = a1 + 2 * (q3 * c0 - q1 * c2);
  const real r2 = a2 + 2 * (q1 * c1 - q2 * c0);
  const real Jr0 = tp.J[0] * r0 + tp.J[1] * r1 + tp.J[2] * r2;
  const real Jr1 = tp.J[3] * r0 + tp.J[4] * r1 + tp.J[5] * r2;
  const real Jr2 = tp.J[6] * r0 + tp.J[7] * r1 + tp.J[8] * r2;
  const real t0 = gg * (r1 * Jr2 - r2 * Jr1);
  const real t1 = gg * (r2 * Jr0 - r0 * Jr2);
  const real t2 = gg * (r0 * Jr1 - r1 * Jr0);
  k[0] = k[0] + (tp.hJi[0] * t0 + tp.hJi[1] * t1 + tp.hJi[2] * t2);
  k[1] = k[1] + (tp.hJi[3] * t0 + tp.hJi[4] * t1 + tp.hJi[5] * t2);
  k[2] = k[2] + (tp.hJi[6] * t0 + tp.hJi[7] * t1 + tp.hJi[8] * t2);
}

// The plant of a realisation of tsat_tvlqr_ensemble_gg for ensemble_rollout: DispersedPlant flying through the slew's gravity
// rows. Slot M (the noise-free realisation) holds the model's inertia, so stats_nominal feels the torque with Jmat.
template <typename real>
struct GgPlant : DispersedPlant<real> {
  const real* GT;
  const TSAT_CONSTMEM real* gt = nullptr;                      // the slew's table: follows btab_idx like the field rows
  TSAT_DEV explicit GgPlant(const GgEnsArgs<real>& g) : DispersedPlant<real>(g.d), GT(g.GT) {}
  TSAT_DEV void load(const Traj<real>& tr, int traj, int r) {
    DispersedPlant<real>::load(tr, traj, r);
    gt = (const TSAT_CONSTMEM real*)(GT + (size_t)this->d.e.bidx[traj] * tr.n_tab * 4);
  }
  TSAT_DEV void disturb(const Traj<real>& tr, int k, double c, const real x[7], real kk[7]) const {
    gg_stage<real>(this->tl, x, gt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, c)) * 4, kk);
  }
};

template <typename real>
TSAT_DEV void gg_wave(const GgEnsArgs<real>& g, int traj, int wave) {
  GgPlant<real> plant(g);
  ensemble_rollout<real>(g.d.e, plant, traj, wave);
}

// the `env` of mpc_held_block under gravity gradient: the lane's own table, rows at the indices of its field rows
template <typename real>
struct GgEnv {
  const TSAT_GLOBAL real* gt;
  TSAT_DEV void stage(const Traj<real>& tp, int row, const real x[7], real k[7]) const {
    gg_stage<real>(tp, x, gt + (size_t)row * 4, k);
  }
};

// trajectory t through the control steps of its block, the torque in every plant step
template <typename real, int ES>
TSAT_DEV void mpc_held_gg_block(const MpcHeldGgArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_held_block<real, ES>(a.h, t, env);
}

}  // namespace tsat
