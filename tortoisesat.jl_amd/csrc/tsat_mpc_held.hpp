// tsat_mpc_held.hpp — the receding-horizon loop that RE-PLANS EVERY R CONTROL STEPS and flies the solver's own gains in between
// (tsat_mpc_run_held, include/tortoise_hip.h): after a solve of the resident batch, a block of r <= R control steps of the noisy,
// dispersed plant of tsat_mpc_dispersed.hpp under the plan just solved — step 0 applies U[0], step j > 0 the iLQR policy
// U[j] + K[j] dx around the plan (or U[j] alone: the open-loop hold) —, then the plan shifted by r knots as the next warm start.
//
// Lane = trajectory: ceil(T / 64) wavefronts, every lane rolls its own trajectory through the block's steps, the mapping of the
// ensemble roll-out (tsat_ensemble.hpp) with nothing wave-uniform left: plan and gain records, field rows, limits, xf, the table
// clock and the generator id all belong to the lane. What a lane reads once per block is one record of HELD_W doubles stored
// component-major across trajectories ([HELD_W][T]: a wave's load of one component is one contiguous access), made once per call
// by mpc_held_pack: the packed plant of dispersed_pack_record, the limits, xf, dt and dtau. x0 and tau0 live in the parameter
// record the solve reads them from and are advanced there. No LDS, no barrier.
//
// The step is the every-step loop's: the pieces of tsat_mpc_dispersed.hpp (mpc_sample, mpc_rk4, mpc_record, mpc_tally) around
// DispersedPlant, so replan_every = 1 repeats tsat_mpc_run_dispersed operation for operation; dx and the gain product are the
// forward sweeps' policy (mpc_held_state_diff, mpc_held_feedback below). The table clock advances by one rounded addition per step,
// tau <- tau + dtau, and the rows of a step are those of brow_index at knot 0 of the current clock — the clock the every-step loop
// has at that step. mpc_held_block is the one block of every held loop: what acts on the body is its Env (NoEnv; GgEnv of
// tsat_gg.hpp), what the controller is fed its Feed (TrueFeed; SensedFeed of tsat_mpc_sensed.hpp; FilteredFeed of tsat_mpc_filtered.hpp;
// ModelFilteredFeed of tsat_mpc_model_filtered.hpp).
#pragma once
#include "tsat_mpc_dispersed.hpp"

namespace tsat {

// the per-trajectory record of the hold: PLW plant components, then
constexpr int HELD_SAT = PLW;              // lo[3], hi[3]
constexpr int HELD_XF = HELD_SAT + SATW;   // xf[7]
constexpr int HELD_H = HELD_XF + 7;        // dt
constexpr int HELD_DTAU = HELD_H + 1;      // dtau
constexpr int HELD_W = HELD_DTAU + 1;

template <typename real>
struct MpcHeldArgs {
  // the every-step loop's block with: s.m.step = first control step of this launch's block, s.d.PL = the records [HELD_W][T],
  // s.d.SAT = the limits [T][SATW] as uploaded (read by the pack only)
  MpcDispArgs<real> s;
  const real* KD;        // [T][N-1][24]   gains of the plan just solved
  int r;                 // control steps of this block
  int feedback;          // 1: U[j] + K[j] dx at j > 0; 0: U[j]
};

// thread t of the pack grid: record t (plant == null: the model's plant) and the zeroed running record
template <typename real>
TSAT_DEV void mpc_held_pack(const real* plant, const real* P, const real* SAT, real us, real* HR, MpcDispRec* rec, int64_t T, int64_t t) {
  if (t >= T) return;
  const size_t st = (size_t)T;
  const TSAT_GLOBAL real* pl = plant ? (const TSAT_GLOBAL real*)(plant + (size_t)t * TSAT_PLANT_W) : nullptr;
  const TSAT_GLOBAL real* p = (const TSAT_GLOBAL real*)(P + (size_t)t * PSTRIDE);
  TSAT_GLOBAL real* out = (TSAT_GLOBAL real*)(HR + t);
  dispersed_pack_record<real>(pl, p, us, out, st);
  for (int i = 0; i < SATW; ++i) out[(size_t)(HELD_SAT + i) * st] = SAT[(size_t)t * SATW + i];
  for (int i = 0; i < 7; ++i) out[(size_t)(HELD_XF + i) * st] = p[P_XF + i];
  out[(size_t)HELD_H * st] = p[P_DT];
  out[(size_t)HELD_DTAU * st] = (real)((double)p[P_DTAU] + (double)p[P_DTAUL]);
  rec[t].first = 0;
  rec[t].clipped = 0;
}

// the lane's plant and limits from its record (what DispersedPlant::load takes from the ensemble's layout)
template <typename real>
TSAT_DEV void mpc_held_load(DispersedPlant<real>& pl, const Traj<real>& tr, const TSAT_GLOBAL real* hr, size_t st) {
  pl.tl = tr;
  const real j0 = hr[0], j1 = hr[st], j2 = hr[2 * st], j3 = hr[3 * st], j4 = hr[4 * st], j5 = hr[5 * st];
  const real i0 = hr[6 * st], i1 = hr[7 * st], i2 = hr[8 * st], i3 = hr[9 * st], i4 = hr[10 * st], i5 = hr[11 * st];
  pl.tl.J[0] = j0; pl.tl.J[1] = j1; pl.tl.J[2] = j2; pl.tl.J[3] = j1; pl.tl.J[4] = j3; pl.tl.J[5] = j4;
  pl.tl.J[6] = j2; pl.tl.J[7] = j4; pl.tl.J[8] = j5;
  pl.tl.hJi[0] = i0; pl.tl.hJi[1] = i1; pl.tl.hJi[2] = i2; pl.tl.hJi[3] = i1; pl.tl.hJi[4] = i3; pl.tl.hJi[5] = i4;
  pl.tl.hJi[6] = i2; pl.tl.hJi[7] = i4; pl.tl.hJi[8] = i5;
  for (int i = 0; i < 9; ++i) pl.G[i] = hr[(size_t)(12 + i) * st];
  for (int i = 0; i < 3; ++i) pl.mr[i] = hr[(size_t)(21 + i) * st];
  for (int c = 0; c < 3; ++c) { pl.lo[c] = hr[(size_t)(HELD_SAT + c) * st]; pl.hi[c] = hr[(size_t)(HELD_SAT + 3 + c) * st]; }
}

// The iLQR policy of the forward sweeps at a knot (forward_sweep, tsat_device.hpp; forward_sweep_packed, tsat_packed.hpp) at
// alpha = 0: the state difference the gains act on, and component c of u + K dx — the sum starts from u, columns ascending.
// x: the flown state; xu: the plan's record; kd: the knot's gains, rows of 7.
template <typename real, int ES>
TSAT_DEV void mpc_held_state_diff(const real x[7], const real xu[XUW], real dx[7]) {
  if (ES) {
    // quaternion_error(new, nominal) = [dw; MRP(q_nom^-1 (x) q_new)]  (src/quaternion_toolbox.jl:58-75)
    for (int i = 0; i < 3; ++i) dx[i] = x[i] - xu[i];
    const real s1 = xu[3], a1 = -xu[4], a2 = -xu[5], a3 = -xu[6];   // conjugate of the nominal quaternion
    const real s2 = x[3], b1 = x[4], b2 = x[5], b3 = x[6];
    const real e0 = s1 * s2 - (a1 * b1 + a2 * b2 + a3 * b3);
    const real e1 = s1 * b1 + s2 * a1 + (a2 * b3 - a3 * b2);
    const real e2 = s1 * b2 + s2 * a2 + (a3 * b1 - a1 * b3);
    const real e3 = s1 * b3 + s2 * a3 + (a1 * b2 - a2 * b1);
    const real ir = rcp_((real)1 + e0);
    dx[3] = e1 * ir; dx[4] = e2 * ir; dx[5] = e3 * ir; dx[6] = 0;
  } else {
    for (int i = 0; i < 7; ++i) dx[i] = x[i] - xu[i];
  }
}
template <typename real, int ES>
TSAT_DEV real mpc_held_feedback(real u, const real kd[21], int c, const real dx[7]) {
  real v = u;
  for (int j = 0; j < BwdCfg<ES>::NH; ++j) v += kd[c * 7 + j] * dx[j];
  return v;
}

// What the controller is fed, as Env answers what acts on the body: the state y the gains act on (`sn`, a Sensor of
// ensemble_rollout: y = sn.state(x) at every step after a block's first) and the x0 a solve starts from, which P_X0 carries between
// launches. TrueFeed: both are the plant's true state. SensedFeed of tsat_mpc_sensed.hpp: measurements.
// Every step tells the sensor what it flies, `sn.flown(uc, b0, b1, b2)`: the limited command and the field rows the plant's step
// reads — the hook beside the roll-outs' `commanded`, for a sensor that models the plant (HeldModelFiltered); empty for the others.
struct TrueFeed {
  TrueState sn;
  // the block begins: the true state, and the y of its first step
  template <typename real>
  TSAT_DEV void load(const TSAT_GLOBAL real* Pg, real x[7], real y[7]) {
    for (int i = 0; i < 7; ++i) y[i] = x[i] = Pg[P_X0 + i];
  }
  // y of step j of the block, for a history of its own
  template <typename real>
  TSAT_DEV void row(int, const real*) {}
  // the block ends in the true state x: what the next solve starts from (`last`: none follows in this call; knot: its step)
  // the block ends in the true state x: what the next solve starts from (y: room for it)
  template <typename real>
  TSAT_DEV const real* next(long long, bool, const real x[7], real*) { return x; }
};

// trajectory t through the a.r control steps of its block
template <typename real, int ES, typename Env = NoEnv, typename Feed = TrueFeed>
TSAT_DEV void mpc_held_block(const MpcHeldArgs<real>& a, int t, const Env& env = Env(), Feed feed = Feed()) {
  const MpcArgs<real>& m = a.s.m;
  const EnsArgs<real>& e = a.s.d.e;
  if (t >= m.T) return;
  const int NS = m.N;
  const size_t st = (size_t)m.T;
  const TSAT_GLOBAL real* hr = (const TSAT_GLOBAL real*)(a.s.d.PL + t);
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  // what the step reads of the slew's constants: xf, dt, the table clock and the table; inertia and h inv(J) are the plant's
  Traj<real> tr = {};
  for (int i = 0; i < 7; ++i) tr.xf[i] = hr[(size_t)(HELD_XF + i) * st];
  tr.h = hr[(size_t)HELD_H * st]; tr.hh = (real)0.5 * tr.h; tr.us = m.us;
  tr.tau0 = (double)Pg[P_TAU0] + (double)Pg[P_TAU0L]; tr.dtau = (double)hr[(size_t)HELD_DTAU * st];
  tr.N = m.nk ? m.nk[t] : m.N; tr.n_tab = m.n_tab;
  tr.bt = (const TSAT_GLOBAL real*)(m.BT + (size_t)m.bidx[t] * m.n_tab * 4);
  DispersedPlant<real> plant(a.s.d);
  mpc_held_load<real>(plant, tr, hr, st);
  const Traj<real>& tp = plant.traj(tr);
  const real cs = control_scale<real, 0>(tr);
  const TSAT_GLOBAL real* XUg = (const TSAT_GLOBAL real*)(m.XU + (size_t)t * NS * XUW);
  const TSAT_GLOBAL real* KDg = (const TSAT_GLOBAL real*)(a.KD + (size_t)t * (NS - 1) * KDW);
  MpcDispRec rec = a.s.rec[t];
  const bool noisy = a.s.noisy != 0;
  const long long gid = e.nid0 ? e.nid0[t] : (long long)t;
  real x[7], y[7];
  feed.load(Pg, x, y);
  mpc_tally<real>(m, t);                                     // the block's one solve
  real* hx = m.HX + ((size_t)t * (m.n_steps + 1) + m.step) * 7;
  real* hu = m.HU + ((size_t)t * m.n_steps + m.step) * 3;
  TSAT_NO_UNROLL
  for (int j = 0; j < a.r; ++j) {
    const int s = m.step + j;
    const int knot = (int)(a.s.step0 + (long long)s);
    mpc_sample<real>(e, tr, x, s + 1, rec.first);                  // the statistic judges the true state
    real xu[XUW];
    for (int i = 0; i < XUW; ++i) xu[i] = XUg[(size_t)j * XUW + i];
    real v[3] = {xu[7], xu[8], xu[9]};
    if (j > 0) feed.sn.state(gid, knot, noisy, x, y);              // s >= 1: an older sample exists, and knot > 0 says so
    if (j > 0 && a.feedback) {                                   // the solver's policy around the plan, alpha = 0
      real kd[21], dx[7];
      for (int i = 0; i < 21; ++i) kd[i] = KDg[(size_t)j * KDW + i];
      mpc_held_state_diff<real, ES>(y, xu, dx);
      for (int c = 0; c < 3; ++c) v[c] = mpc_held_feedback<real, ES>(v[c], kd, c, dx);
    }
    real uc[3], us[3], xn[7];
    for (int c = 0; c < 3; ++c) uc[c] = plant.command(c, v[c], cs);
    plant.actuate(uc, cs, us);
    // rows at tau, tau + dtau / 2, tau + dtau of the current table clock (index, pointer, index, pointer, ...: with the three
    // indices taken first the kernel keeps its length but not its register assignment — tools/isa_compare.py)
    const int i0 = brow_index(tr, 0, 0.0);
    const TSAT_GLOBAL real* p0 = tr.bt + (size_t)i0 * 4;
    const int i1 = brow_index(tr, 0, 0.5);
    const TSAT_GLOBAL real* p1 = tr.bt + (size_t)i1 * 4;
    const int i2 = brow_index(tr, 0, 1.0);
    const TSAT_GLOBAL real* p2 = tr.bt + (size_t)i2 * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    feed.sn.flown(uc, b0, b1, b2);                               // what this step flies, for a sensor that models the plant
    mpc_rk4<real>(tp, e, noisy, gid, knot, x, us, b0, b1, b2, env, i0, i1, i2, xn);
    for (int i = 0; i < 7; ++i) { hx[(size_t)j * 7 + i] = x[i]; x[i] = xn[i]; }
    feed.row(j, y);
    for (int c = 0; c < 3; ++c) hu[(size_t)j * 3 + c] = uc[c];   // the limited command, units of u_scale
    tr.tau0 = tr.tau0 + tr.dtau;
  }
  rec.clipped += plant.clipped;
  const real* x0 = feed.next(gid, noisy, x, y);
  for (int i = 0; i < 7; ++i) Pg[P_X0 + i] = x0[i];
  Pg[P_TAU0] = (real)tr.tau0;
  if (m.step + a.r == m.n_steps) {  // last sample j = n_steps + 1, then the record
    for (int i = 0; i < 7; ++i) hx[(size_t)a.r * 7 + i] = x[i];
    e.stats[t] = mpc_record<real>(e, tr, x, m.n_steps + 1, rec.first);
    if (a.s.d.nclip) a.s.d.nclip[t] = rec.clipped;
  }
  a.s.rec[t] = rec;
}

// wavefront `traj` of the shift grid, lanes = knots: the next warm start is the plan shifted by the block's r knots inside the
// trajectory's own horizon, last control repeated. Reads XU alone, which the hold does not write.
template <typename real>
TSAT_DEV void mpc_held_shift(const MpcArgs<real>& m, int r, int traj) {
  const int lane = TSAT_LANE();
  const int NS = m.N;
  const int N = m.nk ? m.nk[traj] : m.N;
  const TSAT_GLOBAL real* XUg = (const TSAT_GLOBAL real*)(m.XU + (size_t)traj * NS * XUW);
  TSAT_GLOBAL real* U0g = (TSAT_GLOBAL real*)(m.U0 + (size_t)traj * (NS - 1) * 3);
  for (int k = lane; k < N - 1; k += WAVE) {
    const int src = (k + r < N - 1) ? k + r : N - 2;
    for (int c = 0; c < 3; ++c) U0g[(size_t)k * 3 + c] = XUg[(size_t)src * XUW + 7 + c];
  }
}

}  // namespace tsat
