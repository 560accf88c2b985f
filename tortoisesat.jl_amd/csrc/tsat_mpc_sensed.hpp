// tsat_mpc_sensed.hpp — the held re-planning loop FED MEASUREMENTS (tsat_mpc_run_held_sensed, include/tortoise_hip.h): the loop of
// tsat_mpc_held.hpp / tsat_gg.hpp in which the solver and the gains no longer read the plant's true state. Every solve starts from
// a biased, noisy, optionally one-step-old measurement y, and the held steps evaluate U_j + K_j dx on y; the plant, the clip, the
// table clock, the plan shift and the statistic are the parent's and act on the TRUE state.
//
// What is new is one piece of state: the true state and the state the solver is given are two different things. While a call runs,
// P_X0 of the parameter record carries MEASUREMENTS (the solve reads its x0 there and nothing else has to know); the true state
// lives in a record of its own, component-major across trajectories like the hold record ([MSX_W][T]: rows 0..6 the true state,
// rows 7..13 the last raw measurement, which latency 1 hands to the next step — Sensed::hy saved and restored between launches).
// The last block of a call writes the true state back to P_X0, so the resident batch is left as tsat_mpc_run_held leaves it.
//
// The measurement is Sensed::state of tsat_sensed.hpp as it stands, on a [SNW][T] bias record (SensArgs.Mp = T, load(0, t)). Its
// Philox counter has to see the generator's knot step0 + s, its `k > 0` test for the old sample the step s RELATIVE TO THE CALL;
// one argument serves both because the two agree wherever the block calls it: it measures at s >= 1 only, where step0 + s > 0 as
// well (step0 >= 0 is validated). The measurement of s = 0, which has no older sample whatever step0 is, is made by the pack
// launch before the first solve, through a copy of the arguments with latency 0.
//
// The block below RESTATES mpc_held_block (tsat_mpc_held.hpp) rather than giving it a Sensor parameter, by the rule that header
// states for its own copies: the block differs in where the state is read from, what is written back and when a measurement is
// taken, and threading those through the parent would change the instruction streams of the four existing hold kernels
// (tools/isa_compare.py). Every piece of a step that is a function there is called here, not copied. What holds the copy to its
// original: the ideal sensor is tested equal to tsat_mpc_run_held and tsat_mpc_run_held_gg.
#pragma once
#include "tsat_sensed.hpp"

namespace tsat {

constexpr int MSX_X = 0;           // true state x[7]
constexpr int MSX_HY = 7;          // last raw measurement m[7]
constexpr int MSX_W = 14;

template <typename real>
struct MpcSensedArgs {
  MpcHeldArgs<real> h;   // the held loop's block, as it is
  const real* GT;        // [n_btab][n_tab][4] packed gravity rows, or null: the kernels without them
  SensArgs<real> s;      // SN [SNW][T], Mp = T; k0, k1 the plant noise's key
  real* XT;              // [MSX_W][T]
  real* HY;              // [T][n_steps][7]   y_s, the measurement step s's command or solve used
};

// What tsat_mpc_run_held_sensed rejects besides what its parents reject, before anything is allocated or launched: "" or the reason.
// One trajectory is one realisation (M = 1): a non-finite bias is reported with (t, 0).
inline std::string check_mpc_sensed(const tsat_sensor_options* s, const double* sensor, int64_t T, const double* Rtab, double gm) {
  if (!Rtab && !(gm == 0.0)) return "Rtab may be NULL only with gm == 0 (the kernel without the gravity rows)";
  return check_sensor(s, sensor, T, 1);
}

// thread t of the pack grid, before the first solve: the bias record of trajectory t (sensor 9 x T, or null: zeros), the true
// state moved to its own record, and m_0 — the first step of a call sees its own measurement — into P_X0 and the latency record
template <typename real>
TSAT_DEV void mpc_sensed_pack(const MpcSensedArgs<real>& a, const real* sensor, int64_t t) {
  const MpcArgs<real>& m = a.h.s.m;
  const EnsArgs<real>& e = a.h.s.d.e;
  const int64_t T = m.T;
  if (t >= T) return;
  sensed_pack<real>(sensor, (real*)a.s.SN, 1, (int)T, (int)T, t);         // 9 x T is the 9 x M x 1 layout with M = Mp = T
  SensArgs<real> s0 = a.s;
  s0.latency = 0;
  Sensed<real> sn(s0);
  sn.load(0, (int)t);
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  TSAT_GLOBAL real* xt = (TSAT_GLOBAL real*)(a.XT + t);
  const long long gid = e.nid0 ? e.nid0[t] : (long long)t;
  real x[7], y[7];
  for (int i = 0; i < 7; ++i) x[i] = Pg[P_X0 + i];
  sn.state(gid, (int)a.h.s.step0, a.h.s.noisy != 0, x, y);
  for (int i = 0; i < 7; ++i) {
    xt[(size_t)(MSX_X + i) * T] = x[i];
    xt[(size_t)(MSX_HY + i) * T] = y[i];
    Pg[P_X0 + i] = y[i];
  }
}

// trajectory t through the a.h.r control steps of its block: mpc_held_block with the command computed from y
template <typename real, int ES, typename Env>
TSAT_DEV void mpc_sensed_block(const MpcSensedArgs<real>& a, int t, const Env& env) {
  const MpcHeldArgs<real>& ha = a.h;
  const MpcArgs<real>& m = ha.s.m;
  const EnsArgs<real>& e = ha.s.d.e;
  const int NS = m.N;
  const size_t st = (size_t)m.T;
  const TSAT_GLOBAL real* hr = (const TSAT_GLOBAL real*)(ha.s.d.PL + t);
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  TSAT_GLOBAL real* xt = (TSAT_GLOBAL real*)(a.XT + t);
  Traj<real> tr = {};
  for (int i = 0; i < 7; ++i) tr.xf[i] = hr[(size_t)(HELD_XF + i) * st];
  tr.h = hr[(size_t)HELD_H * st]; tr.hh = (real)0.5 * tr.h; tr.us = m.us;
  tr.tau0 = (double)Pg[P_TAU0] + (double)Pg[P_TAU0L]; tr.dtau = (double)hr[(size_t)HELD_DTAU * st];
  tr.N = m.nk ? m.nk[t] : m.N; tr.n_tab = m.n_tab;
  tr.bt = (const TSAT_GLOBAL real*)(m.BT + (size_t)m.bidx[t] * m.n_tab * 4);
  DispersedPlant<real> plant(ha.s.d);
  mpc_held_load<real>(plant, tr, hr, st);
  const Traj<real>& tp = plant.traj(tr);
  const real cs = control_scale<real, 0>(tr);
  const TSAT_GLOBAL real* XUg = (const TSAT_GLOBAL real*)(m.XU + (size_t)t * NS * XUW);
  const TSAT_GLOBAL real* KDg = (const TSAT_GLOBAL real*)(ha.KD + (size_t)t * (NS - 1) * KDW);
  MpcDispRec rec = ha.s.rec[t];
  const bool noisy = ha.s.noisy != 0;
  const long long gid = e.nid0 ? e.nid0[t] : (long long)t;
  Sensed<real> sn(a.s);
  sn.load(0, t);
  real x[7], y[7];
  for (int i = 0; i < 7; ++i) {
    x[i] = xt[(size_t)(MSX_X + i) * st];
    sn.hy[i] = xt[(size_t)(MSX_HY + i) * st];
    y[i] = Pg[P_X0 + i];                                           // y of the block's first step: what the solve started from
  }
  mpc_held_tally<real>(m, t);                                     // the block's one solve
  real* hx = m.HX + ((size_t)t * (m.n_steps + 1) + m.step) * 7;
  real* hu = m.HU + ((size_t)t * m.n_steps + m.step) * 3;
  real* hy = a.HY + ((size_t)t * m.n_steps + m.step) * 7;
  TSAT_NO_UNROLL
  for (int j = 0; j < ha.r; ++j) {
    const int s = m.step + j;
    const int knot = (int)(ha.s.step0 + (long long)s);
    mpc_held_sample<real>(e, tr, x, s + 1, rec.first);             // the statistic judges the true state
    if (j > 0) sn.state(gid, knot, noisy, x, y);                   // s >= 1: the old sample exists, and knot > 0 says so
    real xu[XUW];
    for (int i = 0; i < XUW; ++i) xu[i] = XUg[(size_t)j * XUW + i];
    real v[3] = {xu[7], xu[8], xu[9]};
    if (j > 0 && ha.feedback) {                                    // the solver's policy around the plan, on the measurement
      real kd[21], dx[7];
      for (int i = 0; i < 21; ++i) kd[i] = KDg[(size_t)j * KDW + i];
      mpc_held_state_diff<real, ES>(y, xu, dx);
      for (int c = 0; c < 3; ++c) v[c] = mpc_held_feedback<real, ES>(v[c], kd, c, dx);
    }
    real uc[3], us[3], xn[7];
    for (int c = 0; c < 3; ++c) uc[c] = plant.command(c, v[c], cs);
    plant.actuate(uc, cs, us);
    const int i0 = brow_index(tr, 0, 0.0);
    const TSAT_GLOBAL real* p0 = tr.bt + (size_t)i0 * 4;
    const int i1 = brow_index(tr, 0, 0.5);
    const TSAT_GLOBAL real* p1 = tr.bt + (size_t)i1 * 4;
    const int i2 = brow_index(tr, 0, 1.0);
    const TSAT_GLOBAL real* p2 = tr.bt + (size_t)i2 * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    mpc_held_rk4<real>(tp, e, noisy, gid, knot, x, us, b0, b1, b2, env, i0, i1, i2, xn);
    for (int i = 0; i < 7; ++i) { hx[(size_t)j * 7 + i] = x[i]; hy[(size_t)j * 7 + i] = y[i]; x[i] = xn[i]; }
    for (int c = 0; c < 3; ++c) hu[(size_t)j * 3 + c] = uc[c];   // the limited command, units of u_scale
    tr.tau0 = tr.tau0 + tr.dtau;
  }
  rec.clipped += plant.clipped;
  Pg[P_TAU0] = (real)tr.tau0;
  if (m.step + ha.r == m.n_steps) {  // the call ends: the TRUE state goes back to the resident batch, then the record
    for (int i = 0; i < 7; ++i) { Pg[P_X0 + i] = x[i]; hx[(size_t)ha.r * 7 + i] = x[i]; }
    e.stats[t] = mpc_held_record<real>(e, tr, x, m.n_steps + 1, rec.first);
    if (ha.s.d.nclip) ha.s.d.nclip[t] = rec.clipped;
  } else {                           // the next solve starts from the measurement of the step it plans from
    sn.state(gid, (int)(ha.s.step0 + (long long)(m.step + ha.r)), noisy, x, y);
    for (int i = 0; i < 7; ++i) Pg[P_X0 + i] = y[i];
  }
  for (int i = 0; i < 7; ++i) {
    xt[(size_t)(MSX_X + i) * st] = x[i];
    xt[(size_t)(MSX_HY + i) * st] = sn.hy[i];
  }
  ha.s.rec[t] = rec;
}

// the four kernels' bodies: without and with the gravity rows of tsat_gg.hpp
template <typename real, int ES>
TSAT_DEV void mpc_sensed_traj(const MpcSensedArgs<real>& a, int t) {
  if (t >= a.h.s.m.T) return;
  mpc_sensed_block<real, ES>(a, t, NoEnv());
}

template <typename real, int ES>
TSAT_DEV void mpc_sensed_gg_traj(const MpcSensedArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_sensed_block<real, ES>(a, t, env);
}

}  // namespace tsat
