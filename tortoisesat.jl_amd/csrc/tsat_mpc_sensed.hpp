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
// The block is mpc_held_block itself (tsat_mpc_held.hpp) with SensedFeed below as its Feed, as GgEnv is its Env.
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

// The Feed of mpc_held_block (tsat_mpc_held.hpp) that hands the controller measurements: `sn` is the sensor of trajectory t with
// its latency record restored, the true state comes from and goes back to XT, every step's y goes to HY, and P_X0 carries the
// measurement the next solve starts from until the call's last block puts the true state back.
template <typename real>
struct SensedFeed {
  const MpcHeldArgs<real>& h;
  Sensed<real> sn;
  TSAT_GLOBAL real* xt;      // the trajectory's column of XT, stride st
  const size_t st;
  real* hy;                  // its row of HY at the block's first step
  TSAT_DEV SensedFeed(const MpcSensedArgs<real>& a, int t)
      : h(a.h), sn(a.s), xt((TSAT_GLOBAL real*)(a.XT + t)), st((size_t)a.h.s.m.T),
        hy(a.HY + ((size_t)t * a.h.s.m.n_steps + a.h.s.m.step) * 7) {
    sn.load(0, t);
  }
  // the block begins: the true state, the sensor's memory, and the y of its first step — what the solve started from
  TSAT_DEV void load(const TSAT_GLOBAL real* Pg, real x[7], real y[7]) {
    for (int i = 0; i < 7; ++i) {
      x[i] = xt[(size_t)(MSX_X + i) * st];
      sn.hy[i] = xt[(size_t)(MSX_HY + i) * st];
      y[i] = Pg[P_X0 + i];
    }
  }
  TSAT_DEV void row(int j, const real y[7]) {
    for (int i = 0; i < 7; ++i) hy[(size_t)j * 7 + i] = y[i];
  }
  // the block ends: the next solve starts from the measurement of the step it plans from; when the call ends here, the resident
  // batch gets the TRUE state back
  TSAT_DEV const real* next(long long gid, bool noisy, const real x[7], real y[7]) {
    const int s = h.s.m.step + h.r;
    const bool last = s == h.s.m.n_steps;
    if (!last) sn.state(gid, (int)(h.s.step0 + (long long)s), noisy, x, y);
    for (int i = 0; i < 7; ++i) {
      xt[(size_t)(MSX_X + i) * st] = x[i];
      xt[(size_t)(MSX_HY + i) * st] = sn.hy[i];
    }
    return last ? x : y;
  }
};

// the four kernels' bodies: without and with the gravity rows of tsat_gg.hpp
template <typename real, int ES>
TSAT_DEV void mpc_sensed_traj(const MpcSensedArgs<real>& a, int t) {
  if (t >= a.h.s.m.T) return;
  mpc_held_block<real, ES>(a.h, t, NoEnv(), SensedFeed<real>(a, t));
}

template <typename real, int ES>
TSAT_DEV void mpc_sensed_gg_traj(const MpcSensedArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_held_block<real, ES>(a.h, t, env, SensedFeed<real>(a, t));
}

}  // namespace tsat
