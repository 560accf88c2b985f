// tsat_mpc_filtered.hpp — the held re-planning loop BEHIND THE FILTER (tsat_mpc_run_held_filtered, include/tortoise_hip.h): the loop
// of tsat_mpc_sensed.hpp in which the solver and the gains are handed the estimate of the multiplicative EKF of tsat_filtered.hpp
// instead of the raw measurement. The raw samples m_s, the true state's own record, the plant, the clip, the table clock, the
// shift and the statistic are the parent's; what changes is what goes into P_X0, into dx and into Y_hist.
//
// The filter's arithmetic is Filtered::first / step / estimate as they stand. What is new is where its state lives and which step
// counter it sees. The FLW = 31 values of a lane (FilterState) live in a record of their own, component-major across trajectories
// ([FLW][T], like XT), and are read and written AROUND THE MEASUREMENT only: HeldFiltered::state loads the record, makes the step,
// saves it and hands out the estimate, so the record occupies no registers through the RK4 step, and the same record carries the
// filter from launch to launch and — filt_init / filt_state — from call to call. The inner Sensed's Philox counter has to see the
// generator's knot step0 + s; the filter's "no step at s = 1" of latency 1 needs the step s RELATIVE TO THE CALL: state() is handed
// the knot, as the block hands it to every sensor, and takes step0 off again for the filter.
//
// Sample 0 is the pack's, before the first solve: mpc_sensed_pack as it stands (biases, the true state to XT, m_0 through a copy of
// the arguments with latency 0), then `first` on m_0 — or, with a record given, `step` — and y_0 = (w^_0, q^_0) into P_X0.
//
// The block is mpc_held_block itself (tsat_mpc_held.hpp) with FilteredFeed below as its Feed.
#pragma once
#include "tsat_filtered.hpp"
#include "tsat_mpc_sensed.hpp"

namespace tsat {

// offsets into the flat record (FilterState order)
constexpr int FL_Q = 0, FL_B = 4, FL_W = 7, FL_A = 10, FL_BB = 16, FL_D = 25;
static_assert(FLW == TSAT_FILTER_STATE_W && FL_D + 6 == FLW, "the record of FilterState");

template <typename real>
struct MpcFilteredArgs {
  MpcSensedArgs<real> ms;   // the sensed loop's block, as it is: HY receives the estimates
  FiltArgs<real> f;         // s = ms.s; P, nk, N of the resident batch; M = 1; XH = FF = null (the loop has outputs of its own)
  real* FL;                 // [FLW][T]
};

// What tsat_mpc_run_held_filtered rejects besides what tsat_mpc_run_held_sensed rejects: "" or the reason. f == NULL is the sensed
// call, to which the three arrays mean nothing.
inline std::string check_mpc_filtered(const tsat_filter_options* f, const double* filt_init, const double* filt_state,
                                      const double* filt_final, int64_t T) {
  if (!f) return (filt_init || filt_state || filt_final) ? "filt_init, filt_state and filt_final must be NULL when f is NULL" : "";
  const std::string bad = check_filter(f);
  if (!bad.empty()) return bad;
  if (filt_init)
    for (int64_t t = 0; t < T; ++t) {
      const double* r = filt_init + (size_t)t * FLW;
      for (int i = 0; i < FLW; ++i)
        if (!std::isfinite(r[i])) return "non-finite filt_init entry at t = " + std::to_string(t);
      if (r[FL_Q] * r[FL_Q] + r[FL_Q + 1] * r[FL_Q + 1] + r[FL_Q + 2] * r[FL_Q + 2] + r[FL_Q + 3] * r[FL_Q + 3] == 0.0)
        return "filt_init holds a q^ of zero norm at t = " + std::to_string(t);
    }
  return "";
}

// host side of the record: 31 x T as the caller holds it <-> [FLW][T], and filt_final of a record
inline void filt_records_pack(const double* in, double* out, int64_t T) {
  for (int64_t t = 0; t < T; ++t)
    for (int i = 0; i < FLW; ++i) out[(size_t)i * T + t] = in[(size_t)t * FLW + i];
}
inline void filt_records_unpack(const double* in, int64_t T, double* filt_state, double* filt_final) {
  for (int64_t t = 0; t < T; ++t) {
    double r[FLW];
    for (int i = 0; i < FLW; ++i) r[i] = in[(size_t)i * T + t];
    if (filt_state)
      for (int i = 0; i < FLW; ++i) filt_state[(size_t)t * FLW + i] = r[i];
    if (filt_final) {
      double* ff = filt_final + (size_t)t * FFW;
      for (int i = 0; i < 3; ++i) ff[i] = r[FL_B + i];
      ff[3] = std::sqrt(r[FL_A]); ff[4] = std::sqrt(r[FL_A + 3]); ff[5] = std::sqrt(r[FL_A + 5]);
      ff[6] = std::sqrt(r[FL_D]); ff[7] = std::sqrt(r[FL_D + 3]); ff[8] = std::sqrt(r[FL_D + 5]);
    }
  }
}

// The `Sensor` of mpc_held_block that hands out estimates: the inner Sensed of trajectory t and the filter on its record
template <typename real>
struct HeldFiltered {
  Filtered<real> fl;
  real* rec;                 // the trajectory's column of FL, stride st
  const size_t st;
  const long long step0;
  TSAT_DEV HeldFiltered(const MpcFilteredArgs<real>& a, int t)
      : fl(a.f), rec(a.FL + t), st((size_t)a.ms.h.s.m.T), step0(a.ms.h.s.step0) {
    fl.in.load(0, t);
    const TSAT_GLOBAL real* Pg = (const TSAT_GLOBAL real*)(a.f.P + (size_t)t * PSTRIDE);
    fl.h = Pg[P_DT];
    fl.nt = 0; fl.xh = nullptr; fl.ff = nullptr;               // Filtered::state, which writes them, is not called here
  }
  TSAT_DEV void flown(const real*, const real*, const real*, const real*) {}   // the gyro propagates this filter, not the model
  // sample 0 of the call, which the pack has measured (m): `first`, or a `step` from the record given; y_0 is never predicted
  TSAT_DEV void sample0(const real m[7], bool given, real y[7]) {
    if (given) { fl.st.load(rec, st); fl.step(m); }
    else fl.first(m);
    fl.st.save(rec, st);
    fl.estimate(false, y);
  }
  // y_s at control step s = knot - step0 >= 1 of the call
  TSAT_DEV void state(long long gid, int knot, bool noisy, const real x[7], real y[7]) {
    real m[7];
    fl.in.state(gid, knot, noisy, x, m);                       // m_s, or m_(s-1)
    const int lat = fl.f.s.latency;
    const bool again = lat && (long long)knot - step0 == 1;    // m_0 handed over a second time: no step
    fl.st.load(rec, st);
    if (!again) { fl.step(m); fl.st.save(rec, st); }
    fl.estimate(lat != 0, y);
  }
};

// thread t of the pack grid, before the first solve
template <typename real>
TSAT_DEV void mpc_filtered_pack(const MpcFilteredArgs<real>& a, const real* sensor, int given, int64_t t) {
  const MpcArgs<real>& m = a.ms.h.s.m;
  if (t >= m.T) return;
  mpc_sensed_pack<real>(a.ms, sensor, t);
  HeldFiltered<real> sn(a, (int)t);
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  real m0[7], y[7];
  for (int i = 0; i < 7; ++i) m0[i] = Pg[P_X0 + i];
  sn.sample0(m0, given != 0, y);
  for (int i = 0; i < 7; ++i) Pg[P_X0 + i] = y[i];
}

// The Feed of mpc_held_block that hands the controller estimates: SensedFeed with the filter between the sensor and P_X0 / dx / HY.
// The sensor's latency record is restored and saved as there; the filter's record stays where it is (HeldFiltered).
template <typename real>
struct FilteredFeed {
  const MpcHeldArgs<real>& h;
  HeldFiltered<real> sn;
  TSAT_GLOBAL real* xt;      // the trajectory's column of XT, stride st
  const size_t st;
  real* hy;                  // its row of HY at the block's first step
  TSAT_DEV FilteredFeed(const MpcFilteredArgs<real>& a, int t)
      : h(a.ms.h), sn(a, t), xt((TSAT_GLOBAL real*)(a.ms.XT + t)), st((size_t)a.ms.h.s.m.T),
        hy(a.ms.HY + ((size_t)t * a.ms.h.s.m.n_steps + a.ms.h.s.m.step) * 7) {}
  // the block begins: the true state, the sensor's memory, and the y of its first step — the estimate the solve started from
  TSAT_DEV void load(const TSAT_GLOBAL real* Pg, real x[7], real y[7]) {
    for (int i = 0; i < 7; ++i) {
      x[i] = xt[(size_t)(MSX_X + i) * st];
      sn.fl.in.hy[i] = xt[(size_t)(MSX_HY + i) * st];
      y[i] = Pg[P_X0 + i];
    }
  }
  TSAT_DEV void row(int j, const real y[7]) {
    for (int i = 0; i < 7; ++i) hy[(size_t)j * 7 + i] = y[i];
  }
  // the block ends: the next solve starts from the estimate at the step it plans from; when the call ends here, the resident
  // batch gets the TRUE state back
  TSAT_DEV const real* next(long long gid, bool noisy, const real x[7], real y[7]) {
    const int s = h.s.m.step + h.r;
    const bool last = s == h.s.m.n_steps;
    if (!last) sn.state(gid, (int)(h.s.step0 + (long long)s), noisy, x, y);
    for (int i = 0; i < 7; ++i) {
      xt[(size_t)(MSX_X + i) * st] = x[i];
      xt[(size_t)(MSX_HY + i) * st] = sn.fl.in.hy[i];
    }
    return last ? x : y;
  }
};

// the four kernels' bodies: without and with the gravity rows of tsat_gg.hpp
template <typename real, int ES>
TSAT_DEV void mpc_filtered_traj(const MpcFilteredArgs<real>& a, int t) {
  if (t >= a.ms.h.s.m.T) return;
  mpc_held_block<real, ES>(a.ms.h, t, NoEnv(), FilteredFeed<real>(a, t));
}

template <typename real, int ES>
TSAT_DEV void mpc_filtered_gg_traj(const MpcFilteredArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.ms.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.ms.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_held_block<real, ES>(a.ms.h, t, env, FilteredFeed<real>(a, t));
}

}  // namespace tsat
