// tsat_mpc_model_filtered.hpp — the held re-planning loop BEHIND THE NINE-STATE FILTER (tsat_mpc_run_held_model_filtered,
// include/tortoise_hip.h): the loop of tsat_mpc_sensed.hpp in which the solver and the gains are handed the estimate of the
// model-based multiplicative EKF of tsat_model_filtered.hpp — rate included — instead of the raw measurement. The raw samples m_s, the
// true state's own record, the plant, the clip, the table clock, the shift and the statistic are the parent's; what changes is what
// goes into P_X0, into dx and into Y_hist.
//
// The filter's arithmetic is ModelFiltered::first / predict(b0, b1, b2) / update as they stand. What is new is where its state lives,
// where its model comes from and who tells it what was flown:
//   * the MFLW = 58 values of a lane (ModelFilterState) live in a record of their own, component-major across trajectories
//     ([MFLW][T], like XT), and are read and written AROUND THE MEASUREMENT only: the record occupies no registers through the RK4
//     step, and the same record carries the filter from launch to launch and — filt_init / filt_state — from call to call;
//   * here lane = trajectory, so the model's Traj (h, J, h inv(J), u_scale) is built from the lane's own parameter record by
//     per-lane loads (model_traj below) and not through the wave-uniform constant-address-space pointers of ModelFiltered::load;
//   * mpc_held_block tells the sensor what each step flies — the limited command and the three field rows the plant has just read
//     (`flown`, the hook beside the roll-outs' `commanded`). They are kept in registers until the next state() or the block's next()
//     of the SAME launch: a block's j = 0 makes no filter step, and next() runs in the launch that flew the block's last step, so
//     nothing but the record crosses a launch.
// The inner Sensed's Philox counter has to see the generator's knot step0 + s; the filter's "no update at s = 1" of latency 1 needs
// the step s RELATIVE TO THE CALL: state() is handed the knot and takes step0 off again.
//
// Sample 0 is the pack's, before the first solve: mpc_sensed_pack as it stands, then first(m_0) — or, with a record given,
// update(m_0) on it — and y_0 = (w^_0, q^_0) into P_X0. After the call's last control step next() makes the one closing predict with
// that step's command and rows, so the record left is the prior for x_{n_steps}.
//
// The block is mpc_held_block itself (tsat_mpc_held.hpp) with ModelFilteredFeed below as its Feed.
#pragma once
#include "tsat_model_filtered.hpp"
#include "tsat_mpc_sensed.hpp"

namespace tsat {

// offsets into the flat record (ModelFilterState order)
constexpr int MFL_Q = 0, MFL_W = 4, MFL_B = 7, MFL_U = 10, MFL_A = 13, MFL_WW = 19, MFL_D = 25, MFL_X = 31, MFL_BB = 40, MFL_Y = 49;
static_assert(MFL_Y + 9 == MFLW, "the record of ModelFilterState");

template <typename real>
struct MpcModelFilteredArgs {
  MpcSensedArgs<real> ms;   // the sensed loop's block, as it is: HY receives the estimates
  ModelFiltArgs<real> f;    // s = ms.s; P of the resident batch, us and the seven levels; the rest unused (the rows are handed over)
  real* FL;                 // [MFLW][T]
};

// What tsat_mpc_run_held_model_filtered rejects besides what tsat_mpc_run_held_sensed rejects: "" or the reason. f == NULL is the
// sensed call, to which the three arrays mean nothing.
inline std::string check_mpc_model_filtered(const tsat_model_filter_options* f, const double* filt_init, const double* filt_state,
                                            const double* filt_final, int64_t T) {
  if (!f) return (filt_init || filt_state || filt_final) ? "filt_init, filt_state and filt_final must be NULL when f is NULL" : "";
  const std::string bad = check_model_filter(f);
  if (!bad.empty()) return bad;
  if (filt_init)
    for (int64_t t = 0; t < T; ++t) {
      const double* r = filt_init + (size_t)t * MFLW;
      for (int i = 0; i < MFLW; ++i)
        if (!std::isfinite(r[i])) return "non-finite filt_init entry at t = " + std::to_string(t);
      if (r[MFL_Q] * r[MFL_Q] + r[MFL_Q + 1] * r[MFL_Q + 1] + r[MFL_Q + 2] * r[MFL_Q + 2] + r[MFL_Q + 3] * r[MFL_Q + 3] == 0.0)
        return "filt_init holds a q^ of zero norm at t = " + std::to_string(t);
    }
  return "";
}

// host side of the record: 58 x T as the caller holds it <-> [MFLW][T], and filt_final of a record
inline void model_filt_records_pack(const double* in, double* out, int64_t T) {
  for (int64_t t = 0; t < T; ++t)
    for (int i = 0; i < MFLW; ++i) out[(size_t)i * T + t] = in[(size_t)t * MFLW + i];
}
inline void model_filt_records_unpack(const double* in, int64_t T, double* filt_state, double* filt_final) {
  for (int64_t t = 0; t < T; ++t) {
    double r[MFLW];
    for (int i = 0; i < MFLW; ++i) r[i] = in[(size_t)i * T + t];
    if (filt_state)
      for (int i = 0; i < MFLW; ++i) filt_state[(size_t)t * MFLW + i] = r[i];
    if (filt_final) {
      double* ff = filt_final + (size_t)t * MFFW;
      for (int i = 0; i < 3; ++i) ff[i] = r[MFL_B + i];
      ff[3] = std::sqrt(r[MFL_A]);  ff[4] = std::sqrt(r[MFL_A + 3]);   ff[5] = std::sqrt(r[MFL_A + 5]);
      ff[6] = std::sqrt(r[MFL_WW]); ff[7] = std::sqrt(r[MFL_WW + 3]);  ff[8] = std::sqrt(r[MFL_WW + 5]);
      ff[9] = std::sqrt(r[MFL_D]);  ff[10] = std::sqrt(r[MFL_D + 3]);  ff[11] = std::sqrt(r[MFL_D + 5]);
    }
  }
}

// the model's constants of ONE LANE from its parameter record: what ensemble_traj forms of them (h, h / 2, J, h inv(J), the control
// scales), by per-lane loads; predict reads nothing else of a Traj
template <typename real>
TSAT_DEV Traj<real> model_traj(const TSAT_GLOBAL real* p, real u_scale) {
  Traj<real> tr = {};
  const real h = p[P_DT];
  for (int i = 0; i < 9; ++i) { tr.J[i] = p[P_J + i]; tr.hJi[i] = h * p[P_JI + i]; }
  tr.h = h; tr.hh = (real)0.5 * h; tr.us = u_scale; tr.usj = tr.us * tr.hJi[0];
  return tr;
}

// The `Sensor` of mpc_held_block that hands out the nine-state filter's estimates: the inner Sensed of trajectory t, the filter on
// its record, and what the step just flown was
template <typename real>
struct HeldModelFiltered {
  ModelFiltered<real> fl;
  real* rec;                 // the trajectory's column of FL, stride st
  const size_t st;
  const long long step0;
  real uc[3], r0[3], r1[3], r2[3];   // the limited command and the field rows of the step last flown in this launch
  TSAT_DEV HeldModelFiltered(const MpcModelFilteredArgs<real>& a, int t)
      : fl(a.f), rec(a.FL + t), st((size_t)a.ms.h.s.m.T), step0(a.ms.h.s.step0) {
    fl.in.load(0, t);
    fl.tm = model_traj<real>((const TSAT_GLOBAL real*)(a.f.P + (size_t)t * PSTRIDE), a.f.us);
    fl.bt = nullptr; fl.nt = 0; fl.xh = nullptr; fl.ff = nullptr;   // ModelFiltered::load / state, which use them, are not called here
    for (int c = 0; c < 3; ++c) { uc[c] = 0; r0[c] = 0; r1[c] = 0; r2[c] = 0; }
  }
  // the hook of mpc_held_block: the command as it goes to plant.actuate and the rows the plant's step reads
  TSAT_DEV void flown(const real u[3], const real b0[3], const real b1[3], const real b2[3]) {
    for (int c = 0; c < 3; ++c) { uc[c] = u[c]; r0[c] = b0[c]; r1[c] = b1[c]; r2[c] = b2[c]; }
  }
  // predict across the step last flown, on the record in fl.st
  TSAT_DEV void across() {
    for (int c = 0; c < 3; ++c) fl.st.u[c] = uc[c];
    fl.predict(r0, r1, r2);
  }
  TSAT_DEV void estimate(real y[7]) {
    for (int i = 0; i < 3; ++i) y[i] = fl.st.w[i];
    for (int i = 0; i < 4; ++i) y[3 + i] = fl.st.q[i];
  }
  // sample 0 of the call, which the pack has measured (m): `first`, or an `update` on the record given; y_0 is never predicted
  TSAT_DEV void sample0(const real m[7], bool given, real y[7]) {
    if (given) { fl.st.load(rec, st); fl.update(m); }
    else {
      fl.first(m);
      for (int c = 0; c < 3; ++c) fl.st.u[c] = 0;
    }
    fl.st.save(rec, st);
    estimate(y);
  }
  // y_s at control step s = knot - step0 >= 1 of the call, after step s - 1 was flown in this launch
  TSAT_DEV void state(long long gid, int knot, bool noisy, const real x[7], real y[7]) {
    real m[7];
    fl.in.state(gid, knot, noisy, x, m);                       // m_s, or m_(s-1)
    fl.st.load(rec, st);
    if (fl.f.s.latency) {
      if ((long long)knot - step0 > 1) fl.update(m);           // m_0 handed over a second time makes no update
      across();
    } else {
      across();
      fl.update(m);
    }
    fl.st.save(rec, st);
    estimate(y);
  }
  // the call ends: the one closing predict across its last step, no update — the record left is the prior for x_{n_steps}
  TSAT_DEV void close() {
    fl.st.load(rec, st);
    across();
    fl.st.save(rec, st);
  }
};

// thread t of the pack grid, before the first solve
template <typename real>
TSAT_DEV void mpc_model_filtered_pack(const MpcModelFilteredArgs<real>& a, const real* sensor, int given, int64_t t) {
  const MpcArgs<real>& m = a.ms.h.s.m;
  if (t >= m.T) return;
  mpc_sensed_pack<real>(a.ms, sensor, t);
  HeldModelFiltered<real> sn(a, (int)t);
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  real m0[7], y[7];
  for (int i = 0; i < 7; ++i) m0[i] = Pg[P_X0 + i];
  sn.sample0(m0, given != 0, y);
  for (int i = 0; i < 7; ++i) Pg[P_X0 + i] = y[i];
}

// The Feed of mpc_held_block that hands the controller the nine-state filter's estimates: FilteredFeed of tsat_mpc_filtered.hpp with
// HeldModelFiltered as its sensor, and the closing predict where the call ends.
template <typename real>
struct ModelFilteredFeed {
  const MpcHeldArgs<real>& h;
  HeldModelFiltered<real> sn;
  TSAT_GLOBAL real* xt;      // the trajectory's column of XT, stride st
  const size_t st;
  real* hy;                  // its row of HY at the block's first step
  TSAT_DEV ModelFilteredFeed(const MpcModelFilteredArgs<real>& a, int t)
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
  // the block ends: the next solve starts from the estimate at the step it plans from; when the call ends here, the filter closes
  // its record and the resident batch gets the TRUE state back
  TSAT_DEV const real* next(long long gid, bool noisy, const real x[7], real y[7]) {
    const int s = h.s.m.step + h.r;
    const bool last = s == h.s.m.n_steps;
    if (!last) sn.state(gid, (int)(h.s.step0 + (long long)s), noisy, x, y);
    else sn.close();
    for (int i = 0; i < 7; ++i) {
      xt[(size_t)(MSX_X + i) * st] = x[i];
      xt[(size_t)(MSX_HY + i) * st] = sn.fl.in.hy[i];
    }
    return last ? x : y;
  }
};

// the four kernels' bodies: without and with the gravity rows of tsat_gg.hpp
template <typename real, int ES>
TSAT_DEV void mpc_model_filtered_traj(const MpcModelFilteredArgs<real>& a, int t) {
  if (t >= a.ms.h.s.m.T) return;
  mpc_held_block<real, ES>(a.ms.h, t, NoEnv(), ModelFilteredFeed<real>(a, t));
}

template <typename real, int ES>
TSAT_DEV void mpc_model_filtered_gg_traj(const MpcModelFilteredArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.ms.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.ms.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_held_block<real, ES>(a.ms.h, t, env, ModelFilteredFeed<real>(a, t));
}

}  // namespace tsat
