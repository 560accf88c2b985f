// tsat_mpc_model_mag_filtered.hpp — the held re-planning loop BEHIND THE MAGNETOMETER-UPDATED NINE-STATE FILTER
// (tsat_mpc_run_held_model_mag_filtered, include/tortoise_hip.h): the loop of tsat_mpc_model_filtered.hpp with the filter's
// update(m) replaced by ModelMagFiltered::update(wm, bs, rj) of tsat_model_mag_filtered.hpp, called as it stands — a. the
// magnetometer block against the slew's field row, then b. the gyro block. The attitude sensor is read ONCE, at sample 0 of a call
// without a record (`first`); q_m of every later sample is ignored. Blocks, the clip, the plant, the table clock, the shift, the
// statistic, the model (model_traj), first, predict, the closing predict, the 58-value record and the 12-value filt_final are the
// parent's.
//
// What is new is the magnetometer sample and the row it is formed and paired with. Per control step s, counted from the call:
//   b_m,s = Sensed::field(gid, step0 + s, noisy, x_s, r_s) on the TRUE state x_s, r_s the stage-0 row of the table clock at step s
//   (brow_index(tr, 0, 0.0) on the clock the plant's step s reads): the Philox block the ensembles draw for that id and knot.
// NO NEW TABLE READ IN THE HOLD: mpc_held_block hands the sensor the three rows of each step through flown(uc, b0, b1, b2), and
//   * b2 of step s - 1 is bit for bit b0 of step s: the clock advances by tau <- tau + dtau, and brow_index's fma(1, dtau, tau0)
//     is that same rounded addition, so floor and clamp see the same number and the same row is loaded;
//   * b0 of step s - 1 is r_{s-1}.
// state() and next() run after step s - 1 was flown in the same launch, so r_s = r2 and r_{s-1} = r0 as they stand in registers.
//   latency 0:  s >= 1: predict(u_{s-1}, rows_{s-1}), update(w_m,s, b_m,s, r_s = r2)
//   latency 1:  s = 1: m_0 arrives a second time and makes no update — the field is still sampled, so the one-knot memory holds
//               b_m,1 —, predict(u_0);  s >= 2: update(w_m,s-1, b_m,s-1, r_{s-1} = r0), predict(u_{s-1}): the delayed sample is
//               paired with the row it was formed with
// The inner Sensed keeps the last field sample in hb as it keeps the last (w_m, q_m) in hy; hb crosses launches in a record of its
// own, HB [3][T], component-major like XT, restored and saved next to hy. The filter's record and HB are read and written around
// the measurement only and occupy nothing through the RK4 step. No LDS.
//
// Sample 0 is the pack's, before the first solve: mpc_sensed_pack as it stands, then b_m,0 through a latency-0 copy of the sensor
// with the row of the clock's knot 0 as the call finds it, stored to HB, then first(m_0) — or, with a record given,
// update(w_m,0, b_m,0, r_0) on it — and y_0 into P_X0.
//
// The block is mpc_held_block itself (tsat_mpc_held.hpp) with ModelMagFilteredFeed below as its Feed.
#pragma once
#include "tsat_model_mag_filtered.hpp"
#include "tsat_mpc_model_filtered.hpp"

namespace tsat {

// MpcModelFilteredArgs with the filter's block in the form ModelMagFiltered takes it (the parent's ModelFiltArgs and sigma_m side by
// side), so that the filter refers to the launch's arguments as the parent's does and its record stays in registers, and the
// field's memory
template <typename real>
struct MpcModelMagFilteredArgs {
  MpcSensedArgs<real> ms;          // the sensed loop's block, as it is: HY receives the estimates
  ModelMagFiltArgs<real> f;        // f.m as MpcModelFilteredArgs::f (sa unused), f.sm = sigma_m
  real* FL;                        // [MFLW][T]
  real* HB;                        // [3][T] the last field sample b_m of a trajectory (Sensed::hb between launches)
};

// What tsat_mpc_run_held_model_mag_filtered rejects besides what tsat_mpc_run_held_sensed rejects: "" or the reason. The levels are
// check_model_mag_filter's; the rules of the three arrays are the parent's, asked with levels that pass its own check.
inline std::string check_mpc_model_mag_filtered(const tsat_model_mag_filter_options* f, const double* filt_init, const double* filt_state,
                                                const double* filt_final, int64_t T) {
  if (!f) return check_mpc_model_filtered(nullptr, filt_init, filt_state, filt_final, T);
  const std::string bad = check_model_mag_filter(f);
  if (!bad.empty()) return bad;
  tsat_model_filter_options g;
  g.sigma_v = f->sigma_v; g.sigma_w = f->sigma_w; g.sigma_u = f->sigma_u; g.sigma_a = 1.0; g.sigma_g = f->sigma_g;
  g.p0_att = f->p0_att; g.p0_bias = f->p0_bias; g.reserved = 0;
  return check_mpc_model_filtered(&g, filt_init, filt_state, filt_final, T);
}

// The `Sensor` of mpc_held_block that hands out the magnetometer-updated filter's estimates: HeldModelFiltered with a
// ModelMagFiltered (and through it the ModelFiltered, the inner Sensed and the record) in the place of its ModelFiltered
template <typename real>
struct HeldModelMagFiltered {
  ModelMagFiltered<real> fl;
  real* rec;                 // the trajectory's column of FL, stride st
  const size_t st;
  const long long step0;
  real uc[3], r0[3], r1[3], r2[3];   // the limited command and the field rows of the step last flown in this launch
  TSAT_DEV HeldModelMagFiltered(const MpcModelMagFilteredArgs<real>& a, int t)
      : fl(a.f), rec(a.FL + t), st((size_t)a.ms.h.s.m.T), step0(a.ms.h.s.step0) {
    ModelFiltered<real>& mf = fl.mf;
    mf.in.load(0, t);
    mf.tm = model_traj<real>((const TSAT_GLOBAL real*)(a.f.m.P + (size_t)t * PSTRIDE), a.f.m.us);
    mf.bt = nullptr; mf.nt = 0; mf.xh = nullptr; mf.ff = nullptr;   // the loads and state() that use them are not called here
    for (int c = 0; c < 3; ++c) { uc[c] = 0; r0[c] = 0; r1[c] = 0; r2[c] = 0; fl.bmag[c] = 0; }
  }
  // the hook of mpc_held_block: the command as it goes to plant.actuate and the rows the plant's step reads
  TSAT_DEV void flown(const real u[3], const real b0[3], const real b1[3], const real b2[3]) {
    for (int c = 0; c < 3; ++c) { uc[c] = u[c]; r0[c] = b0[c]; r1[c] = b1[c]; r2[c] = b2[c]; }
  }
  // predict across the step last flown, on the record in fl.mf.st
  TSAT_DEV void across() {
    for (int c = 0; c < 3; ++c) fl.mf.st.u[c] = uc[c];
    fl.mf.predict(r0, r1, r2);
  }
  TSAT_DEV void estimate(real y[7]) {
    for (int i = 0; i < 3; ++i) y[i] = fl.mf.st.w[i];
    for (int i = 0; i < 4; ++i) y[3 + i] = fl.mf.st.q[i];
  }
  // sample 0 of the call, which the pack has measured (m, and bs against the row rj of the clock's knot 0): `first` — the one
  // attitude fix, no magnetometer update —, or an `update` on the record given; y_0 is never predicted
  TSAT_DEV void sample0(const real m[7], const real bs[3], const real rj[3], bool given, real y[7]) {
    if (given) { fl.mf.st.load(rec, st); fl.update(m, bs, rj); }
    else {
      fl.mf.first(m);
      for (int c = 0; c < 3; ++c) fl.mf.st.u[c] = 0;
    }
    fl.mf.st.save(rec, st);
    estimate(y);
  }
  // y_s at control step s = knot - step0 >= 1 of the call, after step s - 1 was flown in this launch: r2 is r_s, r0 is r_{s-1}
  TSAT_DEV void state(long long gid, int knot, bool noisy, const real x[7], real y[7]) {
    real m[7], bs[3];
    fl.mf.in.state(gid, knot, noisy, x, m);                    // m_s, or m_(s-1)
    fl.mf.in.field(gid, knot, noisy, x, r2, bs);               // b_m,s is formed with r_s; handed over: b_m,s, or b_m,(s-1)
    fl.mf.st.load(rec, st);
    if (fl.fm.m.s.latency) {
      if ((long long)knot - step0 > 1) fl.update(m, bs, r0);   // m_0 handed over a second time makes no update
      across();
    } else {
      across();
      fl.update(m, bs, r2);
    }
    fl.mf.st.save(rec, st);
    estimate(y);
  }
  // the call ends: the one closing predict across its last step, no update — the record left is the prior for x_{n_steps}
  TSAT_DEV void close() {
    fl.mf.st.load(rec, st);
    across();
    fl.mf.st.save(rec, st);
  }
};

// thread t of the pack grid, before the first solve and after mpc_held_pack (the clock's step is read from its record)
template <typename real>
TSAT_DEV void mpc_model_mag_filtered_pack(const MpcModelMagFilteredArgs<real>& a, const real* sensor, int given, int64_t t) {
  const MpcSensedArgs<real>& ms = a.ms;
  const MpcArgs<real>& m = ms.h.s.m;
  if (t >= m.T) return;
  mpc_sensed_pack<real>(ms, sensor, t);
  const size_t st = (size_t)m.T;
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)t * PSTRIDE);
  const TSAT_GLOBAL real* xt = (const TSAT_GLOBAL real*)(ms.XT + t);
  const TSAT_GLOBAL real* hr = (const TSAT_GLOBAL real*)(ms.h.s.d.PL + t);
  // r_0: the stage-0 row of the clock as the call finds it — what mpc_held_block reads as b0 of step 0
  Traj<real> tr = {};
  tr.tau0 = (double)Pg[P_TAU0] + (double)Pg[P_TAU0L]; tr.dtau = (double)hr[(size_t)HELD_DTAU * st]; tr.n_tab = m.n_tab;
  const TSAT_GLOBAL real* p0 = (const TSAT_GLOBAL real*)(m.BT + (size_t)m.bidx[t] * m.n_tab * 4) + (size_t)brow_index(tr, 0, 0.0) * 4;
  const real rj[3] = {p0[0], p0[1], p0[2]};
  real x[7], m0[7], bs[3], y[7];
  for (int i = 0; i < 7; ++i) { x[i] = xt[(size_t)(MSX_X + i) * st]; m0[i] = Pg[P_X0 + i]; }
  {  // b_m,0: the sample of step 0 has no older one, whatever the latency
    SensArgs<real> s0 = ms.s;
    s0.latency = 0;
    Sensed<real> sn0(s0);
    sn0.load(0, (int)t);
    const EnsArgs<real>& e = ms.h.s.d.e;
    sn0.field(e.nid0 ? e.nid0[t] : (long long)t, (int)ms.h.s.step0, ms.h.s.noisy != 0, x, rj, bs);
  }
  for (int i = 0; i < 3; ++i) a.HB[(size_t)i * st + t] = bs[i];
  HeldModelMagFiltered<real> sn(a, (int)t);
  sn.sample0(m0, bs, rj, given != 0, y);
  for (int i = 0; i < 7; ++i) Pg[P_X0 + i] = y[i];
}

// The Feed of mpc_held_block that hands the controller this filter's estimates: ModelFilteredFeed with HeldModelMagFiltered as its
// sensor, carrying the field's memory hb as it carries hy.
template <typename real>
struct ModelMagFilteredFeed {
  const MpcHeldArgs<real>& h;
  HeldModelMagFiltered<real> sn;
  TSAT_GLOBAL real* xt;      // the trajectory's column of XT, stride st
  TSAT_GLOBAL real* hb;      // its column of HB, stride st
  const size_t st;
  real* hy;                  // its row of HY at the block's first step
  TSAT_DEV ModelMagFilteredFeed(const MpcModelMagFilteredArgs<real>& a, int t)
      : h(a.ms.h), sn(a, t), xt((TSAT_GLOBAL real*)(a.ms.XT + t)), hb((TSAT_GLOBAL real*)(a.HB + t)),
        st((size_t)a.ms.h.s.m.T), hy(a.ms.HY + ((size_t)t * a.ms.h.s.m.n_steps + a.ms.h.s.m.step) * 7) {}
  // the block begins: the true state, the sensor's memory, and the y of its first step — the estimate the solve started from
  TSAT_DEV void load(const TSAT_GLOBAL real* Pg, real x[7], real y[7]) {
    for (int i = 0; i < 7; ++i) {
      x[i] = xt[(size_t)(MSX_X + i) * st];
      sn.fl.mf.in.hy[i] = xt[(size_t)(MSX_HY + i) * st];
      y[i] = Pg[P_X0 + i];
    }
    for (int i = 0; i < 3; ++i) sn.fl.mf.in.hb[i] = hb[(size_t)i * st];
  }
  TSAT_DEV void row(int j, const real y[7]) {
    for (int i = 0; i < 7; ++i) hy[(size_t)j * 7 + i] = y[i];
  }
  // the block ends: the next solve starts from the estimate at the step it plans from — measured against b2 of the block's last
  // step, the row of that step's clock; when the call ends here, the filter closes its record and the resident batch gets the
  // TRUE state back
  TSAT_DEV const real* next(long long gid, bool noisy, const real x[7], real y[7]) {
    const int s = h.s.m.step + h.r;
    const bool last = s == h.s.m.n_steps;
    if (!last) sn.state(gid, (int)(h.s.step0 + (long long)s), noisy, x, y);
    else sn.close();
    for (int i = 0; i < 7; ++i) {
      xt[(size_t)(MSX_X + i) * st] = x[i];
      xt[(size_t)(MSX_HY + i) * st] = sn.fl.mf.in.hy[i];
    }
    for (int i = 0; i < 3; ++i) hb[(size_t)i * st] = sn.fl.mf.in.hb[i];
    return last ? x : y;
  }
};

// the four kernels' bodies: without and with the gravity rows of tsat_gg.hpp
template <typename real, int ES>
TSAT_DEV void mpc_model_mag_filtered_traj(const MpcModelMagFilteredArgs<real>& a, int t) {
  if (t >= a.ms.h.s.m.T) return;
  mpc_held_block<real, ES>(a.ms.h, t, NoEnv(), ModelMagFilteredFeed<real>(a, t));
}

template <typename real, int ES>
TSAT_DEV void mpc_model_mag_filtered_gg_traj(const MpcModelMagFilteredArgs<real>& a, int t) {
  const MpcArgs<real>& m = a.ms.h.s.m;
  if (t >= m.T) return;
  const GgEnv<real> env{(const TSAT_GLOBAL real*)(a.ms.GT + (size_t)m.bidx[t] * m.n_tab * 4)};
  mpc_held_block<real, ES>(a.ms.h, t, env, ModelMagFilteredFeed<real>(a, t));
}

}  // namespace tsat
