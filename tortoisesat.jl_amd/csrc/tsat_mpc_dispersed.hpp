// tsat_mpc_dispersed.hpp — the receding-horizon step on a NOISY, DISPERSED plant with limits (tsat_mpc_run_dispersed,
// include/tortoise_hip.h): what mpc_advance_trajectory of tsat_device.hpp does after every solve of the resident batch, with the
// plant of a realisation of the dispersed ensemble (tsat_dispersed.hpp) in place of the model's and the slew-time statistic
// evaluated on the closed-loop history while the loop runs.
//
// One wavefront per trajectory, as the advance kernel: lanes = knots for the plan shift; the clip, the plant step, the noise
// draws and the statistic run on lane 0. The plant is DispersedPlant itself, loaded from a packed record of PLW doubles per
// trajectory ([T][PLW]: the dispersed ensemble's component-major layout with one realisation per slew, Mp = 1) and the slew's
// limits ([T][SATW]); the records are made on the device once per call by dispersed_pack_record (mpc_dispersed_pack), the
// model's plant when the call gives none, +-inf limits when it gives none — so the step has one code path. dyn_sim_h<real, 0>
// on the per-trajectory Traj, plant_noise, brow_index and ensemble_angle are the functions the ensemble roll-out calls; the RK4
// stage sequence is the one of ensemble_rollout (draw the stage's nine values, evaluate, combine). The pieces of a control step
// (the sample test, the RK4 step, the record, the tally) are functions here and serve the held loops of tsat_mpc_held.hpp as well.
//
// Between launches a trajectory keeps two integers in MpcDispRec: the first sample that met the statistic's thresholds and
// the clipped steps so far. Sample j (1-based) of a call is x_{j-1}; step s judges sample s + 1 before it advances, the last
// step also judges sample n_steps + 1 and writes the tsat_tvlqr_stats record.
#pragma once
#include "tsat_dispersed.hpp"

namespace tsat {

struct MpcDispRec {
  int first;      // 1-based index of the first sample inside both thresholds, 0 = none yet
  int clipped;    // control steps at which the limits changed the command
};

template <typename real>
struct MpcDispArgs {
  MpcArgs<real> m;       // the advance step's own arguments (plant_integ unused: the noise layout is per RK4 stage)
  // the plant and the statistic. Of d.e only these are read: min_steps, w_tol, ang_tol, k0, k1, sg, sa, fa, nid0 ([T] generator id
  // of each trajectory or null = t) and stats ([T], written by the last step). d.PL [T][PLW], d.Mp = 1, d.SAT [T][SATW],
  // d.nclip [T] (written by the last step) or null.
  DispArgs<real> d;
  int noisy;             // 1: inject the nine draws of (id, knot step0 + step, stage) into every stage
  long long step0;
  MpcDispRec* rec;       // [T]
};

// thread t of the pack grid: the packed plant record of trajectory t (plant == null: the model's) and its running record
template <typename real>
TSAT_DEV void mpc_dispersed_pack(const real* plant, const real* P, real us, real* PL, MpcDispRec* rec, int64_t T, int64_t t) {
  if (t >= T) return;
  const TSAT_GLOBAL real* pl = plant ? (const TSAT_GLOBAL real*)(plant + (size_t)t * TSAT_PLANT_W) : nullptr;
  dispersed_pack_record<real>(pl, (const TSAT_GLOBAL real*)(P + (size_t)t * PSTRIDE), us, (TSAT_GLOBAL real*)(PL + (size_t)t * PLW),
                              (size_t)1);
  rec[t].first = 0;
  rec[t].clipped = 0;
}

// The pieces of a control step, shared by every plant loop: mpc_held_block (tsat_mpc_held.hpp) runs them on every lane,
// mpc_dispersed_trajectory below on lane 0 — all but mpc_rk4, whose stages it keeps inline for the reason given there.

// sample j (1-based) of the call is judged: the first one inside both thresholds is kept
template <typename real>
TSAT_DEV void mpc_sample(const EnsArgs<real>& e, const Traj<real>& tr, const real x[7], int j, int& first) {
  const real wj = sqrt_(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (first == 0 && j > e.min_steps && wj < e.w_tol) {
    if (ensemble_angle<real>(tr, x) < e.ang_tol) first = j;
  }
}

// what acts on the body in an RK4 stage besides m x B: nothing here (GgEnv of tsat_gg.hpp adds the gravity-gradient term).
// `row`: the table row of the stage, x: the stage state as integrated, k: the stage's increment
struct NoEnv {
  template <typename real>
  TSAT_DEV void stage(const Traj<real>&, int, const real*, real*) const {}
};

// one RK4 step of the plant tp under the applied dipole us, field rows b0, b1, b2 (table rows i0, i1, i2): the stage sequence of
// ensemble_rollout (draw the stage's nine values of (gid, knot, stage), evaluate, combine)
template <typename real, typename Env>
TSAT_DEV void mpc_rk4(const Traj<real>& tp, const EnsArgs<real>& e, bool noisy, long long gid, int knot, const real x[7],
                      const real us[3], const real b0[3], const real b1[3], const real b2[3], const Env& env, int i0, int i1, int i2,
                      real xn[7]) {
  real k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
  for (int i = 0; i < 9; ++i) nz[i] = 0;
  if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 0, e.sg, e.sa, e.fa, nz);
  dyn_sim_h<real, 0>(tp, x, us, b0, noisy, nz, k1);
  env.stage(tp, i0, x, k1);
  for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
  if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 1, e.sg, e.sa, e.fa, nz);
  dyn_sim_h<real, 0>(tp, t, us, b1, noisy, nz, k2);
  env.stage(tp, i1, t, k2);
  for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
  if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 2, e.sg, e.sa, e.fa, nz);
  dyn_sim_h<real, 0>(tp, t, us, b1, noisy, nz, k3);
  env.stage(tp, i1, t, k3);
  for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
  if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 3, e.sg, e.sa, e.fa, nz);
  dyn_sim_h<real, 0>(tp, t, us, b2, noisy, nz, k4);
  env.stage(tp, i2, t, k4);
  for (int i = 0; i < 7; ++i) xn[i] = x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (real)(1.0 / 6.0);
}

// the last sample j = n of the call is judged, then the record of the call's history
template <typename real>
TSAT_DEV tsat_tvlqr_stats mpc_record(const EnsArgs<real>& e, const Traj<real>& tr, const real xn[7], int n, int& first) {
  const real wN = sqrt_(xn[0] * xn[0] + xn[1] * xn[1] + xn[2] * xn[2]);
  const real angN = ensemble_angle<real>(tr, xn);
  if (first == 0 && n > e.min_steps && wN < e.w_tol && angN < e.ang_tol) first = n;
  tsat_tvlqr_stats st;
  st.slew_index = first;
  st.failed = first ? 0 : 1;
  st.slew_time = (double)tr.h * (first ? (double)first : (double)n);
  st.final_w_norm = (double)wN;
  st.final_angle = (double)angN;
  return st;
}

// executed counts of the solve that has just finished, added to the loop's running sums
template <typename real>
TSAT_DEV void mpc_tally(const MpcArgs<real>& m, int traj) {
  if (!m.tally) return;
  const tsat_stats& st = m.stats[traj];
  long long* tl = m.tally + (size_t)traj * 4;
  tl[0] += st.n_backward; tl[1] += st.n_forward; tl[2] += (st.outer_iters > 1 ? st.outer_iters - 1 : 0); tl[3] += st.inner_iters;
}

template <typename real>
TSAT_DEV void mpc_dispersed_trajectory(const MpcDispArgs<real>& a, int traj) {
  const MpcArgs<real>& m = a.m;
  const EnsArgs<real>& e = a.d.e;
  real* lds = lds_base<real>();
  const int lane = TSAT_LANE();
  const int NS = m.N;
  const int N = m.nk ? m.nk[traj] : m.N;
  TSAT_GLOBAL real* Pg = (TSAT_GLOBAL real*)(m.P + (size_t)traj * PSTRIDE);
  stage_traj<real>(Pg, m.us);
  TSAT_SYNC();
  const Traj<real> tr = load_traj<real>(N, m.n_tab, (const TSAT_GLOBAL real*)(m.BT + (size_t)m.bidx[traj] * m.n_tab * 4));
  const TSAT_GLOBAL real* XUg = (const TSAT_GLOBAL real*)(m.XU + (size_t)traj * NS * XUW);
  TSAT_GLOBAL real* U0g = (TSAT_GLOBAL real*)(m.U0 + (size_t)traj * (NS - 1) * 3);
  // the next warm start: the plan shifted by one knot, last control repeated (as mpc_advance_trajectory)
  for (int k = lane; k < N - 1; k += WAVE) {
    const int src = (k + 1 < N - 1) ? k + 1 : N - 2;
    for (int c = 0; c < 3; ++c) U0g[(size_t)k * 3 + c] = XUg[(size_t)src * XUW + 7 + c];
  }
  if (lane == 0) {
    DispersedPlant<real> plant(a.d);
    plant.load(tr, traj, 0);
    const Traj<real>& tp = plant.traj(tr);                     // the model's constants with Jp and h inv(Jp)
    const real cs = control_scale<real, 0>(tr);
    MpcDispRec rec = a.rec[traj];
    real x[7], uc[3], us[3];
    for (int i = 0; i < 7; ++i) x[i] = lds[L_TR + P_X0 + i];
    mpc_sample<real>(e, tr, x, m.step + 1, rec.first);
    for (int c = 0; c < 3; ++c) uc[c] = plant.command(c, XUg[7 + c], cs);
    plant.actuate(uc, cs, us);
    rec.clipped += plant.clipped;
    // rows at tau, tau + dtau / 2, tau + dtau of the current table clock
    const TSAT_GLOBAL real* p0 = tr.bt + (size_t)brow_index(tr, 0, 0.0) * 4;
    const TSAT_GLOBAL real* p1 = tr.bt + (size_t)brow_index(tr, 0, 0.5) * 4;
    const TSAT_GLOBAL real* p2 = tr.bt + (size_t)brow_index(tr, 0, 1.0) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    const bool noisy = a.noisy != 0;
    const long long gid = e.nid0 ? e.nid0[traj] : (long long)traj;
    const int knot = (int)(a.step0 + (long long)m.step);
    // the stages of mpc_rk4 without an Env, kept inline: called as a function they cost this kernel eight registers and 90
    // instructions (tools/isa_compare.py, tools/resource_usage.py)
    real k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
    for (int i = 0; i < 9; ++i) nz[i] = 0;
    if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 0, e.sg, e.sa, e.fa, nz);
    dyn_sim_h<real, 0>(tp, x, us, b0, noisy, nz, k1);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
    if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 1, e.sg, e.sa, e.fa, nz);
    dyn_sim_h<real, 0>(tp, t, us, b1, noisy, nz, k2);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
    if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 2, e.sg, e.sa, e.fa, nz);
    dyn_sim_h<real, 0>(tp, t, us, b1, noisy, nz, k3);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
    if (noisy) plant_noise<real>(e.k0, e.k1, gid, knot, 3, e.sg, e.sa, e.fa, nz);
    dyn_sim_h<real, 0>(tp, t, us, b2, noisy, nz, k4);
    real xn[7];
    for (int i = 0; i < 7; ++i) xn[i] = x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (real)(1.0 / 6.0);
    real* hx = m.HX + ((size_t)traj * (m.n_steps + 1) + m.step) * 7;
    real* hu = m.HU + ((size_t)traj * m.n_steps + m.step) * 3;
    for (int i = 0; i < 7; ++i) { hx[i] = x[i]; Pg[P_X0 + i] = xn[i]; }
    for (int c = 0; c < 3; ++c) hu[c] = uc[c];                 // the limited command, units of u_scale
    Pg[P_TAU0] = (real)(tr.tau0 + tr.dtau);
    mpc_tally<real>(m, traj);
    if (m.step == m.n_steps - 1) {  // last sample j = n_steps + 1, then the record
      for (int i = 0; i < 7; ++i) hx[7 + i] = xn[i];
      e.stats[traj] = mpc_record<real>(e, tr, xn, m.n_steps + 1, rec.first);
      if (a.d.nclip) a.d.nclip[traj] = rec.clipped;
    }
    a.rec[traj] = rec;
  }
}

}  // namespace tsat
