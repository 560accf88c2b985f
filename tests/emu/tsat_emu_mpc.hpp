// tsat_emu_mpc.hpp — the receding-horizon plant loops under the CPU lane emulator (TEST INFRASTRUCTURE): what the drivers of
// tsat_mpc_run_dispersed (tsat_emu_mpc_dispersed.cpp) and of the three held loops (tsat_emu_mpc_held.cpp, tsat_emu_gg.cpp,
// tsat_emu_mpc_sensed.cpp) share. Takes run_wave / for_each_wave, the emulated solve (solve_block) and the packing code from
// tsat_emu.cpp as they are. MpcBatch is the emulated resident batch with the arguments every plant loop has; emu_mpc_held is the
// loop of tsat_mpc_run_held, _held_gg and _held_sensed: the product's own packs, one call per thread of their grids, then per
// block the emulated solve of every trajectory, mpc_held_block per trajectory with the call's Env and Feed, and mpc_held_shift per
// wavefront. The arguments are validated by the library's own host functions (tsat_host_pack.hpp, tsat_mpc_sensed.hpp).
#pragma once
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_mpc_sensed.hpp"

// the arguments of emu_mpc_held_batch, in its order: the batch as emu_mpc_batch, then those of tsat_mpc_run_held
// (include/tortoise_hip.h), the last plan, n_knots. emu_mpc_dispersed_batch has them all but replan_every and feedback.
struct MpcIn {
  const tsat_options* o;
  const tsat_tvlqr_options* po;
  int64_t T, n_btab;
  const double *x0, *xf, *Btab;
  const int32_t* btab_idx;
  const double *tau0, *dtau, *dt, *Jmat, *Qd, *Qfd, *Rd, *ulo, *uhi, *U0;
  int32_t n_steps;
  int64_t step0;
  int32_t replan_every, feedback;
  const double *plant, *sat_lo, *sat_hi;
  const int64_t* noise_id;
  double *X_hist, *U_hist;
  tsat_stats* stats_last;
  tsat_tvlqr_stats* stats;
  int32_t* n_clipped;
  double *X_last, *U_last;
  const int32_t* n_knots;
};

// what tsat_mpc_run_dispersed rejects
static bool mpc_in_valid(const MpcIn& in) {
  const tsat_options& o = *in.o;
  return check_options(o, o.n_knots, o.n_tab, o.max_linesearch).empty() && o.precision == 64 &&
         check_mpc_dispersed(*in.po, in.n_steps, in.step0, in.plant, in.sat_lo, in.sat_hi, in.T).empty();
}

// the emulated device buffers of a valid call, the solve's arguments and the plant loop's (md: all but PL, step and the caller's own)
struct MpcBatch {
  const MpcIn& in;
  const int N, max_ls;
  std::vector<double> P, BT, U0w, SAT, XU, KD, LAM, CAND;
  std::vector<int> bidx;
  std::vector<MpcDispRec> rec;
  KArgs<double> a;
  blk_t blk;
  MpcBatch(const MpcIn& in_, MpcDispArgs<double>& md)
      : in(in_), N(in.o->n_knots), max_ls(in.o->max_linesearch < NSTORE ? in.o->max_linesearch : NSTORE), P((size_t)in.T * PSTRIDE),
        BT((size_t)in.n_btab * in.o->n_tab * 4), U0w(in.U0, in.U0 + (size_t)in.T * (N - 1) * 3), SAT(pack_limits(in.sat_lo, in.sat_hi, in.T)),
        XU((size_t)in.T * N * XUW, 0.0), KD((size_t)in.T * (N - 1) * KDW, 0.0), LAM((size_t)in.T * (N - 1) * LMW, 0.0),
        CAND((size_t)in.T * max_ls * N * XUW, 0.0), bidx(in.T), rec((size_t)in.T) {
    const int64_t T = in.T;
    const int n_tab = in.o->n_tab;
    pack_params<double>(T, in.x0, in.xf, in.tau0, in.dtau, in.dt, in.Jmat, in.Qd, in.Qfd, in.Rd, in.ulo, in.uhi, P.data());
    pack_btab<double>(in.n_btab, n_tab, in.Btab, BT.data());
    for (int64_t t = 0; t < T; ++t) bidx[t] = in.btab_idx ? in.btab_idx[t] : (int)t;
    a.T = (int)T; a.N = N; a.n_tab = n_tab; a.max_ls = max_ls; a.opt = *in.o;
    a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = in.n_knots; a.U0 = U0w.data();
    a.XU = XU.data(); a.KD = KD.data(); a.LAM = LAM.data(); a.CAND = CAND.data();
    a.stats = in.stats_last; a.trace = nullptr; a.trace_rows = 0;
    blk = solve_block(*in.o, inertia_class(T, in.Jmat));
    MpcArgs<double>& m = md.m;
    m.T = (int)T; m.N = N; m.n_tab = n_tab; m.plant_integ = 4; m.n_steps = in.n_steps; m.us = in.o->u_scale;
    m.P = P.data(); m.BT = BT.data(); m.bidx = bidx.data(); m.nk = in.n_knots; m.XU = XU.data(); m.U0 = U0w.data();
    m.HX = in.X_hist; m.HU = in.U_hist; m.stats = nullptr; m.tally = nullptr;
    md.d.Mp = 1; md.d.SAT = SAT.data(); md.d.nclip = in.n_clipped;
    fill_ens_options(*in.po, md.d.e);
    md.d.e.nid0 = (const long long*)in.noise_id; md.d.e.stats = in.stats;
    md.noisy = in.po->noise_mode; md.step0 = (long long)in.step0; md.rec = rec.data();
  }
  void solve() {
    tsat_emu::for_each_wave((int)in.T, [&](int t) { blk(a, t); });
  }
  void export_last() {
    for (int64_t e = 0; e < in.T * (int64_t)N; ++e) export_record<double>(e, N, in.n_knots, XU.data(), KD.data(), in.X_last, in.U_last, nullptr);
  }
};

// The loop of tsat_mpc_run_held. Rtab: that of tsat_mpc_run_held_gg (the hold through the gravity rows), or null. s: the sensor of
// tsat_mpc_run_held_sensed with its `sensor` and Y_hist (either may be null), or null: the true state. x0_after (sensed call, or
// null): x0 of the parameter records as the call leaves them — what a following solve of the resident batch would start from.
static int emu_mpc_held(const MpcIn& in, const double* Rtab, double gm, const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                        double* x0_after) {
  const int64_t T = in.T, rows = in.n_btab * (int64_t)in.o->n_tab;
  if (!mpc_in_valid(in)) return -1;
  if (Rtab && !check_gravity(Rtab, gm, rows).empty()) return -1;
  if (s && !check_mpc_sensed(s, sensor, T, Rtab, gm).empty()) return -1;
  int min_nk = in.o->n_knots;
  for (int64_t t = 0; in.n_knots && t < T; ++t) min_nk = in.n_knots[t] < min_nk ? in.n_knots[t] : min_nk;
  if (!check_mpc_held(in.replan_every, in.feedback, min_nk).empty()) return -1;
  MpcSensedArgs<double> ms = {};
  MpcHeldArgs<double>& mh = ms.h;
  MpcArgs<double>& m = mh.s.m;
  MpcBatch b(in, mh.s);
  std::vector<double> PL((size_t)T * HELD_W), GT, SN, XT, Yw;
  mh.s.d.PL = PL.data(); mh.KD = b.KD.data(); mh.feedback = in.feedback;
  for (int64_t t = 0; t < T; ++t) mpc_held_pack<double>(in.plant, b.P.data(), b.SAT.data(), in.o->u_scale, PL.data(), b.rec.data(), T, t);
  if (Rtab) {
    GT.resize((size_t)rows * 4);
    for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  }
  const double* gt = Rtab ? GT.data() : nullptr;
  if (s) {
    SN.assign((size_t)T * SNW, -1.0); XT.assign((size_t)T * MSX_W, -1.0);   // the pack writes every slot
    if (!Y_hist) { Yw.resize((size_t)T * in.n_steps * 7); Y_hist = Yw.data(); }
    ms.GT = gt; ms.XT = XT.data(); ms.HY = Y_hist;
    ms.s.SN = SN.data(); ms.s.Mp = (int)T; ms.s.sgy = s->sigma_gyro; ms.s.sat = s->sigma_att; ms.s.smg = s->sigma_mag;
    ms.s.latency = s->latency; ms.s.k0 = mh.s.d.e.k0; ms.s.k1 = mh.s.d.e.k1;
    for (int64_t t = 0; t < T; ++t) mpc_sensed_pack<double>(ms, sensor, t);
  }
  const int es = in.o->error_state ? 1 : 0;
  for (int sb = 0; sb < in.n_steps; sb += in.replan_every) {
    b.solve();
    m.step = sb;
    mh.r = in.replan_every < in.n_steps - sb ? in.replan_every : in.n_steps - sb;
    const MpcHeldGgArgs<double> mg = {mh, gt};
    for (int t = 0; t < (int)T; ++t) {    // lane = trajectory: no lane of the hold talks to another
      if (s && gt) es ? mpc_sensed_gg_traj<double, 1>(ms, t) : mpc_sensed_gg_traj<double, 0>(ms, t);
      else if (s) es ? mpc_sensed_traj<double, 1>(ms, t) : mpc_sensed_traj<double, 0>(ms, t);
      else if (gt) es ? mpc_held_gg_block<double, 1>(mg, t) : mpc_held_gg_block<double, 0>(mg, t);
      else es ? mpc_held_block<double, 1>(mh, t) : mpc_held_block<double, 0>(mh, t);
    }
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_held_shift<double>(m, mh.r, t); });
  }
  b.export_last();
  if (x0_after)
    for (int64_t t = 0; t < T; ++t)
      for (int i = 0; i < 7; ++i) x0_after[7 * t + i] = b.P[(size_t)t * PSTRIDE + P_X0 + i];
  return 0;
}
