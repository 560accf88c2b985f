// tsat_emu_mpc_sensed.cpp — the held re-planning loop fed measurements (tortoisesat.jl_amd/csrc/tsat_mpc_sensed.hpp) under the CPU
// lane emulator (TEST INFRASTRUCTURE). Takes run_wave / for_each_wave, the emulated solve (run_block) and the packing code from
// tsat_emu.cpp as they are. The driver is that of tsat_emu_mpc_held.cpp / tsat_emu_gg.cpp with the loop of
// tsat_mpc_run_held_sensed: the product's own packs, one call per thread of their grids (mpc_held_pack, gg_pack_row when there is
// an orbit table, mpc_sensed_pack), then per block the emulated solve, mpc_sensed_traj or mpc_sensed_gg_traj per trajectory and
// mpc_held_shift per wavefront. The sensor arguments are validated by the library's own check_mpc_sensed, which
// emu_mpc_sensed_check exposes alone. Besides the entry point's outputs the driver returns x0 of the parameter records as the call
// leaves them (x0_after): what a following solve of the resident batch would start from.
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_mpc_sensed.hpp"

// arguments: the batch as emu_mpc_held_gg_batch (tsat_emu_gg.cpp; Rtab may be null with gm == 0), then s, sensor, Y_hist, x0_after
extern "C" int emu_mpc_held_sensed_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab, const double* x0,
                                         const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                         const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                         const double* Rd, const double* ulo, const double* uhi, const double* U0, int32_t n_steps,
                                         int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                                         const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist,
                                         tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last,
                                         double* U_last, const int32_t* n_knots, const double* Rtab, double gm,
                                         const tsat_sensor_options* s, const double* sensor, double* Y_hist, double* x0_after) {
  const int N = o->n_knots, n_tab = o->n_tab;
  if (!check_options(*o, N, n_tab, o->max_linesearch).empty() || o->precision != 64) return -1;
  if (!check_mpc_dispersed(*po, n_steps, step0, plant, sat_lo, sat_hi, T).empty()) return -1;
  if (Rtab && !check_gravity(Rtab, gm, n_btab * (int64_t)n_tab).empty()) return -1;
  if (!check_mpc_sensed(s, sensor, T, Rtab, gm).empty()) return -1;
  int min_nk = N;
  for (int64_t t = 0; n_knots && t < T; ++t) min_nk = n_knots[t] < min_nk ? n_knots[t] : min_nk;
  if (!check_mpc_held(replan_every, feedback, min_nk).empty()) return -1;
  const int max_ls = o->max_linesearch < NSTORE ? o->max_linesearch : NSTORE;
  std::vector<double> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), U0w(U0, U0 + (size_t)T * (N - 1) * 3),
      PL((size_t)T * HELD_W), SAT((size_t)T * SATW), GT, SN((size_t)T * SNW, -1.0), XT((size_t)T * MSX_W, -1.0);   // the pack writes every slot
  std::vector<int> bidx(T);
  std::vector<MpcDispRec> rec((size_t)T);
  pack_params<double>(T, x0, xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  for (int64_t t = 0; t < T; ++t) bidx[t] = btab_idx ? btab_idx[t] : (int)t;
  for (int64_t t = 0; t < T; ++t)
    for (int c = 0; c < 3; ++c) {
      SAT[SATW * t + c] = sat_lo ? sat_lo[3 * t + c] : -HUGE_VAL;
      SAT[SATW * t + 3 + c] = sat_hi ? sat_hi[3 * t + c] : HUGE_VAL;
    }
  for (int64_t t = 0; t < T; ++t) mpc_held_pack<double>(plant, P.data(), SAT.data(), o->u_scale, PL.data(), rec.data(), T, t);
  if (Rtab) {
    const int64_t rows = n_btab * (int64_t)n_tab;
    GT.resize((size_t)rows * 4);
    for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  }
  std::vector<double> XU((size_t)T * N * XUW, 0.0), KD((size_t)T * (N - 1) * KDW, 0.0),
      LAM((size_t)T * (N - 1) * LMW, 0.0), CAND((size_t)T * max_ls * N * XUW, 0.0), Yw;
  if (!Y_hist) { Yw.resize((size_t)T * n_steps * 7); Y_hist = Yw.data(); }
  KArgs<double> a;
  a.T = (int)T; a.N = N; a.n_tab = n_tab; a.max_ls = max_ls; a.opt = *o;
  a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = n_knots; a.U0 = U0w.data();
  a.XU = XU.data(); a.KD = KD.data(); a.LAM = LAM.data(); a.CAND = CAND.data();
  a.stats = stats_last; a.trace = nullptr; a.trace_rows = 0;
  MpcSensedArgs<double> ms = {};
  MpcHeldArgs<double>& mh = ms.h;
  MpcDispArgs<double>& md = mh.s;
  MpcArgs<double>& m = md.m;
  m.T = (int)T; m.N = N; m.n_tab = n_tab; m.plant_integ = 4; m.n_steps = n_steps; m.us = o->u_scale;
  m.P = P.data(); m.BT = BT.data(); m.bidx = bidx.data(); m.nk = n_knots; m.XU = XU.data(); m.U0 = U0w.data();
  m.HX = X_hist; m.HU = U_hist; m.stats = nullptr; m.tally = nullptr;
  md.d.PL = PL.data(); md.d.Mp = 1; md.d.SAT = SAT.data(); md.d.nclip = n_clipped;
  EnsArgs<double>& e = md.d.e;
  e.min_steps = po->min_steps; e.w_tol = po->w_tol; e.ang_tol = po->angle_tol;
  e.k0 = (unsigned)(po->noise_seed & 0xFFFFFFFFull); e.k1 = (unsigned)(po->noise_seed >> 32);
  e.nid0 = (const long long*)noise_id; e.sg = po->sigma_gyro; e.sa = po->sigma_att; e.fa = po->field_amp; e.stats = stats;
  md.noisy = po->noise_mode; md.step0 = (long long)step0; md.rec = rec.data();
  mh.KD = KD.data(); mh.feedback = feedback;
  ms.GT = Rtab ? GT.data() : nullptr; ms.XT = XT.data(); ms.HY = Y_hist;
  ms.s.SN = SN.data(); ms.s.Mp = (int)T; ms.s.sgy = s->sigma_gyro; ms.s.sat = s->sigma_att; ms.s.smg = s->sigma_mag;
  ms.s.latency = s->latency; ms.s.k0 = e.k0; ms.s.k1 = e.k1;
  for (int64_t t = 0; t < T; ++t) mpc_sensed_pack<double>(ms, sensor, t);
  const int cls = inertia_class(T, Jmat);
  using blk_t = void (*)(const KArgs<double>&, int);
  static const blk_t variants[2][3][2] = {
      {{run_block<3, 0, 0>, run_block<3, 0, 1>}, {run_block<3, 1, 0>, run_block<3, 1, 1>}, {run_block<3, 2, 0>, run_block<3, 2, 1>}},
      {{run_block<4, 0, 0>, run_block<4, 0, 1>}, {run_block<4, 1, 0>, run_block<4, 1, 1>}, {run_block<4, 2, 0>, run_block<4, 2, 1>}}};
  const blk_t blk = variants[o->integrator == 4 ? 1 : 0][cls][o->error_state ? 1 : 0];
  const int es = o->error_state ? 1 : 0;
  for (int sb = 0; sb < n_steps; sb += replan_every) {
    tsat_emu::for_each_wave((int)T, [&](int t) { blk(a, t); });
    m.step = sb;
    mh.r = replan_every < n_steps - sb ? replan_every : n_steps - sb;
    for (int t = 0; t < (int)T; ++t) {    // lane = trajectory: no lane of the hold talks to another
      if (ms.GT) es ? mpc_sensed_gg_traj<double, 1>(ms, t) : mpc_sensed_gg_traj<double, 0>(ms, t);
      else es ? mpc_sensed_traj<double, 1>(ms, t) : mpc_sensed_traj<double, 0>(ms, t);
    }
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_held_shift<double>(m, mh.r, t); });
  }
  for (int64_t ee = 0; ee < T * (int64_t)N; ++ee) export_record<double>(ee, N, n_knots, XU.data(), KD.data(), X_last, U_last, nullptr);
  if (x0_after)
    for (int64_t t = 0; t < T; ++t)
      for (int i = 0; i < 7; ++i) x0_after[7 * t + i] = P[(size_t)t * PSTRIDE + P_X0 + i];
  return 0;
}

// the argument checks tsat_mpc_run_held_sensed adds: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_sensed_check(const tsat_sensor_options* s, const double* sensor, int64_t T, const double* Rtab, double gm, char* text,
                                    int32_t cap) {
  const std::string why = check_mpc_sensed(s, sensor, T, Rtab, gm);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
