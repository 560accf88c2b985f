// tsat_emu_mpc_held.cpp — the hold and the plan shift of tsat_mpc_run_held (tortoisesat.jl_amd/csrc/tsat_mpc_held.hpp) under the
// CPU lane emulator (TEST INFRASTRUCTURE). Takes run_wave / for_each_wave, the emulated solve (run_block) and the packing code
// from tsat_emu.cpp as they are and adds the loop of tsat_mpc_run_held: per block the emulated solve of every trajectory, then
// mpc_held_block per trajectory and mpc_held_shift per wavefront; the records are made by the product's own pack function, one
// call per thread of its grid. The arguments are validated by the library's own host functions (check_mpc_dispersed,
// check_mpc_held of tsat_host_pack.hpp); emu_mpc_held_check exposes the second on its own.
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_mpc_held.hpp"

// arguments: the batch as emu_mpc_batch, then those of tsat_mpc_run_held (include/tortoise_hip.h), the last plan, n_knots
extern "C" int emu_mpc_held_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab, const double* x0,
                                       const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                       const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                       const double* Rd, const double* ulo, const double* uhi, const double* U0, int32_t n_steps,
                                       int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last,
                                       tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last, double* U_last,
                                       const int32_t* n_knots) {
  const int N = o->n_knots, n_tab = o->n_tab;
  if (!check_options(*o, N, n_tab, o->max_linesearch).empty() || o->precision != 64) return -1;
  if (!check_mpc_dispersed(*po, n_steps, step0, plant, sat_lo, sat_hi, T).empty()) return -1;
  int min_nk = N;
  for (int64_t t = 0; n_knots && t < T; ++t) min_nk = n_knots[t] < min_nk ? n_knots[t] : min_nk;
  if (!check_mpc_held(replan_every, feedback, min_nk).empty()) return -1;
  const int max_ls = o->max_linesearch < NSTORE ? o->max_linesearch : NSTORE;
  std::vector<double> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), U0w(U0, U0 + (size_t)T * (N - 1) * 3),
      PL((size_t)T * HELD_W), SAT((size_t)T * SATW);
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
  std::vector<double> XU((size_t)T * N * XUW, 0.0), KD((size_t)T * (N - 1) * KDW, 0.0),
      LAM((size_t)T * (N - 1) * LMW, 0.0), CAND((size_t)T * max_ls * N * XUW, 0.0);
  KArgs<double> a;
  a.T = (int)T; a.N = N; a.n_tab = n_tab; a.max_ls = max_ls; a.opt = *o;
  a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = n_knots; a.U0 = U0w.data();
  a.XU = XU.data(); a.KD = KD.data(); a.LAM = LAM.data(); a.CAND = CAND.data();
  a.stats = stats_last; a.trace = nullptr; a.trace_rows = 0;
  MpcHeldArgs<double> mh = {};
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
  const int cls = inertia_class(T, Jmat);
  using blk_t = void (*)(const KArgs<double>&, int);
  static const blk_t variants[2][3][2] = {
      {{run_block<3, 0, 0>, run_block<3, 0, 1>}, {run_block<3, 1, 0>, run_block<3, 1, 1>}, {run_block<3, 2, 0>, run_block<3, 2, 1>}},
      {{run_block<4, 0, 0>, run_block<4, 0, 1>}, {run_block<4, 1, 0>, run_block<4, 1, 1>}, {run_block<4, 2, 0>, run_block<4, 2, 1>}}};
  const blk_t blk = variants[o->integrator == 4 ? 1 : 0][cls][o->error_state ? 1 : 0];
  const int es = o->error_state ? 1 : 0;
  for (int s = 0; s < n_steps; s += replan_every) {
    tsat_emu::for_each_wave((int)T, [&](int t) { blk(a, t); });
    m.step = s;
    mh.r = replan_every < n_steps - s ? replan_every : n_steps - s;
    for (int t = 0; t < (int)T; ++t)      // lane = trajectory: no lane of the hold talks to another
      es ? mpc_held_block<double, 1>(mh, t) : mpc_held_block<double, 0>(mh, t);
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_held_shift<double>(m, mh.r, t); });
  }
  for (int64_t ee = 0; ee < T * (int64_t)N; ++ee) export_record<double>(ee, N, n_knots, XU.data(), KD.data(), X_last, U_last, nullptr);
  return 0;
}

// the argument checks tsat_mpc_run_held adds: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_held_check(int32_t replan_every, int32_t feedback, int32_t min_nk, char* text, int32_t cap) {
  const std::string why = check_mpc_held(replan_every, feedback, min_nk);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
