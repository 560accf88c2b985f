// tsat_emu_gg.cpp — the gravity-gradient ensemble and hold (tortoisesat.jl_amd/csrc/tsat_gg.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE). Takes run_wave / for_each_wave, the emulated solve (run_block) and the packing code from tsat_emu.cpp as they
// are. The two drivers are those of tsat_emu_ensemble.cpp (its dispersed branch) and tsat_emu_mpc_held.cpp with the orbit table
// packed by the product's own gg_pack_row, one call per thread of its grid, and gg_wave / mpc_held_gg_block in place of
// dispersed_wave / mpc_held_block; the orbit table is validated by the library's own check_gravity, which emu_gg_check exposes.
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_gg.hpp"

static std::vector<double> gg_rows(const double* Rtab, double gm, int64_t rows) {
  std::vector<double> GT((size_t)rows * 4);
  for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  return GT;
}
static void limits(const double* sat_lo, const double* sat_hi, int64_t T, std::vector<double>& SAT) {
  for (int64_t t = 0; t < T; ++t)
    for (int c = 0; c < 3; ++c) {
      SAT[SATW * t + c] = sat_lo ? sat_lo[3 * t + c] : -HUGE_VAL;
      SAT[SATW * t + 3 + c] = sat_hi ? sat_hi[3 * t + c] : HUGE_VAL;
    }
}

// arguments as tsat_tvlqr_ensemble_gg (include/tortoise_hip.h), with K_lqr 3 x 6 x (N-1) x T as an INPUT (before `stats`); the
// plants are taken as valid
extern "C" int emu_tvlqr_ensemble_gg(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                     const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                     const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                     const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                     const double* plant, const double* sat_lo, const double* sat_hi, const double* K_lqr,
                                     tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                                     int32_t* n_clipped, const double* Rtab, double gm) {
  if (!check_tv_options(*o).empty() || o->noise_mode != 1 || o->rate_as_written != 0 || M < 1 || M > 65535) return -1;
  if (!plant || ((sat_lo == nullptr) != (sat_hi == nullptr))) return -1;
  const int N = o->n_knots, n_tab = o->n_tab;
  if (!check_gravity(Rtab, gm, n_btab * (int64_t)n_tab).empty()) return -1;
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  std::vector<double> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR((size_t)T * N * XUW),
      KD((size_t)T * (N - 1) * KDW, 0.0), x0n((size_t)T * 7), PL((size_t)T * PLW * Mp, 0.0), SAT((size_t)T * SATW);
  std::vector<int> bidx(T);
  for (int64_t t = 0; t < T; ++t)
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = X[(size_t)t * N * 7 + i];
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  pack_xu_records<double>(T, N, X, U, XUR.data());
  for (int64_t t = 0; t < T; ++t) bidx[t] = btab_idx ? btab_idx[t] : (int)t;
  for (size_t ek = 0; ek < (size_t)T * (N - 1); ++ek)        // the inverse of unpack_tv: solver sign, rows of 7
    for (int j = 0; j < 6; ++j)
      for (int c = 0; c < 3; ++c) KD[ek * KDW + c * 7 + j] = -K_lqr[ek * 18 + j * 3 + c];
  limits(sat_lo, sat_hi, T, SAT);
  for (int64_t e = 0; e < T * (int64_t)(M + 1); ++e) dispersed_pack<double>(plant, P.data(), o->u_scale, PL.data(), T, M, Mp, e);
  const std::vector<double> GT = gg_rows(Rtab, gm, n_btab * (int64_t)n_tab);
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * (size_t)T * M * N * 7);
  std::vector<tsat_tvlqr_stats> nom((size_t)T);
  GgEnsArgs<double> g;
  DispArgs<double>& d = g.d;
  EnsArgs<double>& a = d.e;
  a.T = (int)T; a.N = N; a.n_tab = n_tab; a.M = M; a.min_steps = o->min_steps;
  a.us = o->u_scale; a.w_tol = o->w_tol; a.ang_tol = o->angle_tol;
  a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = n_knots; a.XUR = XUR.data(); a.KD = KD.data(); a.X0 = x0_sim;
  a.k0 = (unsigned)(o->noise_seed & 0xFFFFFFFFull); a.k1 = (unsigned)(o->noise_seed >> 32);
  a.nid0 = (const long long*)noise_id0; a.sg = o->sigma_gyro; a.sa = o->sigma_att; a.fa = o->field_amp;
  a.XS = X_sim; a.stats = stats; a.stats_nom = nom.data();
  d.PL = PL.data(); d.Mp = Mp; d.SAT = SAT.data(); d.nclip = n_clipped;
  g.GT = GT.data();
  tsat_emu::for_each_wave((int)T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() { gg_wave<double>(g, t, w); });   // the kernel uses no LDS
  });
  if (stats_nominal) std::memcpy(stats_nominal, nom.data(), sizeof(tsat_tvlqr_stats) * (size_t)T);
  ensemble_summary(T, M, stats, summary);
  return 0;
}

// arguments: the batch as emu_mpc_held_batch (tsat_emu_mpc_held.cpp), then Rtab and gm
extern "C" int emu_mpc_held_gg_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab, const double* x0,
                                     const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                     const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                     const double* Rd, const double* ulo, const double* uhi, const double* U0, int32_t n_steps,
                                     int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                                     const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist,
                                     tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last,
                                     double* U_last, const int32_t* n_knots, const double* Rtab, double gm) {
  const int N = o->n_knots, n_tab = o->n_tab;
  if (!check_options(*o, N, n_tab, o->max_linesearch).empty() || o->precision != 64) return -1;
  if (!check_mpc_dispersed(*po, n_steps, step0, plant, sat_lo, sat_hi, T).empty()) return -1;
  if (!check_gravity(Rtab, gm, n_btab * (int64_t)n_tab).empty()) return -1;
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
  limits(sat_lo, sat_hi, T, SAT);
  for (int64_t t = 0; t < T; ++t) mpc_held_pack<double>(plant, P.data(), SAT.data(), o->u_scale, PL.data(), rec.data(), T, t);
  const std::vector<double> GT = gg_rows(Rtab, gm, n_btab * (int64_t)n_tab);
  std::vector<double> XU((size_t)T * N * XUW, 0.0), KD((size_t)T * (N - 1) * KDW, 0.0),
      LAM((size_t)T * (N - 1) * LMW, 0.0), CAND((size_t)T * max_ls * N * XUW, 0.0);
  KArgs<double> a;
  a.T = (int)T; a.N = N; a.n_tab = n_tab; a.max_ls = max_ls; a.opt = *o;
  a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = n_knots; a.U0 = U0w.data();
  a.XU = XU.data(); a.KD = KD.data(); a.LAM = LAM.data(); a.CAND = CAND.data();
  a.stats = stats_last; a.trace = nullptr; a.trace_rows = 0;
  MpcHeldGgArgs<double> mg = {};
  MpcHeldArgs<double>& mh = mg.h;
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
  mg.GT = GT.data();
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
      es ? mpc_held_gg_block<double, 1>(mg, t) : mpc_held_gg_block<double, 0>(mg, t);
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_held_shift<double>(m, mh.r, t); });
  }
  for (int64_t ee = 0; ee < T * (int64_t)N; ++ee) export_record<double>(ee, N, n_knots, XU.data(), KD.data(), X_last, U_last, nullptr);
  return 0;
}

// the argument checks the two entry points add: 0 and "" or -1 and the text their error functions would hold
extern "C" int emu_gg_check(const double* Rtab, double gm, int64_t rows, char* text, int32_t cap) {
  const std::string why = check_gravity(Rtab, gm, rows);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
