// tsat_emu_gg.cpp — the gravity-gradient ensemble and hold (tortoisesat.jl_amd/csrc/tsat_gg.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE). Takes run_wave / for_each_wave, the emulated solve (run_block) and the packing code from tsat_emu.cpp as they
// are. The ensemble driver is that of tsat_emu_ensemble.cpp (its dispersed branch) with the orbit table packed by the product's own
// gg_pack_row, one call per thread of its grid, and gg_wave in place of dispersed_wave; the hold is the driver of tsat_emu_mpc.hpp
// with the orbit table. The table is validated by the library's own check_gravity, which emu_gg_check exposes.
#include "tsat_emu_mpc.hpp"

static std::vector<double> gg_rows(const double* Rtab, double gm, int64_t rows) {
  std::vector<double> GT((size_t)rows * 4);
  for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  return GT;
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
      KD((size_t)T * (N - 1) * KDW, 0.0), x0n((size_t)T * 7), PL((size_t)T * PLW * Mp, 0.0);
  const std::vector<double> SAT = pack_limits(sat_lo, sat_hi, T);
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
  for (int64_t e = 0; e < T * (int64_t)(M + 1); ++e) dispersed_pack<double>(plant, P.data(), o->u_scale, PL.data(), T, M, Mp, e);
  const std::vector<double> GT = gg_rows(Rtab, gm, n_btab * (int64_t)n_tab);
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * (size_t)T * M * N * 7);
  std::vector<tsat_tvlqr_stats> nom((size_t)T);
  GgEnsArgs<double> g;
  DispArgs<double>& d = g.d;
  EnsArgs<double>& a = d.e;
  a = ens_args<EnsArgs<double>>(*o, T, M, P.data(), BT.data(), bidx.data(), n_knots, XUR.data(), KD.data(), x0_sim,
                                (const long long*)noise_id0, X_sim, stats, nom.data());
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
  if (!Rtab) return -1;
  return emu_mpc_held({o, po, T, n_btab, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0, n_steps, step0, replan_every, feedback,
                    plant, sat_lo, sat_hi, noise_id, X_hist, U_hist, stats_last, stats, n_clipped, X_last, U_last, n_knots}, Rtab, gm, nullptr, nullptr, nullptr, nullptr);
}

// the argument checks the two entry points add: 0 and "" or -1 and the text their error functions would hold
extern "C" int emu_gg_check(const double* Rtab, double gm, int64_t rows, char* text, int32_t cap) {
  const std::string why = check_gravity(Rtab, gm, rows);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
