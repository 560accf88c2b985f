// tsat_emu_pd.cpp — the projection PD baseline (tortoisesat.jl_amd/csrc/tsat_pd.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE). Takes run_wave / for_each_wave and the packing code from tsat_emu.cpp as they are. The driver follows the host
// code of tsat_pd_ensemble step by step: the library's own check_pd first (emu_pd_check exposes it alone), the model's plant when
// the call gives none, the plants packed by dispersed_pack and the orbit table by gg_pack_row, one call per thread of their
// grids, then pd_wave / pd_gg_wave per wavefront.
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_pd.hpp"

// arguments as tsat_pd_ensemble (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                               const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                               const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                               int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                               const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                               tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                               int32_t* n_clipped, const double* Rtab, double gm) {
  if (!check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom, n_knots,
                plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm).empty())
    return -1;
  const int N = o->n_knots, n_tab = o->n_tab;
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  const size_t Tn = (size_t)T, nS = Tn * (size_t)M;
  std::vector<double> P(Tn * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR, x0n(Tn * 7), zero(Tn * 6, 0.0), gain(Tn * PDGW),
      PL(Tn * PLW * Mp, 0.0), model, GT;
  const std::vector<double> SAT = pack_limits(sat_lo, sat_hi, T);
  std::vector<int> bidx(Tn);
  for (size_t t = 0; t < Tn; ++t) {
    bidx[t] = btab_idx ? btab_idx[t] : (int)t;
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = x0_nom ? x0_nom[7 * t + i] : (X ? X[t * N * 7 + i] : xf[7 * t + i]);
    for (int c = 0; c < 3; ++c) {
      gain[PDGW * t + c] = kd[3 * t + c];
      gain[PDGW * t + 3 + c] = kp[3 * t + c];
    }
  }
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, zero.data(), zero.data(), zero.data(), P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  if (X) {
    std::vector<double> U0;
    if (!feedforward) { U0.assign(Tn * (size_t)(N - 1) * 3, 0.0); U = U0.data(); }
    XUR.resize(Tn * N * XUW);
    pack_xu_records<double>(T, N, X, U, XUR.data());
  }
  if (!plant) {
    model = model_plants(Jmat, Tn, M);
    plant = model.data();
  }
  for (int64_t e = 0; e < T * (int64_t)(M + 1); ++e) dispersed_pack<double>(plant, P.data(), o->u_scale, PL.data(), T, M, Mp, e);
  if (Rtab) {
    const int64_t rows = n_btab * (int64_t)n_tab;
    GT.resize((size_t)rows * 4);
    for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  }
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * nS * N * 7);
  std::vector<tsat_tvlqr_stats> nom(Tn);
  PdArgs<double> pa;
  pa.d.e = ens_args<EnsArgs<double>>(*o, T, M, P.data(), BT.data(), bidx.data(), n_knots, X ? XUR.data() : nullptr, nullptr, x0_sim,
                                     (const long long*)noise_id0, X_sim, stats, nom.data());
  pa.d.PL = PL.data(); pa.d.Mp = Mp; pa.d.SAT = SAT.data(); pa.d.nclip = n_clipped;
  pa.GT = Rtab ? GT.data() : nullptr; pa.GAIN = gain.data(); pa.X0N = x0n.data(); pa.feedforward = feedforward; pa.limit_mode = limit_mode;
  tsat_emu::for_each_wave((int)T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() { pa.GT ? pd_gg_wave<double>(pa, t, w) : pd_wave<double>(pa, t, w); });   // the kernels use no LDS
  });
  if (stats_nominal) std::memcpy(stats_nominal, nom.data(), sizeof(tsat_tvlqr_stats) * Tn);
  ensemble_summary(T, M, stats, summary);
  return 0;
}

// the argument checks of the entry point: 0 and "" or -1 and the text tsat_ensemble_last_error would hold. Arguments as
// emu_pd_ensemble without noise_id0, X_sim and n_clipped (which nothing is asked of), then the text buffer
extern "C" int emu_pd_check(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                            const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                            const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                            int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int32_t* n_knots, const double* plant,
                            const double* sat_lo, const double* sat_hi, const void* stats, const double* summary,
                            const void* stats_nominal, const double* Rtab, double gm, char* text, int32_t cap) {
  const std::string why = check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim,
                                   x0_nom, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
