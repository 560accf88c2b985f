// tsat_emu_ensemble.cpp — the ensemble tracking kernels (tortoisesat.jl_amd/csrc/tsat_ensemble.hpp, tsat_dispersed.hpp) under the
// CPU lane emulator (TEST INFRASTRUCTURE). Takes the run_wave / for_each_wave machinery and the packing code from tsat_emu.cpp as
// it is and adds one driver for both entry points: the gains come in as an array (from the emulated tracking kernel or the
// oracle), ensemble_wave or — with plants — dispersed_wave runs with lane = realisation, the per-lane plant records are made by
// the product's own pack function (dispersed_pack), one call per thread of its grid, the summary by its own host function.
#include <cmath>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_dispersed.hpp"

// both symbols: `plant` == nullptr is emu_tvlqr_ensemble
static int run_emu_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                            const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                            const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                            const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                            const double* sat_lo, const double* sat_hi, const double* K_lqr, tsat_tvlqr_stats* stats, double* summary,
                            tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped) {
  if (!check_tv_options(*o).empty() || o->noise_mode != 1 || o->rate_as_written != 0 || M < 1 || M > 65535) return -1;
  const int N = o->n_knots, n_tab = o->n_tab;
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  std::vector<double> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR((size_t)T * N * XUW),
      KD((size_t)T * (N - 1) * KDW, 0.0), x0n((size_t)T * 7), PL(plant ? (size_t)T * PLW * Mp : 0, 0.0), SAT;
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
  if (plant) {
    SAT = pack_limits(sat_lo, sat_hi, T);
    for (int64_t e = 0; e < T * (int64_t)(M + 1); ++e) dispersed_pack<double>(plant, P.data(), o->u_scale, PL.data(), T, M, Mp, e);
  }
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * (size_t)T * M * N * 7);
  std::vector<tsat_tvlqr_stats> nom((size_t)T);
  DispArgs<double> d;
  EnsArgs<double>& a = d.e;
  a = ens_args<EnsArgs<double>>(*o, T, M, P.data(), BT.data(), bidx.data(), n_knots, XUR.data(), KD.data(), x0_sim,
                                (const long long*)noise_id0, X_sim, stats, nom.data());
  d.PL = PL.data(); d.Mp = Mp; d.SAT = SAT.data(); d.nclip = n_clipped;
  const int cls = inertia_class(T, Jmat);
  tsat_emu::for_each_wave((int)T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() {                             // the kernels use no LDS
      if (plant) dispersed_wave<double>(d, t, w);
      else if (cls == 2) ensemble_wave<double, 2>(a, t, w);
      else if (cls == 1) ensemble_wave<double, 1>(a, t, w);
      else ensemble_wave<double, 0>(a, t, w);
    });
  });
  if (stats_nominal) std::memcpy(stats_nominal, nom.data(), sizeof(tsat_tvlqr_stats) * (size_t)T);
  ensemble_summary(T, M, stats, summary);
  return 0;
}

// arguments as tsat_tvlqr_ensemble (include/tortoise_hip.h), with K_lqr 3 x 6 x (N-1) x T as an INPUT
extern "C" int emu_tvlqr_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                  const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                  const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                  const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                  const int32_t* n_knots, const double* K_lqr, tsat_tvlqr_stats* stats, double* summary,
                                  tsat_tvlqr_stats* stats_nominal, double* X_sim) {
  return run_emu_ensemble(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                          nullptr, nullptr, nullptr, K_lqr, stats, summary, stats_nominal, X_sim, nullptr);
}

// arguments as tsat_tvlqr_ensemble_dispersed (include/tortoise_hip.h), with K_lqr 3 x 6 x (N-1) x T as an INPUT; the plants are
// taken as valid (the validation is host code of the library, checked on the GPU tier)
extern "C" int emu_tvlqr_ensemble_dispersed(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                            const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                            const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                                            const double* Qd, const double* Qfd, const double* Rd, const double* x0_sim,
                                            const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                                            const double* sat_lo, const double* sat_hi, const double* K_lqr, tsat_tvlqr_stats* stats,
                                            double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped) {
  if (!plant || ((sat_lo == nullptr) != (sat_hi == nullptr))) return -1;
  return run_emu_ensemble(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                          plant, sat_lo, sat_hi, K_lqr, stats, summary, stats_nominal, X_sim, n_clipped);
}

// the summary function alone, on statistics of the caller's making
extern "C" void emu_ensemble_summary(int64_t T, int32_t M, const tsat_tvlqr_stats* stats, double* summary) {
  ensemble_summary(T, M, stats, summary);
}
