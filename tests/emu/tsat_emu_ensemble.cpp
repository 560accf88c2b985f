// tsat_emu_ensemble.cpp — the ensemble tracking kernels (tortoisesat.jl_amd/csrc/tsat_ensemble.hpp, tsat_dispersed.hpp) under the
// CPU lane emulator (TEST INFRASTRUCTURE). The staging and the roll-out are those of tsat_emu_rollout.hpp: the gains come in as an
// array (from the emulated tracking kernel or the oracle), ensemble_wave of the model's inertia class or — with plants —
// dispersed_wave runs with lane = realisation.
#include "tsat_emu_rollout.hpp"

// arguments as tsat_tvlqr_ensemble (include/tortoise_hip.h), with K_lqr 3 x 6 x (N-1) x T as an INPUT
extern "C" int emu_tvlqr_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                  const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                  const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                  const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                  const int32_t* n_knots, const double* K_lqr, tsat_tvlqr_stats* stats, double* summary,
                                  tsat_tvlqr_stats* stats_nominal, double* X_sim) {
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = EmuTv{Qd, Qfd, Rd, K_lqr};
  if (!tv_call_valid(c)) return -1;
  EmuBuffers b;
  const EnsArgs<double> a = stage_tv(c, b).d.e;
  const int cls = inertia_class(T, Jmat);
  return roll(c, b, [&](int t, int w) {
    if (cls == 2) ensemble_wave<double, 2>(a, t, w);
    else if (cls == 1) ensemble_wave<double, 1>(a, t, w);
    else ensemble_wave<double, 0>(a, t, w);
  });
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
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = EmuTv{Qd, Qfd, Rd, K_lqr};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  if (!tv_call_valid(c)) return -1;
  EmuBuffers b;
  const DispArgs<double> d = stage_tv(c, b).d;
  return roll(c, b, [&](int t, int w) { dispersed_wave<double>(d, t, w); });
}

// the summary function alone, on statistics of the caller's making
extern "C" void emu_ensemble_summary(int64_t T, int32_t M, const tsat_tvlqr_stats* stats, double* summary) {
  ensemble_summary(T, M, stats, summary);
}
