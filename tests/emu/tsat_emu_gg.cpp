// tsat_emu_gg.cpp — the gravity-gradient ensemble and hold (tortoisesat.jl_amd/csrc/tsat_gg.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE). The ensemble is the dispersed call of tsat_emu_rollout.hpp with the orbit table packed by the product's own
// gg_pack_row and gg_wave in place of dispersed_wave; the hold is the driver of tsat_emu_mpc.hpp with the orbit table. The table is
// validated by the library's own check_gravity, which emu_gg_check exposes.
#include "tsat_emu_mpc.hpp"
#include "tsat_emu_rollout.hpp"

// arguments as tsat_tvlqr_ensemble_gg (include/tortoise_hip.h), with K_lqr 3 x 6 x (N-1) x T as an INPUT (before `stats`); the
// plants are taken as valid
extern "C" int emu_tvlqr_ensemble_gg(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                     const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                     const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                     const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                     const double* plant, const double* sat_lo, const double* sat_hi, const double* K_lqr,
                                     tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                                     int32_t* n_clipped, const double* Rtab, double gm) {
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = EmuTv{Qd, Qfd, Rd, K_lqr};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  c.grav = EmuGravity{Rtab, gm};
  if (!tv_call_valid(c)) return -1;
  EmuBuffers b;
  const GgEnsArgs<double> g = stage_tv(c, b);
  return roll(c, b, [&](int t, int w) { gg_wave<double>(g, t, w); });
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
  return check_result(check_gravity(Rtab, gm, rows), text, cap);
}
