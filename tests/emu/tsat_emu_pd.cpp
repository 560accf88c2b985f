// tsat_emu_pd.cpp — the projection PD baseline (tortoisesat.jl_amd/csrc/tsat_pd.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE). The staging and the roll-out are those of tsat_emu_rollout.hpp, which follow the host code of tsat_pd_ensemble:
// the library's own check_pd first (emu_pd_check exposes it alone), the model's plant when the call gives none, then pd_wave /
// pd_gg_wave per wavefront.
#include "tsat_emu_rollout.hpp"

// arguments as tsat_pd_ensemble (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                               const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                               const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                               int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                               const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                               tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                               int32_t* n_clipped, const double* Rtab, double gm) {
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = EmuPd{kd, kp, feedforward, limit_mode, x0_nom};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  c.grav = EmuGravity{Rtab, gm};
  if (!pd_call_valid(c)) return -1;
  EmuBuffers b;
  const PdArgs<double> pa = stage_pd(c, b);
  return roll(c, b, [&](int t, int w) { pa.GT ? pd_gg_wave<double>(pa, t, w) : pd_wave<double>(pa, t, w); });
}

// the argument checks of the entry point: 0 and "" or -1 and the text tsat_ensemble_last_error would hold. Arguments as
// emu_pd_ensemble without noise_id0, X_sim and n_clipped (which nothing is asked of), then the text buffer
extern "C" int emu_pd_check(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                            const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                            const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                            int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int32_t* n_knots, const double* plant,
                            const double* sat_lo, const double* sat_hi, const void* stats, const double* summary,
                            const void* stats_nominal, const double* Rtab, double gm, char* text, int32_t cap) {
  return check_result(check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom,
                               n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm),
                      text, cap);
}
