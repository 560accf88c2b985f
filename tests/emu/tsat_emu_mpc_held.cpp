// tsat_emu_mpc_held.cpp — the hold and the plan shift of tsat_mpc_run_held (tortoisesat.jl_amd/csrc/tsat_mpc_held.hpp) under the
// CPU lane emulator (TEST INFRASTRUCTURE): the driver of tsat_emu_mpc.hpp with neither an orbit table nor a sensor.
// emu_mpc_held_check exposes the library's check_mpc_held (tsat_host_pack.hpp) on its own.
#include "tsat_emu_mpc.hpp"

// arguments: the batch as emu_mpc_batch, then those of tsat_mpc_run_held (include/tortoise_hip.h), the last plan, n_knots
extern "C" int emu_mpc_held_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab, const double* x0,
                                       const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                       const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                       const double* Rd, const double* ulo, const double* uhi, const double* U0, int32_t n_steps,
                                       int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last,
                                       tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last, double* U_last,
                                       const int32_t* n_knots) {
  return emu_mpc_held({o, po, T, n_btab, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0, n_steps, step0, replan_every, feedback,
                    plant, sat_lo, sat_hi, noise_id, X_hist, U_hist, stats_last, stats, n_clipped, X_last, U_last, n_knots}, nullptr, 0.0, nullptr, nullptr, nullptr, nullptr);
}

// the argument checks tsat_mpc_run_held adds: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_held_check(int32_t replan_every, int32_t feedback, int32_t min_nk, char* text, int32_t cap) {
  const std::string why = check_mpc_held(replan_every, feedback, min_nk);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
