// tsat_emu_mpc_sensed.cpp — the held re-planning loop fed measurements (tortoisesat.jl_amd/csrc/tsat_mpc_sensed.hpp) under the CPU
// lane emulator (TEST INFRASTRUCTURE): the driver of tsat_emu_mpc.hpp with a sensor, and the orbit table when there is one. The
// sensor arguments are validated by the library's own check_mpc_sensed, which emu_mpc_sensed_check exposes alone.
#include "tsat_emu_mpc.hpp"

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
  if (!s) return -1;
  return emu_mpc_held({o, po, T, n_btab, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0, n_steps, step0, replan_every, feedback,
                    plant, sat_lo, sat_hi, noise_id, X_hist, U_hist, stats_last, stats, n_clipped, X_last, U_last, n_knots}, Rtab, gm, s, sensor, Y_hist, x0_after);
}

// the argument checks tsat_mpc_run_held_sensed adds: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_sensed_check(const tsat_sensor_options* s, const double* sensor, int64_t T, const double* Rtab, double gm, char* text,
                                    int32_t cap) {
  const std::string why = check_mpc_sensed(s, sensor, T, Rtab, gm);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
