// tsat_emu_sensed.cpp — the ensemble controllers fed measurements (tortoisesat.jl_amd/csrc/tsat_sensed.hpp) under the CPU lane
// emulator (TEST INFRASTRUCTURE). The two drivers are sensed_tv and sensed_pd of tsat_emu_rollout.hpp: like the entry points they
// take the model's plant for a NULL plant and the kernels without gravity rows for a NULL Rtab. Here are the two calls as EmuCall
// (the four filter files, which include this one, extend them) and the symbols. The sensor arguments are validated by the library's
// own check_sensor, which emu_sensed_check exposes alone.
#include "tsat_emu_rollout.hpp"

// the arguments of emu_tvlqr_ensemble_sensed, in its order, as a call
static EmuCall sensed_tv_call(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                              const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                              const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                              const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                              const double* sat_lo, const double* sat_hi, const double* K_lqr, tsat_tvlqr_stats* stats, double* summary,
                              tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                              const tsat_sensor_options* s, const double* sensor) {
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = EmuTv{Qd, Qfd, Rd, K_lqr};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  c.grav = EmuGravity{Rtab, gm};
  c.sens = EmuSensing{s, sensor};
  return c;
}

// ... and of emu_pd_ensemble_sensed
static EmuCall sensed_pd_call(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                              const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                              const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                              int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                              const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                              tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped,
                              const double* Rtab, double gm, const tsat_sensor_options* s, const double* sensor) {
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = EmuPd{kd, kp, feedforward, limit_mode, x0_nom};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  c.grav = EmuGravity{Rtab, gm};
  c.sens = EmuSensing{s, sensor};
  return c;
}

// arguments as tsat_tvlqr_ensemble_sensed (include/tortoise_hip.h) without the handle, with K_lqr 3 x 6 x (N-1) x T as an INPUT
// (before `stats`, as emu_tvlqr_ensemble_gg); the plants are taken as valid
extern "C" int emu_tvlqr_ensemble_sensed(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                         const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                         const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                         const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                         const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                         const double* K_lqr, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                         const double* sensor) {
  return sensed_tv(sensed_tv_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                                  plant, sat_lo, sat_hi, K_lqr, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, s, sensor));
}

// arguments as tsat_pd_ensemble_sensed (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble_sensed(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                      const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                      const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                      int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                      const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                      const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                      double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                      const double* sensor) {
  return sensed_pd(sensed_pd_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim,
                                  x0_nom, noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm,
                                  s, sensor));
}

// check_sensor alone: 0 and "" or -1 and the text tsat_ensemble_last_error would hold
extern "C" int emu_sensed_check(const tsat_sensor_options* s, const double* sensor, int64_t T, int32_t M, char* text, int32_t cap) {
  return check_result(check_sensor(s, sensor, T, M), text, cap);
}
