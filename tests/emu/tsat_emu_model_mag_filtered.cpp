// tsat_emu_model_mag_filtered.cpp — the ensemble controllers behind the model-based rate filter updated by the magnetometer
// (tortoisesat.jl_amd/csrc/tsat_model_mag_filtered.hpp) under the CPU lane emulator (TEST INFRASTRUCTURE). tsat_emu_filtered.cpp with the
// filter exchanged (ModelMagEkf below): the drivers are filtered_tv / filtered_pd of tsat_emu_rollout.hpp. The filter options are
// validated by the library's own check_model_mag_filter, which emu_model_mag_filter_check exposes alone.
#include "tsat_emu_sensed.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_model_mag_filtered.hpp"

namespace {
struct ModelMagEkf {
  using Options = tsat_model_mag_filter_options;
  using TvArgs = ModelMagFilteredTvArgs<double>;
  using PdArgs = ModelMagFilteredPdArgs<double>;
  static std::string check(const Options* f) { return check_model_mag_filter(f); }
  static auto args(const Options& f, const SensArgs<double>& sa, const EnsArgs<double>& e, double* XH, double* FF) {
    return model_mag_filt_args(f, sa, e, XH, FF);
  }
  static void tv(const TvArgs& a, int t, int w) { model_mag_filtered_tv_wave<double>(a, t, w); }
  static void tv_gg(const TvArgs& a, int t, int w) { model_mag_filtered_tv_gg_wave<double>(a, t, w); }
  static void pd(const PdArgs& a, int t, int w) { model_mag_filtered_pd_wave<double>(a, t, w); }
  static void pd_gg(const PdArgs& a, int t, int w) { model_mag_filtered_pd_gg_wave<double>(a, t, w); }
};
}  // namespace

// arguments as tsat_tvlqr_ensemble_model_mag_filtered (include/tortoise_hip.h) without the handle, with K_lqr as an INPUT before `stats`
extern "C" int emu_tvlqr_ensemble_model_mag_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                           const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                           const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                           const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                           const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                           const double* K_lqr, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                           double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                           const double* sensor, const tsat_model_mag_filter_options* f, double* X_hat, double* filt_final) {
  return filtered_tv<ModelMagEkf>(sensed_tv_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                                        plant, sat_lo, sat_hi, K_lqr, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, s, sensor),
                         f, X_hat, filt_final);
}

// arguments as tsat_pd_ensemble_model_mag_filtered (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble_model_mag_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                        const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                        const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                        int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                        const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                        const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                        double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                        const double* sensor, const tsat_model_mag_filter_options* f, double* X_hat, double* filt_final) {
  return filtered_pd<ModelMagEkf>(sensed_pd_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode,
                                        x0_sim, x0_nom, noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim,
                                        n_clipped, Rtab, gm, s, sensor),
                         f, X_hat, filt_final);
}

// check_model_mag_filter alone: 0 and "" or -1 and the text tsat_ensemble_last_error would hold
extern "C" int emu_model_mag_filter_check(const tsat_model_mag_filter_options* f, char* text, int32_t cap) {
  return check_result(check_model_mag_filter(f), text, cap);
}
