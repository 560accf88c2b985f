// tsat_emu_model_mag_sun_filtered.cpp — the ensemble controllers behind the magnetometer-updated model filter with a sun sensor
// (tortoisesat.jl_amd/csrc/tsat_model_mag_sun_filtered.hpp) under the CPU lane emulator (TEST INFRASTRUCTURE). The calls end with
// the sun table and sigma_sun, which the Family template of tsat_emu_rollout.hpp does not carry: the two drivers below are its
// filtered_tv / filtered_pd with the sun rows packed by the product's pack of the field rows and the dispatch of the entry points
// (f == NULL: the emulated sensed call; Stab == NULL: the emulated model-mag-filtered call on the seven shared options). The
// options, sigma_sun and the table are validated by the library's own check_model_mag_sun_filter, which
// emu_model_mag_sun_filter_check exposes alone.
#include "tsat_emu_sensed.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_model_mag_sun_filtered.hpp"

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

std::vector<double> packed_sun_rows(const EmuCall& c, const double* Stab) {
  std::vector<double> ST((size_t)c.n_btab * c.o->n_tab * 4);
  pack_btab<double>(c.n_btab, c.o->n_tab, Stab, ST.data());
  return ST;
}

int sun_tv(EmuCall c, const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final, const double* Stab, double sigma_sun) {
  if (!check_sun_arguments(f != nullptr, Stab, sigma_sun).empty()) return -1;
  if (!Stab) {
    tsat_model_mag_filter_options g;
    if (f) g = model_mag_options_of(*f);
    return filtered_tv<ModelMagEkf>(c, f ? &g : nullptr, X_hat, filt_final);
  }
  c.filt = EmuFiltering{X_hat, filt_final};
  if (!tv_call_valid(c) || !check_model_mag_sun_filter(f, Stab, sigma_sun, c.n_btab * (int64_t)c.o->n_tab).empty()) return -1;
  EmuBuffers b;
  const std::vector<double> ST = packed_sun_rows(c, Stab);
  ModelMagSunFilteredTvArgs<double> a;
  a.g = stage_tv(c, b);
  a.f = model_mag_sun_filt_args(*f, sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp), a.g.d.e, X_hat, filt_final, ST.data(), sigma_sun);
  return roll(c, b, [&](int t, int w) {
    a.g.GT ? model_mag_sun_filtered_tv_gg_wave<double>(a, t, w) : model_mag_sun_filtered_tv_wave<double>(a, t, w);
  });
}

int sun_pd(EmuCall c, const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final, const double* Stab, double sigma_sun) {
  if (!check_sun_arguments(f != nullptr, Stab, sigma_sun).empty()) return -1;
  if (!Stab) {
    tsat_model_mag_filter_options g;
    if (f) g = model_mag_options_of(*f);
    return filtered_pd<ModelMagEkf>(c, f ? &g : nullptr, X_hat, filt_final);
  }
  c.filt = EmuFiltering{X_hat, filt_final};
  if (!pd_call_valid(c) || !check_model_mag_sun_filter(f, Stab, sigma_sun, c.n_btab * (int64_t)c.o->n_tab).empty()) return -1;
  EmuBuffers b;
  const std::vector<double> ST = packed_sun_rows(c, Stab);
  ModelMagSunFilteredPdArgs<double> a;
  a.p = stage_pd(c, b);
  a.f = model_mag_sun_filt_args(*f, sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp), a.p.d.e, X_hat, filt_final, ST.data(), sigma_sun);
  return roll(c, b, [&](int t, int w) {
    a.p.GT ? model_mag_sun_filtered_pd_gg_wave<double>(a, t, w) : model_mag_sun_filtered_pd_wave<double>(a, t, w);
  });
}
}  // namespace

// arguments as tsat_tvlqr_ensemble_model_mag_sun_filtered (include/tortoise_hip.h) without the handle, with K_lqr as an INPUT before `stats`
extern "C" int emu_tvlqr_ensemble_model_mag_sun_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                           const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                           const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                           const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                           const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                           const double* K_lqr, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                           double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                           const double* sensor, const tsat_model_mag_sun_filter_options* f, double* X_hat,
                                           double* filt_final, const double* Stab, double sigma_sun) {
  return sun_tv(sensed_tv_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                               plant, sat_lo, sat_hi, K_lqr, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, s, sensor),
                f, X_hat, filt_final, Stab, sigma_sun);
}

// arguments as tsat_pd_ensemble_model_mag_sun_filtered (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble_model_mag_sun_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                        const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                        const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                        int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                        const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                        const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                        double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                        const double* sensor, const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final,
                                        const double* Stab, double sigma_sun) {
  return sun_pd(sensed_pd_call(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode,
                               x0_sim, x0_nom, noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim,
                               n_clipped, Rtab, gm, s, sensor),
                f, X_hat, filt_final, Stab, sigma_sun);
}

// check_sun_arguments, then check_model_mag_sun_filter alone on a table of `rows` rows: 0 and "" or -1
// and the text tsat_ensemble_last_error would hold. Stab == NULL with f given checks the seven shared options as the parent does.
extern "C" int emu_model_mag_sun_filter_check(const tsat_model_mag_sun_filter_options* f, const double* Stab, double sigma_sun, int64_t rows,
                                              char* text, int32_t cap) {
  const std::string bad = check_sun_arguments(f != nullptr, Stab, sigma_sun);
  if (!bad.empty()) return check_result(bad, text, cap);
  if (!Stab && f) {
    const tsat_model_mag_filter_options g = model_mag_options_of(*f);
    return check_result(check_model_mag_filter(&g), text, cap);
  }
  return check_result(check_model_mag_sun_filter(f, Stab, sigma_sun, rows), text, cap);
}
