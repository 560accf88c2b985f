// tsat_emu_mag_bias_filtered.cpp — the ensemble controllers behind the magnetometer-updated EKF that estimates the magnetometer bias
// (tortoisesat.jl_amd/csrc/tsat_mag_bias_filtered.hpp) under the CPU lane emulator (TEST INFRASTRUCTURE). tsat_emu_mag_filtered.cpp with
// the filter exchanged: it takes tsat_emu_sensed.cpp as it is — its packing (Common), its argument blocks and its two drivers — and
// adds the drivers of the four mag-bias-filtered waves: those of the sensed calls with the filter's block, X_hat zero-filled as the
// entry points zero it. f == NULL dispatches to the sensed driver, as the entry points do. The filter options are validated by the
// library's own check_mag_bias_filter, which emu_mag_bias_filter_check exposes alone.
#include "tsat_emu_sensed.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_mag_bias_filtered.hpp"

// arguments as tsat_tvlqr_ensemble_mag_bias_filtered (include/tortoise_hip.h) without the handle, with K_lqr as an INPUT before `stats`
extern "C" int emu_tvlqr_ensemble_mag_bias_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                                    const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                                    const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                                                    const double* Qd, const double* Qfd, const double* Rd, const double* x0_sim,
                                                    const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                                                    const double* sat_lo, const double* sat_hi, const double* K_lqr, tsat_tvlqr_stats* stats,
                                                    double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped,
                                                    const double* Rtab, double gm, const tsat_sensor_options* s, const double* sensor,
                                                    const tsat_mag_bias_filter_options* f, double* X_hat, double* filt_final) {
  if (!f) {
    if (X_hat || filt_final) return -1;
    return emu_tvlqr_ensemble_sensed(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots,
                                     plant, sat_lo, sat_hi, K_lqr, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, s, sensor);
  }
  if (!check_tv_options(*o).empty() || o->noise_mode != 1 || o->rate_as_written != 0 || M < 1 || M > 65535) return -1;
  if ((sat_lo == nullptr) != (sat_hi == nullptr)) return -1;
  const int N = o->n_knots, n_tab = o->n_tab;
  if (Rtab ? !check_gravity(Rtab, gm, n_btab * (int64_t)n_tab).empty() : !(gm == 0.0)) return -1;
  if (!check_sensor(s, sensor, T, M).empty() || !check_mag_bias_filter(f).empty()) return -1;
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  std::vector<double> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR((size_t)T * N * XUW), KD((size_t)T * (N - 1) * KDW, 0.0),
      x0n((size_t)T * 7);
  std::vector<int> bidx(T);
  for (int64_t t = 0; t < T; ++t) {
    bidx[t] = btab_idx ? btab_idx[t] : (int)t;
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = X[(size_t)t * N * 7 + i];
  }
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  pack_xu_records<double>(T, N, X, U, XUR.data());
  for (size_t ek = 0; ek < (size_t)T * (N - 1); ++ek)
    for (int j = 0; j < 6; ++j)
      for (int c = 0; c < 3; ++c) KD[ek * KDW + c * 7 + j] = -K_lqr[ek * 18 + j * 3 + c];
  Common cm;
  cm.fill(o, T, n_btab, M, P.data(), Jmat, plant, sat_lo, sat_hi, Rtab, gm, sensor);
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * (size_t)T * M * N * 7);
  if (X_hat) std::memset(X_hat, 0, sizeof(double) * (size_t)T * M * N * 7);
  std::vector<tsat_tvlqr_stats> nom((size_t)T);
  MagBiasFilteredTvArgs<double> fa;
  fa.g.d.e = ens_args<EnsArgs<double>>(*o, T, M, P.data(), BT.data(), bidx.data(), n_knots, XUR.data(), KD.data(), x0_sim,
                                       (const long long*)noise_id0, X_sim, stats, nom.data());
  fa.g.d.PL = cm.PL.data(); fa.g.d.Mp = Mp; fa.g.d.SAT = cm.SAT.data(); fa.g.d.nclip = n_clipped;
  fa.g.GT = Rtab ? cm.GT.data() : nullptr;
  fa.f = mag_bias_filt_args(*f, sens_args(*s, *o, cm.SN.data(), Mp), fa.g.d.e, X_hat, filt_final);
  tsat_emu::for_each_wave((int)T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() { fa.g.GT ? mag_bias_filtered_tv_gg_wave<double>(fa, t, w) : mag_bias_filtered_tv_wave<double>(fa, t, w); });   // no LDS
  });
  if (stats_nominal) std::memcpy(stats_nominal, nom.data(), sizeof(tsat_tvlqr_stats) * (size_t)T);
  ensemble_summary(T, M, stats, summary);
  return 0;
}

// arguments as tsat_pd_ensemble_mag_bias_filtered (include/tortoise_hip.h) without the handle
extern "C" int emu_pd_ensemble_mag_bias_filtered(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                                 const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                                 const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                                                 const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                                                 const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                                                 const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                                 tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                                                 int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* s,
                                                 const double* sensor, const tsat_mag_bias_filter_options* f, double* X_hat,
                                                 double* filt_final) {
  if (!f) {
    if (X_hat || filt_final) return -1;
    return emu_pd_ensemble_sensed(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim,
                                  x0_nom, noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab,
                                  gm, s, sensor);
  }
  if (!check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom, n_knots,
                plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm).empty())
    return -1;
  if (!check_sensor(s, sensor, T, M).empty() || !check_mag_bias_filter(f).empty()) return -1;
  const int N = o->n_knots, n_tab = o->n_tab;
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  const size_t Tn = (size_t)T;
  std::vector<double> P(Tn * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR, x0n(Tn * 7), zero(Tn * 6, 0.0), gain(Tn * PDGW);
  std::vector<int> bidx(Tn);
  for (size_t t = 0; t < Tn; ++t) {
    bidx[t] = btab_idx ? btab_idx[t] : (int)t;
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = x0_nom ? x0_nom[7 * t + i] : (X ? X[t * N * 7 + i] : xf[7 * t + i]);
    for (int c = 0; c < 3; ++c) { gain[PDGW * t + c] = kd[3 * t + c]; gain[PDGW * t + 3 + c] = kp[3 * t + c]; }
  }
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, zero.data(), zero.data(), zero.data(), P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  if (X) {
    std::vector<double> U0;
    if (!feedforward) { U0.assign(Tn * (size_t)(N - 1) * 3, 0.0); U = U0.data(); }
    XUR.resize(Tn * N * XUW);
    pack_xu_records<double>(T, N, X, U, XUR.data());
  }
  Common cm;
  cm.fill(o, T, n_btab, M, P.data(), Jmat, plant, sat_lo, sat_hi, Rtab, gm, sensor);
  if (X_sim) std::memset(X_sim, 0, sizeof(double) * Tn * M * N * 7);
  if (X_hat) std::memset(X_hat, 0, sizeof(double) * Tn * M * N * 7);
  std::vector<tsat_tvlqr_stats> nom(Tn);
  MagBiasFilteredPdArgs<double> fa;
  PdArgs<double>& pa = fa.p;
  pa.d.e = ens_args<EnsArgs<double>>(*o, T, M, P.data(), BT.data(), bidx.data(), n_knots, X ? XUR.data() : nullptr, nullptr, x0_sim,
                                     (const long long*)noise_id0, X_sim, stats, nom.data());
  pa.d.PL = cm.PL.data(); pa.d.Mp = Mp; pa.d.SAT = cm.SAT.data(); pa.d.nclip = n_clipped;
  pa.GT = Rtab ? cm.GT.data() : nullptr; pa.GAIN = gain.data(); pa.X0N = x0n.data(); pa.feedforward = feedforward; pa.limit_mode = limit_mode;
  fa.f = mag_bias_filt_args(*f, sens_args(*s, *o, cm.SN.data(), Mp), pa.d.e, X_hat, filt_final);
  tsat_emu::for_each_wave((int)T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() { pa.GT ? mag_bias_filtered_pd_gg_wave<double>(fa, t, w) : mag_bias_filtered_pd_wave<double>(fa, t, w); });   // no LDS
  });
  if (stats_nominal) std::memcpy(stats_nominal, nom.data(), sizeof(tsat_tvlqr_stats) * Tn);
  ensemble_summary(T, M, stats, summary);
  return 0;
}

// check_mag_bias_filter alone: 0 and "" or -1 and the text tsat_ensemble_last_error would hold
extern "C" int emu_mag_bias_filter_check(const tsat_mag_bias_filter_options* f, char* text, int32_t cap) {
  const std::string why = check_mag_bias_filter(f);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
