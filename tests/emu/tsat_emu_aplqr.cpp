// tsat_emu_aplqr.cpp — the asymptotic periodic LQR (tortoisesat.jl_amd/csrc/tsat_aplqr.hpp) under the CPU lane emulator (TEST
// INFRASTRUCTURE): care6 alone (emu_care6, a test-only export), the synthesis (emu_aplqr_gains: the library's own check and pack
// functions, then aplqr_gains_wave per slew), the roll-out (emu_aplqr_ensemble: the staging of tsat_emu_rollout.hpp's PD call with
// the gain records of pack_aplqr_law, then aplqr_wave / aplqr_gg_wave per wavefront) and the two validation functions alone.
#include "tsat_emu_rollout.hpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_aplqr.hpp"

// A, G, Q, P 6 x 6 row-major; info one tsat_aplqr_info
extern "C" int emu_care6(const double* A, const double* G, const double* Q, double res_tol, double* P, void* info) {
  tsat_emu::run_wave((size_t)AQL_REALS * 8, [&]() {
    double* lds = aplqr_lds();
    const CareInfo ci = care6(A, G, Q, res_tol, lds, lds + AQL_P);
    const int lane = TSAT_LANE();
    if (lane < 36) P[lane] = lds[AQL_P + lane];
    if (lane == 0) *static_cast<tsat_aplqr_info*>(info) = tsat_aplqr_info{ci.status, ci.iterations, ci.residual, ci.pivot_min};
  });
  return 0;
}

// arguments as tsat_aplqr_gains (include/tortoise_hip.h) without the handle
extern "C" int emu_aplqr_gains(int64_t T, int64_t n_btab, int32_t n_tab, const double* xf, const double* Btab, const int32_t* btab_idx,
                               const int32_t* avg_lo, const int32_t* avg_hi, const double* Jmat, const double* qd, const double* rd,
                               const double* alpha, double res_tol, double* Kg, double* P_ss, double* Gamma, void* info) {
  if (!check_aplqr_gains(T, n_btab, n_tab, xf, Btab, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha, res_tol, Kg, info).empty()) return -1;
  const std::vector<double> gp = pack_aplqr_gains(T, n_tab, xf, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha);
  std::vector<double> P((size_t)T * 36), Gm((size_t)T * 9);
  const AplqrGainArgs a{gp.data(), Btab, n_tab, res_tol, Kg, P.data(), Gm.data(), info};
  tsat_emu::for_each_wave((int)T, [&](int t) { tsat_emu::run_wave((size_t)AQL_REALS * 8, [&]() { aplqr_gains_wave(a, t); }); });
  if (P_ss) std::memcpy(P_ss, P.data(), sizeof(double) * P.size());
  if (Gamma) std::memcpy(Gamma, Gm.data(), sizeof(double) * Gm.size());
  return 0;
}

// 0 and "" or -1 and the text tsat_ensemble_last_error would hold
extern "C" int emu_aplqr_gains_check(int64_t T, int64_t n_btab, int32_t n_tab, const double* xf, const double* Btab, const int32_t* btab_idx,
                                     const int32_t* avg_lo, const int32_t* avg_hi, const double* Jmat, const double* qd, const double* rd,
                                     const double* alpha, double res_tol, const double* Kg, const void* info, char* text, int32_t cap) {
  return check_result(check_aplqr_gains(T, n_btab, n_tab, xf, Btab, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha, res_tol, Kg, info), text, cap);
}

// arguments as tsat_aplqr_ensemble without the handle
extern "C" int emu_aplqr_ensemble(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                                  const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                                  const double* dt, const double* Jmat, const double* Kg, const double* rd, int32_t feedforward,
                                  int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                                  const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                  tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
                                  int32_t* n_clipped, const double* Rtab, double gm) {
  if (!check_aplqr(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Kg, rd, feedforward, limit_mode, x0_sim, x0_nom, n_knots,
                   plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm)
           .empty())
    return -1;
  // the PD call's staging with zero PD gains, then the law's own gain records in their place
  const std::vector<double> zero((size_t)T * 3, 0.0);
  EmuCall c{o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = EmuPd{zero.data(), zero.data(), feedforward, limit_mode, x0_nom};
  c.disp = EmuDispersion{plant, sat_lo, sat_hi, n_clipped};
  c.grav = EmuGravity{Rtab, gm};
  EmuBuffers b;
  PdArgs<double> pa = stage_pd(c, b);
  b.gain = pack_aplqr_law(T, Kg, rd);
  pa.GAIN = b.gain.data();
  return roll(c, b, [&](int t, int w) { pa.GT ? aplqr_gg_wave<double>(pa, t, w) : aplqr_wave<double>(pa, t, w); });
}

// arguments as emu_aplqr_ensemble without noise_id0, X_sim and n_clipped (which nothing is asked of), then the text buffer
extern "C" int emu_aplqr_check(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                               const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                               const double* dt, const double* Jmat, const double* Kg, const double* rd, int32_t feedforward,
                               int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int32_t* n_knots, const double* plant,
                               const double* sat_lo, const double* sat_hi, const void* stats, const double* summary,
                               const void* stats_nominal, const double* Rtab, double gm, char* text, int32_t cap) {
  return check_result(check_aplqr(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Kg, rd, feedforward, limit_mode, x0_sim, x0_nom,
                                  n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm),
                      text, cap);
}
