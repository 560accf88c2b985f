// tsat_emu_mpc_dispersed.cpp — the receding-horizon step on a dispersed plant (tortoisesat.jl_amd/csrc/tsat_mpc_dispersed.hpp) under the
// CPU lane emulator (TEST INFRASTRUCTURE). The loop of tsat_mpc_run_dispersed on the emulated batch of tsat_emu_mpc.hpp: per control
// step the emulated solve of every trajectory, then mpc_dispersed_trajectory; the plant records are made by the product's own pack
// function, one call per thread of its grid. The arguments are validated by the library's own host function (check_mpc_dispersed,
// tsat_host_pack.hpp), which emu_mpc_dispersed_check also exposes on its own: what the entry point rejects can be tested without a GPU.
#include "tsat_emu_mpc.hpp"

// arguments: the batch as emu_mpc_batch, then those of tsat_mpc_run_dispersed (include/tortoise_hip.h), the last plan, n_knots
extern "C" int emu_mpc_dispersed_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab, const double* x0,
                                       const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                       const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                       const double* Rd, const double* ulo, const double* uhi, const double* U0, int32_t n_steps,
                                       int64_t step0, const double* plant, const double* sat_lo, const double* sat_hi,
                                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last,
                                       tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last, double* U_last,
                                       const int32_t* n_knots) {
  const MpcIn in = {o, po, T, n_btab, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0, n_steps, step0, 0, 0,
                    plant, sat_lo, sat_hi, noise_id, X_hist, U_hist, stats_last, stats, n_clipped, X_last, U_last, n_knots};
  if (!mpc_in_valid(in)) return -1;
  MpcDispArgs<double> md = {};
  MpcBatch b(in, md);
  std::vector<double> PL((size_t)T * PLW);
  md.d.PL = PL.data();
  for (int64_t t = 0; t < T; ++t) mpc_dispersed_pack<double>(plant, b.P.data(), o->u_scale, PL.data(), b.rec.data(), T, t);
  for (int s = 0; s < n_steps; ++s) {
    b.solve();
    md.m.step = s;
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_dispersed_trajectory<double>(md, t); });
  }
  b.export_last();
  return 0;
}

// the argument checks of tsat_mpc_run_dispersed alone: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_dispersed_check(const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0, const double* plant,
                                       const double* sat_lo, const double* sat_hi, int64_t T, char* text, int32_t cap) {
  const std::string why = check_mpc_dispersed(*po, n_steps, step0, plant, sat_lo, sat_hi, T);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
