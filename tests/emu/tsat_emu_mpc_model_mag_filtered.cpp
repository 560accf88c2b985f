// tsat_emu_mpc_model_mag_filtered.cpp — the held re-planning loop behind the magnetometer-updated nine-state filter
// (tortoisesat.jl_amd/csrc/tsat_mpc_model_mag_filtered.hpp) under the CPU lane emulator (TEST INFRASTRUCTURE): the loop of
// tsat_emu_mpc_model_filtered.cpp with the product's own model-mag-filtered pack and hold in place of the model-filtered ones and the
// field's memory HB beside the records, as tsat_mpc_run_held_model_mag_filtered has it. f == NULL is the emulated sensed loop, as the
// entry point dispatches. The filter arguments are validated by the library's own check_mpc_model_mag_filtered, which
// emu_mpc_model_mag_filtered_check exposes alone.
#include "tsat_emu_mpc.hpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_mpc_model_mag_filtered.hpp"

// arguments: those of emu_mpc_held_model_filtered_batch, f of this filter's type
extern "C" int emu_mpc_held_model_mag_filtered_batch(const tsat_options* o, const tsat_tvlqr_options* po, int64_t T, int64_t n_btab,
                                                     const double* x0, const double* xf, const double* Btab, const int32_t* btab_idx,
                                                     const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                                                     const double* Qd, const double* Qfd, const double* Rd, const double* ulo,
                                                     const double* uhi, const double* U0, int32_t n_steps, int64_t step0,
                                                     int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                                                     const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist,
                                                     tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped, double* X_last,
                                                     double* U_last, const int32_t* n_knots, const double* Rtab, double gm,
                                                     const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                                                     const tsat_model_mag_filter_options* f, const double* filt_init, double* filt_state,
                                                     double* filt_final, double* x0_after) {
  if (!s) return -1;
  const MpcIn in = {o, po, T, n_btab, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0, n_steps, step0, replan_every, feedback,
                    plant, sat_lo, sat_hi, noise_id, X_hist, U_hist, stats_last, stats, n_clipped, X_last, U_last, n_knots};
  if (!check_mpc_model_mag_filtered(f, filt_init, filt_state, filt_final, T).empty()) return -1;
  if (!f) return emu_mpc_held(in, Rtab, gm, s, sensor, Y_hist, x0_after);
  const int64_t rows = n_btab * (int64_t)o->n_tab;
  if (!mpc_in_valid(in)) return -1;
  if (Rtab && !check_gravity(Rtab, gm, rows).empty()) return -1;
  if (!check_mpc_sensed(s, sensor, T, Rtab, gm).empty()) return -1;
  int min_nk = o->n_knots;
  for (int64_t t = 0; n_knots && t < T; ++t) min_nk = n_knots[t] < min_nk ? n_knots[t] : min_nk;
  if (!check_mpc_held(replan_every, feedback, min_nk).empty()) return -1;
  MpcModelMagFilteredArgs<double> mg = {};
  MpcSensedArgs<double>& ms = mg.ms;
  ModelFiltArgs<double>& mf = mg.f.m;
  MpcHeldArgs<double>& mh = ms.h;
  MpcArgs<double>& m = mh.s.m;
  MpcBatch b(in, mh.s);
  std::vector<double> PL((size_t)T * HELD_W), GT, SN((size_t)T * SNW, -1.0), XT((size_t)T * MSX_W, -1.0), Yw, FL((size_t)T * MFLW, -1.0),
      HB((size_t)T * 3, -1.0);
  mh.s.d.PL = PL.data(); mh.KD = b.KD.data(); mh.feedback = feedback;
  for (int64_t t = 0; t < T; ++t) mpc_held_pack<double>(plant, b.P.data(), b.SAT.data(), o->u_scale, PL.data(), b.rec.data(), T, t);
  if (Rtab) {
    GT.resize((size_t)rows * 4);
    for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(Rtab, gm, GT.data(), rows, e);
  }
  if (!Y_hist) { Yw.resize((size_t)T * n_steps * 7); Y_hist = Yw.data(); }
  ms.GT = Rtab ? GT.data() : nullptr; ms.XT = XT.data(); ms.HY = Y_hist;
  ms.s.SN = SN.data(); ms.s.Mp = (int)T; ms.s.sgy = s->sigma_gyro; ms.s.sat = s->sigma_att; ms.s.smg = s->sigma_mag;
  ms.s.latency = s->latency; ms.s.k0 = mh.s.d.e.k0; ms.s.k1 = mh.s.d.e.k1;
  mg.FL = FL.data(); mg.HB = HB.data(); mg.f.sm = f->sigma_m;
  mf.s = ms.s; mf.P = b.P.data(); mf.M = 1; mf.N = b.N; mf.n_tab = o->n_tab; mf.us = o->u_scale;
  mf.sv = f->sigma_v; mf.sw = f->sigma_w; mf.su = f->sigma_u; mf.sa = 0.0; mf.sg = f->sigma_g;
  mf.p0a = f->p0_att; mf.p0b = f->p0_bias;
  if (filt_init) model_filt_records_pack(filt_init, FL.data(), T);
  for (int64_t t = 0; t < T; ++t) mpc_model_mag_filtered_pack<double>(mg, sensor, filt_init != nullptr, t);
  const int es = o->error_state ? 1 : 0;
  for (int sb = 0; sb < n_steps; sb += replan_every) {
    b.solve();
    m.step = sb;
    mh.r = replan_every < n_steps - sb ? replan_every : n_steps - sb;
    for (int t = 0; t < (int)T; ++t) {    // lane = trajectory: no lane of the hold talks to another
      if (ms.GT) es ? mpc_model_mag_filtered_gg_traj<double, 1>(mg, t) : mpc_model_mag_filtered_gg_traj<double, 0>(mg, t);
      else es ? mpc_model_mag_filtered_traj<double, 1>(mg, t) : mpc_model_mag_filtered_traj<double, 0>(mg, t);
    }
    for (int t = 0; t < (int)T; ++t)
      tsat_emu::run_wave((size_t)LDS_REALS * 8, [&]() { mpc_held_shift<double>(m, mh.r, t); });
  }
  b.export_last();
  model_filt_records_unpack(FL.data(), T, filt_state, filt_final);
  if (x0_after)
    for (int64_t t = 0; t < T; ++t)
      for (int i = 0; i < 7; ++i) x0_after[7 * t + i] = b.P[(size_t)t * PSTRIDE + P_X0 + i];
  return 0;
}

// the argument checks tsat_mpc_run_held_model_mag_filtered adds: 0 and "" or -1 and the text tsat_last_error would hold
extern "C" int emu_mpc_model_mag_filtered_check(const tsat_model_mag_filter_options* f, const double* filt_init, double* filt_state,
                                                double* filt_final, int64_t T, char* text, int32_t cap) {
  const std::string why = check_mpc_model_mag_filtered(f, filt_init, filt_state, filt_final, T);
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
