// tsat_emu_rollout.hpp — the ensemble roll-outs under the CPU lane emulator (TEST INFRASTRUCTURE): what the drivers of the
// ensemble entry points (tsat_emu_ensemble.cpp, _gg, _pd, _sensed and the four filter files) share, as run_call of
// tortoisesat.jl_amd/csrc/tsat_kernels_ensemble.hip is what the entry points share. Takes run_wave / for_each_wave and the packing
// code from tsat_emu.cpp as they are. EmuCall describes a call as `Call` does there; tv_call_valid / pd_call_valid are its checks,
// made of the library's own host functions; stage_tv / stage_pd fill the emulated device buffers (EmuBuffers) with the product's own
// pack functions, one call per thread of their grids, zero the outputs the entry points zero and return the launch block of the law;
// roll runs a wave function with lane = realisation over the grid of the roll-out, copies the nominal statistics out and forms the
// summary with the library's own host function. sensed_tv / sensed_pd are the drivers of the two sensed calls, filtered_tv /
// filtered_pd those of the calls behind a filter, one template for the four filter families (a `Family`: tsat_emu_filtered.cpp).
#pragma once
#include <cmath>
#include <optional>
#include "tsat_emu.cpp"
#include "../../tortoisesat.jl_amd/csrc/tsat_sensed.hpp"

// what only the TVLQR calls carry: the weights, and K_lqr 3 x 6 x (N-1) x T as an INPUT (from the emulated tracking kernel or the oracle)
struct EmuTv {
  const double *Qd, *Qfd, *Rd, *K_lqr;
};

// ... and only the PD ones
struct EmuPd {
  const double *kd, *kp;
  int32_t feedforward, limit_mode;
  const double* x0_nom;
};

// what tsat_tvlqr_ensemble_dispersed adds to tsat_tvlqr_ensemble, _gg to that, the sensed calls to either law, the filtered to those
struct EmuDispersion {
  const double *plant, *sat_lo, *sat_hi;
  int32_t* n_clipped;
};
struct EmuGravity {
  const double* Rtab;
  double gm;
};
struct EmuSensing {
  const tsat_sensor_options* s;
  const double* sensor;
};
struct EmuFiltering {
  double *X_hat, *filt_final;
};

// One call of any entry point: the arrays every one of them takes, the part of its law (exactly one of `tv` / `pd`), and what the
// call adds to tsat_tvlqr_ensemble (empty: not this entry point). The PD calls always carry `disp` and `grav`.
struct EmuCall {
  const tsat_tvlqr_options* o;
  int64_t T, n_btab;
  int32_t M;
  const double *X, *U, *xf, *Btab;
  const int32_t* btab_idx;
  const double *tau0, *dtau, *dt, *Jmat, *x0_sim;
  const int64_t* noise_id0;
  const int32_t* n_knots;
  tsat_tvlqr_stats* stats;
  double* summary;
  tsat_tvlqr_stats* stats_nominal;
  double* X_sim;
  std::optional<EmuTv> tv;
  std::optional<EmuPd> pd;
  std::optional<EmuDispersion> disp;
  std::optional<EmuGravity> grav;
  std::optional<EmuSensing> sens;
  std::optional<EmuFiltering> filt;
};

// what a TVLQR entry point rejects of the arguments the emulator is given (check_tvlqr of the library, without the null and range
// checks of the arrays): only the sensed calls take the model's plant for a null plant and the kernels without gravity rows for a
// null Rtab with gm == 0
static bool tv_call_valid(const EmuCall& c) {
  const tsat_tvlqr_options& o = *c.o;
  if (!check_tv_options(o).empty() || o.noise_mode != 1 || o.rate_as_written != 0 || c.M < 1 || c.M > 65535) return false;
  if (c.disp && ((c.disp->sat_lo == nullptr) != (c.disp->sat_hi == nullptr) || (!c.sens && !c.disp->plant))) return false;
  if (c.grav && c.sens && !c.grav->Rtab) {
    if (!(c.grav->gm == 0.0)) return false;
  } else if (c.grav && !check_gravity(c.grav->Rtab, c.grav->gm, c.n_btab * (int64_t)o.n_tab).empty()) {
    return false;
  }
  return !c.sens || check_sensor(c.sens->s, c.sens->sensor, c.T, c.M).empty();
}

// ... of a PD one: check_pd is the authority
static bool pd_call_valid(const EmuCall& c) {
  return check_pd(c.o, c.T, c.n_btab, c.M, c.X, c.U, c.xf, c.Btab, c.btab_idx, c.tau0, c.dtau, c.dt, c.Jmat, c.pd->kd, c.pd->kp,
                  c.pd->feedforward, c.pd->limit_mode, c.x0_sim, c.pd->x0_nom, c.n_knots, c.disp->plant, c.disp->sat_lo, c.disp->sat_hi,
                  c.stats, c.summary, c.stats_nominal, c.grav->Rtab, c.grav->gm)
             .empty() &&
         (!c.sens || check_sensor(c.sens->s, c.sens->sensor, c.T, c.M).empty());
}

// the emulated device buffers of a valid call
struct EmuBuffers {
  int nw, Mp;            // wavefronts of a slew, 64 * nw
  std::vector<double> P, BT, XUR, KD, gain, x0n, SAT, PL, GT, SN, model;
  std::vector<int> bidx;
  std::vector<tsat_tvlqr_stats> nom;
};

// what both laws stage once P is packed: the field table, the limits, the plants (the model's when null), the gravity rows (none
// when Rtab is null), the sensor records, the zeroed outputs; returns the block of the dispersed call (its PL and SAT null without
// plants) around the reference records XUR and the gains KD (either may be null)
static DispArgs<double> stage_rest(const EmuCall& c, EmuBuffers& b, const double* XUR, const double* KD) {
  const int64_t T = c.T;
  const int M = c.M, N = c.o->n_knots, n_tab = c.o->n_tab;
  const size_t Tn = (size_t)T;
  b.nw = ensemble_waves(M);
  const int Mp = b.Mp = b.nw * WAVE;
  b.BT.resize((size_t)c.n_btab * n_tab * 4);
  pack_btab<double>(c.n_btab, n_tab, c.Btab, b.BT.data());
  b.bidx.resize(Tn);
  for (size_t t = 0; t < Tn; ++t) b.bidx[t] = c.btab_idx ? c.btab_idx[t] : (int)t;
  if (c.disp) {
    b.SAT = pack_limits(c.disp->sat_lo, c.disp->sat_hi, T);
    const double* plant = c.disp->plant;
    if (!plant) {
      b.model = model_plants(c.Jmat, Tn, M);
      plant = b.model.data();
    }
    b.PL.assign(Tn * PLW * Mp, 0.0);
    for (int64_t e = 0; e < T * (int64_t)(M + 1); ++e) dispersed_pack<double>(plant, b.P.data(), c.o->u_scale, b.PL.data(), T, M, Mp, e);
  }
  if (c.grav && c.grav->Rtab) {
    const int64_t rows = c.n_btab * (int64_t)n_tab;
    b.GT.resize((size_t)rows * 4);
    for (int64_t e = 0; e < rows; ++e) gg_pack_row<double>(c.grav->Rtab, c.grav->gm, b.GT.data(), rows, e);
  }
  if (c.sens) {
    b.SN.assign(Tn * SNW * Mp, -1.0);                          // the pack has to write every slot
    for (int64_t e = 0; e < T * (int64_t)Mp; ++e) sensed_pack<double>(c.sens->sensor, b.SN.data(), T, M, Mp, e);
  }
  if (c.X_sim) std::memset(c.X_sim, 0, sizeof(double) * Tn * M * N * 7);
  if (c.filt && c.filt->X_hat) std::memset(c.filt->X_hat, 0, sizeof(double) * Tn * M * N * 7);
  b.nom.resize(Tn);
  DispArgs<double> d;
  d.e = ens_args<EnsArgs<double>>(*c.o, T, M, b.P.data(), b.BT.data(), b.bidx.data(), c.n_knots, XUR, KD, c.x0_sim,
                                  (const long long*)c.noise_id0, c.X_sim, c.stats, b.nom.data());
  d.PL = c.disp ? b.PL.data() : nullptr; d.Mp = Mp; d.SAT = c.disp ? b.SAT.data() : nullptr; d.nclip = c.disp ? c.disp->n_clipped : nullptr;
  return d;
}

// a TVLQR call: the block of tsat_tvlqr_ensemble_gg (g.d that of _dispersed, g.d.e that of tsat_tvlqr_ensemble; g.GT null without
// an orbit table)
static GgEnsArgs<double> stage_tv(const EmuCall& c, EmuBuffers& b) {
  const int64_t T = c.T;
  const int N = c.o->n_knots;
  b.P.resize((size_t)T * PSTRIDE);
  b.x0n.resize((size_t)T * 7);
  for (int64_t t = 0; t < T; ++t)
    for (int i = 0; i < 7; ++i) b.x0n[7 * t + i] = c.X[(size_t)t * N * 7 + i];
  pack_tv_params<double>(T, b.x0n.data(), c.xf, c.tau0, c.dtau, c.dt, c.Jmat, c.tv->Qd, c.tv->Qfd, c.tv->Rd, b.P.data());
  b.XUR.resize((size_t)T * N * XUW);
  pack_xu_records<double>(T, N, c.X, c.U, b.XUR.data());
  b.KD.assign((size_t)T * (N - 1) * KDW, 0.0);
  for (size_t ek = 0; ek < (size_t)T * (N - 1); ++ek)          // the inverse of unpack_tv: solver sign, rows of 7
    for (int j = 0; j < 6; ++j)
      for (int k = 0; k < 3; ++k) b.KD[ek * KDW + k * 7 + j] = -c.tv->K_lqr[ek * 18 + j * 3 + k];
  GgEnsArgs<double> g;
  g.d = stage_rest(c, b, b.XUR.data(), b.KD.data());
  g.GT = (c.grav && c.grav->Rtab) ? b.GT.data() : nullptr;
  return g;
}

// a PD call: the block of tsat_pd_ensemble. Without X the law regulates to xf and there are no reference records; without
// feed-forward U is not read and the records carry zeros
static PdArgs<double> stage_pd(const EmuCall& c, EmuBuffers& b) {
  const EmuPd& pd = *c.pd;
  const int N = c.o->n_knots;
  const size_t Tn = (size_t)c.T;
  const std::vector<double> zero(Tn * 6, 0.0);
  b.P.resize(Tn * PSTRIDE);
  b.x0n.resize(Tn * 7);
  b.gain.resize(Tn * PDGW);
  for (size_t t = 0; t < Tn; ++t) {
    for (int i = 0; i < 7; ++i) b.x0n[7 * t + i] = pd.x0_nom ? pd.x0_nom[7 * t + i] : (c.X ? c.X[t * N * 7 + i] : c.xf[7 * t + i]);
    for (int k = 0; k < 3; ++k) {
      b.gain[PDGW * t + k] = pd.kd[3 * t + k];
      b.gain[PDGW * t + 3 + k] = pd.kp[3 * t + k];
    }
  }
  pack_tv_params<double>(c.T, b.x0n.data(), c.xf, c.tau0, c.dtau, c.dt, c.Jmat, zero.data(), zero.data(), zero.data(), b.P.data());
  if (c.X) {
    const std::vector<double> U0(pd.feedforward ? 0 : Tn * (size_t)(N - 1) * 3, 0.0);
    b.XUR.resize(Tn * N * XUW);
    pack_xu_records<double>(c.T, N, c.X, pd.feedforward ? c.U : U0.data(), b.XUR.data());
  }
  PdArgs<double> pa;
  pa.d = stage_rest(c, b, c.X ? b.XUR.data() : nullptr, nullptr);
  pa.GT = c.grav->Rtab ? b.GT.data() : nullptr; pa.GAIN = b.gain.data(); pa.X0N = b.x0n.data();
  pa.feedforward = pd.feedforward; pa.limit_mode = pd.limit_mode;
  return pa;
}

// the roll-out of a staged call: wave(t, w) is wavefront w of slew t (the kernels use no LDS)
template <typename Wave>
static int roll(const EmuCall& c, const EmuBuffers& b, Wave wave) {
  const int nw = b.nw;
  tsat_emu::for_each_wave((int)c.T * nw, [&](int i) {
    const int t = i / nw, w = i - t * nw;
    tsat_emu::run_wave(64, [&]() { wave(t, w); });
  });
  if (c.stats_nominal) std::memcpy(c.stats_nominal, b.nom.data(), sizeof(tsat_tvlqr_stats) * (size_t)c.T);
  ensemble_summary(c.T, c.M, c.stats, c.summary);
  return 0;
}

// tsat_tvlqr_ensemble_sensed and tsat_pd_ensemble_sensed: the sensed waves, those without gravity rows for a null Rtab
static int sensed_tv(const EmuCall& c) {
  if (!tv_call_valid(c)) return -1;
  EmuBuffers b;
  SensedTvArgs<double> a;
  a.g = stage_tv(c, b);
  a.s = sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp);
  return roll(c, b, [&](int t, int w) { a.g.GT ? sensed_tv_gg_wave<double>(a, t, w) : sensed_tv_wave<double>(a, t, w); });
}

static int sensed_pd(const EmuCall& c) {
  if (!pd_call_valid(c)) return -1;
  EmuBuffers b;
  SensedPdArgs<double> a;
  a.p = stage_pd(c, b);
  a.s = sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp);
  return roll(c, b, [&](int t, int w) { a.p.GT ? sensed_pd_gg_wave<double>(a, t, w) : sensed_pd_wave<double>(a, t, w); });
}

// The calls behind a filter: `c` is the sensed call, f the family's options. f == NULL is the sensed call, which has no X_hat and no
// filt_final to fill. A Family names the filter: Options, TvArgs / PdArgs (the sensed blocks with the filter's in `f`), check(f) ("" or
// the reason), args(f, sensor block, EnsArgs, X_hat, filt_final) (the filter's launch block) and its four waves tv, tv_gg, pd, pd_gg.
template <typename Family>
static int filtered_tv(EmuCall c, const typename Family::Options* f, double* X_hat, double* filt_final) {
  if (!f) return (X_hat || filt_final) ? -1 : sensed_tv(c);
  c.filt = EmuFiltering{X_hat, filt_final};
  if (!tv_call_valid(c) || !Family::check(f).empty()) return -1;
  EmuBuffers b;
  typename Family::TvArgs a;
  a.g = stage_tv(c, b);
  a.f = Family::args(*f, sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp), a.g.d.e, X_hat, filt_final);
  return roll(c, b, [&](int t, int w) { a.g.GT ? Family::tv_gg(a, t, w) : Family::tv(a, t, w); });
}

template <typename Family>
static int filtered_pd(EmuCall c, const typename Family::Options* f, double* X_hat, double* filt_final) {
  if (!f) return (X_hat || filt_final) ? -1 : sensed_pd(c);
  c.filt = EmuFiltering{X_hat, filt_final};
  if (!pd_call_valid(c) || !Family::check(f).empty()) return -1;
  EmuBuffers b;
  typename Family::PdArgs a;
  a.p = stage_pd(c, b);
  a.f = Family::args(*f, sens_args(*c.sens->s, *c.o, b.SN.data(), b.Mp), a.p.d.e, X_hat, filt_final);
  return roll(c, b, [&](int t, int w) { a.p.GT ? Family::pd_gg(a, t, w) : Family::pd(a, t, w); });
}

// a check function's result as the *_check symbols return it: 0 and "" or -1 and the text tsat_ensemble_last_error would hold
static int check_result(const std::string& why, char* text, int32_t cap) {
  if (cap > 0) { std::strncpy(text, why.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return why.empty() ? 0 : -1;
}
