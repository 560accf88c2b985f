// tsat_kernels_ensemble.hip — the host side of the twenty-two ensemble entry points (include/tortoise_hip.h): tsat_tvlqr_ensemble and its
// _dispersed, _gg, _sensed, _filtered, _model_filtered, _mag_filtered, _mag_bias_filtered, _model_mag_filtered,
// _model_mag_sun_filtered, and tsat_pd_ensemble with its _sensed, _filtered, _model_filtered, _mag_filtered, _mag_bias_filtered,
// _model_mag_filtered, _model_mag_sun_filtered, and tsat_aplqr_ensemble (a PD
// call with another law) with its synthesis tsat_aplqr_gains (run_aplqr_gains: no roll-out, a call of its own). A
// translation unit of its own, built on the public ABI: `struct tsat_handle` is private to tsat_kernels.hip, so a call keeps its own
// buffers and stream. An entry point only describes its call (`Call`: the common arrays, the part of its law, and what it adds —
// Dispersion, Gravity, Sensing, Filtering); run_call goes through the stages once, all of it synchronous:
//   1. checks, in each entry point's own order (check_tvlqr / check_pd, then check_sensor, then the filter's);
//   2. the handle: a one-slew, two-knot call of tsat_tvlqr_batch validates it and the options block with the library's own checks
//      and leaves its GPU current on the calling thread (TVLQR); hipSetDevice on its GPU (PD);
//   3. allocation and upload: X, U and the tables go up AS THEY ARE, the plan only when there is one (a PD call with X == NULL
//      regulates to xf and uploads nothing of size N);
//   4. packs on the device: knot records, padded table rows, per-lane plant records, gravity rows (a grow-only workspace of the
//      handle), per-lane sensor records; X_hat zero-filled;
//   5. the gains kernel (TVLQR only): one wavefront per slew runs the gain half of the tracking kernel, so K is what
//      tsat_tvlqr_batch returns, and it never leaves the device unless asked for;
//   6. the roll-out: grid (T, ceil((M + 1) / 64)), one dispatch per law (launch_tvlqr / launch_pd) to the unit that holds the kernel;
//      the extra realisation is the noise-free plant (stats_nominal);
//   7. statistics (and K / X_sim / n_clipped / X_hat / filt_final when asked for) come down; `summary` is formed on the host.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "tsat_host_pack.hpp"
#include "tsat_ensemble.hpp"
#include "tsat_dispersed.hpp"
#include "tsat_gg.hpp"
#include "tsat_pd.hpp"
#include "tsat_sensed.hpp"
#include "tsat_filtered.hpp"
#include "tsat_model_filtered.hpp"
#include "tsat_mag_filtered.hpp"
#include "tsat_mag_bias_filtered.hpp"
#include "tsat_model_mag_filtered.hpp"
#include "tsat_model_mag_sun_filtered.hpp"
#include "tsat_ensemble_launch.hpp"
#include "tsat_aplqr.hpp"

using namespace tsat;

// the handle's workspace for the packed gravity rows, counted by tsat_workspace_bytes, and its GPU (tsat_kernels.hip)
double* tsat_ws_gravity(tsat_handle* h, size_t bytes);
double* tsat_ws_sun(tsat_handle* h, size_t bytes);             // ... and for the packed sun rows
int tsat_handle_device(const tsat_handle* h);

template <typename real, int DIAGJ>
__global__ __launch_bounds__(64) void tsat_ensemble_kernel(EnsArgs<real> a) {
  ensemble_wave<real, DIAGJ>(a, (int)blockIdx.x, (int)blockIdx.y);
}

template <typename real>
__global__ __launch_bounds__(64) void tsat_dispersed_kernel(DispArgs<real> d) {
  dispersed_wave<real>(d, (int)blockIdx.x, (int)blockIdx.y);
}
// plants 21 x M x T -> packed per-lane records [T][PLW][Mp], slot M = the model's plant; one thread per realisation
__global__ __launch_bounds__(256) void tsat_dispersed_pack_kernel(const double* plant, const double* P, double us, double* PL, int64_t T,
                                                                  int M, int Mp) {
  dispersed_pack<double>(plant, P, us, PL, T, M, Mp, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

template <typename real, int DIAGJ>
__global__ __launch_bounds__(64) void tsat_ensemble_gains_kernel(const real* P, const real* BT, const int* bidx, const int* nk,
                                                                 const real* XUR, real* KD, int N, int n_tab, real u_scale,
                                                                 int lin_sq) {
  ensemble_gains<real, DIAGJ>(P, BT, bidx, nk, XUR, KD, N, n_tab, u_scale, lin_sq, (int)blockIdx.x);
}

// X (T,N,7) + U (T,N-1,3) -> knot records [T][N][10] (pack_xu_records, on the device)
__global__ __launch_bounds__(256) void tsat_ensemble_pack_xu_kernel(int64_t n_rec, int N, const double* X, const double* U, double* XU) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_rec) return;
  const int64_t t = e / N;
  const int k = (int)(e - t * N);
  double* r = XU + (size_t)e * XUW;
  for (int i = 0; i < 7; ++i) r[i] = X[(size_t)e * 7 + i];
  for (int c = 0; c < 3; ++c) r[7 + c] = (k < N - 1) ? U[((size_t)t * (N - 1) + k) * 3 + c] : 0.0;
}
// field rows [rows][3] -> [rows][4] (pack_btab, on the device)
__global__ __launch_bounds__(256) void tsat_ensemble_pack_bt_kernel(int64_t rows, const double* B, double* BT) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows) return;
  BT[4 * e + 0] = B[3 * e + 0]; BT[4 * e + 1] = B[3 * e + 1]; BT[4 * e + 2] = B[3 * e + 2]; BT[4 * e + 3] = 0.0;
}
// gains in the solver's sign [T][N-1][24] -> K_lqr 3 x 6 x (N-1) x T (unpack_tv, on the device)
__global__ __launch_bounds__(256) void tsat_ensemble_export_k_kernel(int64_t n, const double* KD, double* K) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  for (int j = 0; j < 6; ++j)
    for (int c = 0; c < 3; ++c) K[(size_t)e * 18 + j * 3 + c] = -KD[(size_t)e * KDW + c * 7 + j];
}

namespace {

thread_local std::string g_err;

int efail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// the call's device buffers, stream and events: released on every way out
struct EnsScope {
  std::vector<void*> bufs;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};
  ~EnsScope() {
    for (void* p : bufs) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <typename Tp>
  bool alloc(Tp** p, size_t n) {
    void* q = nullptr;
    const size_t b = n * sizeof(Tp);
    if (hipMalloc(&q, b ? b : 16) != hipSuccess) return false;
    bufs.push_back(q);
    *p = reinterpret_cast<Tp*>(q);
    return true;
  }
};

// what tsat_tvlqr_ensemble_dispersed adds to the call
struct Dispersion {
  const double *plant, *sat_lo, *sat_hi;
  int32_t* n_clipped;
};

// ... and tsat_tvlqr_ensemble_gg to the dispersed call
struct Gravity {
  const double* Rtab;
  double gm;
};

// ... and the sensed calls to either law
struct Sensing {
  const tsat_sensor_options* s;
  const double* sensor;
};

// ... and the filtered calls to the sensed ones
struct Filtering {
  const tsat_filter_options* f;
  double *X_hat, *filt_final;
  const tsat_model_filter_options* mf = nullptr;   // the nine-state filter in place of f
  const tsat_mag_filter_options* gf = nullptr;     // ... or the magnetometer-updated one
  const tsat_mag_bias_filter_options* bf = nullptr;   // ... or the one that estimates the magnetometer bias too
  const tsat_model_mag_filter_options* mg = nullptr;  // ... or the nine-state filter updated by the magnetometer
  const tsat_model_mag_sun_filter_options* ms = nullptr;   // ... or that one with the sun-vector update, against Stab
  const double* Stab = nullptr;                       // n_btab x n_tab x 3, sun_rows rows
  double sigma_sun = 0.0;
  int64_t sun_rows = 0;
  std::string check() const {
    if (ms) return check_model_mag_sun_filter(ms, Stab, sigma_sun, sun_rows);
    if (mg) return check_model_mag_filter(mg);
    return bf ? check_mag_bias_filter(bf) : (gf ? check_mag_filter(gf) : (mf ? check_model_filter(mf) : check_filter(f)));
  }
  size_t final_w() const { return bf ? (size_t)MBFFW : ((mf || mg || ms) ? (size_t)MFFW : (size_t)FFW); }
};

// f == NULL is the sensed parent, which has no X_hat and no filt_final to fill
bool unfiltered_outputs(const double* X_hat, const double* filt_final) {
  if (!X_hat && !filt_final) return false;
  g_err = "f is NULL (the sensed call): X_hat and filt_final must be NULL";
  return true;
}

// ... and no sun table; without a sun table (the model-mag-filtered parent) there is no sun sensor to draw for
bool no_sun_arguments(bool has_f, const double* Stab, double sigma_sun) {
  const std::string bad = check_sun_arguments(has_f, Stab, sigma_sun);
  if (bad.empty()) return false;
  g_err = bad;
  return true;
}

std::string at_tm(int64_t t, int m) { return " at (t, m) = (" + std::to_string(t) + ", " + std::to_string(m) + ")"; }

// the host only validates the plants: "" or the reason, with the offending (t, m)
std::string check_dispersion(const Dispersion& d, int64_t T, int M) {
  if (!d.plant) return "null plant array";
  const std::string lim = check_limits(d.sat_lo, d.sat_hi, T);
  if (!lim.empty()) return lim;
  for (int64_t t = 0; t < T; ++t)
    for (int m = 0; m < M; ++m) {
      const std::string bad = check_plant_record(d.plant + ((size_t)t * M + m) * TSAT_PLANT_W);
      if (!bad.empty()) return bad + at_tm(t, m);
    }
  return "";
}

// what only the TVLQR entry points carry: the weights of the gain recursion and where K_lqr goes (or null)
struct TvlqrPart {
  const double *Qd, *Qfd, *Rd;
  double* K_lqr;
};

// ... and only the PD ones; with Kg the law is the asymptotic periodic LQR of tsat_aplqr_ensemble (Kg, rd) and kd, kp are null
struct PdPart {
  const double *kd, *kp;
  int32_t feedforward, limit_mode;
  const double* x0_nom;
  const double *Kg = nullptr, *rd = nullptr;
  bool aplqr = false;
};

// One call of any entry point: the arrays every one of them takes, the part of its law (exactly one of `tv` / `pd`), and what the
// call adds to tsat_tvlqr_ensemble (null: not this entry point). The PD calls always carry `disp` and `grav`.
struct Call {
  const char* name;
  tsat_handle* h;
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
  const TvlqrPart* tv = nullptr;
  const PdPart* pd = nullptr;
  const Dispersion* disp = nullptr;
  const Gravity* grav = nullptr;
  const Sensing* sens = nullptr;
  const Filtering* filt = nullptr;
};

// stage 1 of a TVLQR call: "" or the reason, in the order the entry points have always given them
std::string check_tvlqr(const Call& c) {
  const tsat_tvlqr_options* o = c.o;
  if (!c.h || !o) return "null handle or options";
  const std::string why = check_tv_options(*o);
  if (!why.empty()) return why;
  if (o->noise_mode != 1) return "noise_mode must be 1: the ensemble draws its noise in the kernel";
  if (o->rate_as_written != 0) return "rate_as_written must be 0: the statistic is evaluated while the roll-out runs";
  if (c.M < 1 || c.M > 65535) return "M must be in [1, 65535]";
  if (c.T < 1 || c.T > 0x7fffffff || c.n_btab < 1) return "bad batch dimensions";
  if (!c.X || !c.U || !c.xf || !c.Btab || !c.tau0 || !c.dtau || !c.dt || !c.Jmat || !c.tv->Qd || !c.tv->Qfd || !c.tv->Rd || !c.x0_sim ||
      !c.stats || !c.summary)
    return "null array";
  if (!c.btab_idx && c.n_btab != c.T) return "btab_idx is NULL but n_btab != T";
  for (int64_t t = 0; t < c.T; ++t) {
    const int64_t v = c.btab_idx ? c.btab_idx[t] : t;
    if (v < 0 || v >= c.n_btab) return "btab_idx out of range";
    if (!(c.dt[t] > 0.0)) return "dt must be positive";
    if (c.n_knots && (c.n_knots[t] < 2 || c.n_knots[t] > o->n_knots)) return "n_knots[t] must be in [2, N]";
  }
  if (c.disp) {   // the sensed call takes the model's plant for a NULL plant
    const std::string bad =
        (c.sens && !c.disp->plant) ? check_limits(c.disp->sat_lo, c.disp->sat_hi, c.T) : check_dispersion(*c.disp, c.T, c.M);
    if (!bad.empty()) return bad;
  }
  if (c.grav && c.sens && !c.grav->Rtab) {   // ... and the kernel without the gravity rows for a NULL Rtab
    if (!(c.grav->gm == 0.0)) return "Rtab is NULL but gm != 0: the gravity-gradient term needs the orbit table";
  } else if (c.grav) {
    const std::string bad = check_gravity(c.grav->Rtab, c.grav->gm, c.n_btab * (int64_t)o->n_tab);
    if (!bad.empty()) return bad;
  }
  return "";
}

// ... and of a PD call: check_pd is the authority
std::string check_pd_call(const Call& c) {
  if (!c.h) return "null handle or options";
  if (c.pd->aplqr)
    return check_aplqr(c.o, c.T, c.n_btab, c.M, c.X, c.U, c.xf, c.Btab, c.btab_idx, c.tau0, c.dtau, c.dt, c.Jmat, c.pd->Kg, c.pd->rd,
                       c.pd->feedforward, c.pd->limit_mode, c.x0_sim, c.pd->x0_nom, c.n_knots, c.disp->plant, c.disp->sat_lo,
                       c.disp->sat_hi, c.stats, c.summary, c.stats_nominal, c.grav->Rtab, c.grav->gm);
  return check_pd(c.o, c.T, c.n_btab, c.M, c.X, c.U, c.xf, c.Btab, c.btab_idx, c.tau0, c.dtau, c.dt, c.Jmat, c.pd->kd, c.pd->kp,
                  c.pd->feedforward, c.pd->limit_mode, c.x0_sim, c.pd->x0_nom, c.n_knots, c.disp->plant, c.disp->sat_lo, c.disp->sat_hi,
                  c.stats, c.summary, c.stats_nominal, c.grav->Rtab, c.grav->gm);
}

// stage 6, one dispatch per law: the nested argument block inside-out, then the unit that holds its kernel.
// d == null: tsat_tvlqr_ensemble (the kernel of the model's inertia class `cls`); GT == null: the plants without the gravity rows
hipError_t launch_tvlqr(const EnsArgs<double>& a, const DispArgs<double>* d, const double* GT, const SensArgs<double>* sa,
                        const Filtering* fl, double* dXH, double* dFF, const double* dST, int cls, int nw, hipStream_t st) {
  if (!d) {
    auto kern = cls == 2 ? tsat_ensemble_kernel<double, 2> : (cls == 1 ? tsat_ensemble_kernel<double, 1> : tsat_ensemble_kernel<double, 0>);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.T, (unsigned)nw), dim3(64), 0, st, a);
    return hipGetLastError();
  }
  const GgEnsArgs<double> g{*d, GT};
  if (fl && fl->ms)
    return tsat_launch_model_mag_sun_filtered_tv({g, model_mag_sun_filt_args(*fl->ms, *sa, a, dXH, dFF, dST, fl->sigma_sun)}, nw, st);
  if (fl && fl->mg) return tsat_launch_model_mag_filtered_tv({g, model_mag_filt_args(*fl->mg, *sa, a, dXH, dFF)}, nw, st);
  if (fl && fl->bf) return tsat_launch_mag_bias_filtered_tv({g, mag_bias_filt_args(*fl->bf, *sa, a, dXH, dFF)}, nw, st);
  if (fl && fl->gf) return tsat_launch_mag_filtered_tv({g, mag_filt_args(*fl->gf, *sa, a, dXH, dFF)}, nw, st);
  if (fl && fl->mf) return tsat_launch_model_filtered_tv({g, model_filt_args(*fl->mf, *sa, a, dXH, dFF)}, nw, st);
  if (fl) return tsat_launch_filtered_tv({g, filt_args(*fl->f, *sa, a, dXH, dFF)}, nw, st);
  if (sa) return tsat_launch_sensed_tv({g, *sa}, nw, st);
  if (GT) return tsat_launch_ensemble_gg(g, nw, st);
  hipLaunchKernelGGL(tsat_dispersed_kernel<double>, dim3((unsigned)a.T, (unsigned)nw), dim3(64), 0, st, *d);
  return hipGetLastError();
}

hipError_t launch_pd(const PdArgs<double>& pa, const SensArgs<double>* sa, const Filtering* fl, double* dXH, double* dFF,
                     const double* dST, int nw, hipStream_t st, bool aplqr) {
  if (aplqr) return tsat_launch_aplqr(pa, nw, st);             // GAIN holds [T][AQGW]; no sensed or filtered variant
  if (fl && fl->ms)
    return tsat_launch_model_mag_sun_filtered_pd({pa, model_mag_sun_filt_args(*fl->ms, *sa, pa.d.e, dXH, dFF, dST, fl->sigma_sun)}, nw, st);
  if (fl && fl->mg) return tsat_launch_model_mag_filtered_pd({pa, model_mag_filt_args(*fl->mg, *sa, pa.d.e, dXH, dFF)}, nw, st);
  if (fl && fl->bf) return tsat_launch_mag_bias_filtered_pd({pa, mag_bias_filt_args(*fl->bf, *sa, pa.d.e, dXH, dFF)}, nw, st);
  if (fl && fl->gf) return tsat_launch_mag_filtered_pd({pa, mag_filt_args(*fl->gf, *sa, pa.d.e, dXH, dFF)}, nw, st);
  if (fl && fl->mf) return tsat_launch_model_filtered_pd({pa, model_filt_args(*fl->mf, *sa, pa.d.e, dXH, dFF)}, nw, st);
  if (fl) return tsat_launch_filtered_pd({pa, filt_args(*fl->f, *sa, pa.d.e, dXH, dFF)}, nw, st);
  if (sa) return tsat_launch_sensed_pd({pa, *sa}, nw, st);
  return tsat_launch_pd(pa, nw, st);
}

#define ENS_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return efail(-10, std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)

// every entry point, in the stages of the header comment
int run_call(const Call& c) {
  const tsat_tvlqr_options* o = c.o;
  const int64_t T = c.T;
  const int32_t M = c.M;
  const Dispersion* disp = c.disp;
  const Sensing* sens = c.sens;
  const Filtering* filt = c.filt;
  // ---- 1. checks: the law's own sequence, then the sensor's and the filter's ------------------------------------------
  g_err.clear();
  {
    std::string bad = c.tv ? check_tvlqr(c) : check_pd_call(c);
    if (bad.empty() && sens) bad = check_sensor(sens->s, sens->sensor, T, M);
    if (bad.empty() && filt) bad = filt->check();
    if (!bad.empty()) return efail(-1, bad);
  }
  const Gravity* grav = (c.grav && c.grav->Rtab) ? c.grav : nullptr;   // a NULL Rtab that passed the checks: no gravity rows
  const int N = o->n_knots, n_tab = o->n_tab;
  const size_t Tn = (size_t)T;
  std::vector<int> bi(Tn);
  for (size_t t = 0; t < Tn; ++t) bi[t] = c.btab_idx ? c.btab_idx[t] : (int)t;
  // ---- 2. the handle: TVLQR runs the library's own checks on slew 0 cut to two knots, which leaves the handle's GPU current on
  //         the calling thread; PD only makes it current -------------------------------------------------------------------
  if (c.tv) {
    tsat_tvlqr_options op = *o;
    op.n_knots = 2; op.noise_mode = 0;
    tsat_tvlqr_stats probe;
    const int rc = tsat_tvlqr_batch(c.h, &op, 1, 1, c.X, c.U, c.xf, c.Btab + (size_t)bi[0] * n_tab * 3, nullptr, c.tau0, c.dtau, c.dt, c.Jmat,
                                    c.tv->Qd, c.tv->Qfd, c.tv->Rd, c.X, nullptr, nullptr, nullptr, nullptr, &probe, nullptr, nullptr);
    if (rc) return efail(rc, std::string("tsat_tvlqr_batch: ") + tsat_last_error(c.h));
  } else {
    ENS_HIP(hipSetDevice(tsat_handle_device(c.h)));
  }
  // ---- 3. allocation and upload: the plan only when there is one (a PD call without X regulates to xf) ----------------
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  const size_t nX = Tn * N * 7, nU = Tn * (size_t)(N - 1) * 3, nB = (size_t)c.n_btab * n_tab, nXU = Tn * N * XUW,
               nKD = Tn * (size_t)(N - 1) * KDW, nS = Tn * (size_t)M, nXS = c.X_sim ? nS * N * 7 : 0;
  const bool aplqr = c.pd && c.pd->aplqr;
  std::vector<double> P(Tn * PSTRIDE), x0n(Tn * 7), zero(c.pd ? Tn * 6 : 0, 0.0), gain((c.pd && !aplqr) ? Tn * PDGW : 0), model;
  for (size_t t = 0; t < Tn; ++t) {
    for (int i = 0; i < 7; ++i)
      x0n[7 * t + i] = (c.pd && c.pd->x0_nom) ? c.pd->x0_nom[7 * t + i] : (c.X ? c.X[t * N * 7 + i] : c.xf[7 * t + i]);
    for (int k = 0; c.pd && !aplqr && k < 3; ++k) {
      gain[PDGW * t + k] = c.pd->kd[3 * t + k];
      gain[PDGW * t + 3 + k] = c.pd->kp[3 * t + k];
    }
  }
  if (aplqr) gain = pack_aplqr_law(T, c.pd->Kg, c.pd->rd);
  if (c.tv) pack_tv_params<double>(T, x0n.data(), c.xf, c.tau0, c.dtau, c.dt, c.Jmat, c.tv->Qd, c.tv->Qfd, c.tv->Rd, P.data());
  else pack_tv_params<double>(T, x0n.data(), c.xf, c.tau0, c.dtau, c.dt, c.Jmat, zero.data(), zero.data(), zero.data(), P.data());
  const int cls = inertia_class(T, c.Jmat);
  const double* plant = disp ? disp->plant : nullptr;
  if (disp && !plant) {   // the model's plant for a NULL plant
    model = model_plants(c.Jmat, Tn, M);
    plant = model.data();
  }
  const std::vector<double> sat = disp ? pack_limits(disp->sat_lo, disp->sat_hi, T) : std::vector<double>();
  double* K_lqr = c.tv ? c.tv->K_lqr : nullptr;
  EnsScope s;
  double *dP = nullptr, *dX = nullptr, *dU = nullptr, *dB = nullptr, *dBT = nullptr, *dXU = nullptr, *dKD = nullptr, *dX0 = nullptr,
         *dX0N = nullptr, *dGain = nullptr, *dXS = nullptr, *dK = nullptr;
  int *dbi = nullptr, *dnk = nullptr;
  long long* dnid = nullptr;
  tsat_tvlqr_stats *dst = nullptr, *dsn = nullptr;
  bool ok = s.alloc(&dP, P.size()) && s.alloc(&dB, nB * 3) && s.alloc(&dBT, nB * 4) && s.alloc(&dX0, nS * 7) && s.alloc(&dbi, Tn) &&
            s.alloc(&dst, nS) && s.alloc(&dsn, Tn);
  if (ok && c.X) ok = s.alloc(&dX, nX) && s.alloc(&dU, nU) && s.alloc(&dXU, nXU);
  if (ok && c.tv) ok = s.alloc(&dKD, nKD);
  if (ok && c.pd) ok = s.alloc(&dX0N, Tn * 7) && s.alloc(&dGain, gain.size());
  if (ok && c.n_knots) ok = s.alloc(&dnk, Tn);
  if (ok && c.noise_id0) ok = s.alloc(&dnid, Tn);
  if (ok && c.X_sim) ok = s.alloc(&dXS, nXS);
  if (ok && K_lqr) ok = s.alloc(&dK, Tn * (size_t)(N - 1) * 18);
  // the dispersed call: raw plants, packed per-lane records, limits, clipped-knot counters
  double *dPlant = nullptr, *dPL = nullptr, *dSat = nullptr;
  int* dClip = nullptr;
  if (ok && disp) ok = s.alloc(&dPlant, nS * TSAT_PLANT_W) && s.alloc(&dPL, Tn * PLW * (size_t)Mp) && s.alloc(&dSat, Tn * SATW);
  if (ok && disp && disp->n_clipped) ok = s.alloc(&dClip, nS);
  // the gravity call: the raw orbit table is the call's, the packed rows are the handle's
  double *dR = nullptr, *dGT = nullptr;
  if (ok && grav) ok = s.alloc(&dR, nB * 3) && (dGT = tsat_ws_gravity(c.h, nB * 4 * 8)) != nullptr;
  // the sensed call: raw biases (when given) and the per-lane records
  double *dSens = nullptr, *dSN = nullptr;
  if (ok && sens) ok = s.alloc(&dSN, Tn * SNW * (size_t)Mp) && (!sens->sensor || s.alloc(&dSens, nS * SNW));
  // the filtered call: what the law saw and the filter's last state, when asked for
  double *dXH = nullptr, *dFF = nullptr;
  if (ok && filt && filt->X_hat) ok = s.alloc(&dXH, nS * N * 7);
  if (ok && filt && filt->filt_final) ok = s.alloc(&dFF, nS * filt->final_w());
  // the sun call: the raw sun table is the call's, the packed rows are the handle's
  double *dS = nullptr, *dST = nullptr;
  if (ok && filt && filt->ms) ok = s.alloc(&dS, nB * 3) && (dST = tsat_ws_sun(c.h, nB * 4 * 8)) != nullptr;
  if (!ok) return efail(-10, std::string("device allocation failed in ") + ((c.pd && !aplqr) ? "tsat_pd_ensemble" : c.name));
  ENS_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : s.ev) ENS_HIP(hipEventCreate(&e));
  ENS_HIP(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dB, c.Btab, nB * 3 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dX0, c.x0_sim, nS * 7 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dbi, bi.data(), Tn * sizeof(int), hipMemcpyHostToDevice));
  if (c.pd) {
    ENS_HIP(hipMemcpy(dX0N, x0n.data(), x0n.size() * 8, hipMemcpyHostToDevice));
    ENS_HIP(hipMemcpy(dGain, gain.data(), gain.size() * 8, hipMemcpyHostToDevice));
  }
  if (c.n_knots) ENS_HIP(hipMemcpy(dnk, c.n_knots, Tn * sizeof(int), hipMemcpyHostToDevice));
  if (c.noise_id0) ENS_HIP(hipMemcpy(dnid, c.noise_id0, Tn * sizeof(long long), hipMemcpyHostToDevice));
  // ---- 4. packs on the device ------------------------------------------------------------------------------------------
  if (c.X) {
    ENS_HIP(hipMemcpy(dX, c.X, nX * 8, hipMemcpyHostToDevice));
    if (c.tv || c.pd->feedforward) ENS_HIP(hipMemcpy(dU, c.U, nU * 8, hipMemcpyHostToDevice));
    else ENS_HIP(hipMemset(dU, 0, nU * 8));                  // U is not read without feed-forward: the records carry zeros
    const int64_t n_rec = T * (int64_t)N;
    hipLaunchKernelGGL(tsat_ensemble_pack_xu_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s.stream, n_rec, N, dX, dU, dXU);
  }
  hipLaunchKernelGGL(tsat_ensemble_pack_bt_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, s.stream, (int64_t)nB, dB, dBT);
  ENS_HIP(hipGetLastError());
  if (c.n_knots) {   // ragged: the slabs beyond a slew's own horizon stay zero
    if (dKD) ENS_HIP(hipMemsetAsync(dKD, 0, nKD * 8, s.stream));
    if (c.X_sim) ENS_HIP(hipMemsetAsync(dXS, 0, nXS * 8, s.stream));
  }
  if (disp) {
    ENS_HIP(hipMemcpy(dPlant, plant, nS * TSAT_PLANT_W * 8, hipMemcpyHostToDevice));
    ENS_HIP(hipMemcpy(dSat, sat.data(), sat.size() * 8, hipMemcpyHostToDevice));
    if (c.tv) ENS_HIP(hipEventRecord(s.ev[3], s.stream));
    const int64_t n = T * (int64_t)(M + 1);
    hipLaunchKernelGGL(tsat_dispersed_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, dPlant, dP, o->u_scale, dPL,
                       T, M, Mp);
    ENS_HIP(hipGetLastError());
  }
  if (grav) {
    ENS_HIP(hipMemcpy(dR, grav->Rtab, nB * 3 * 8, hipMemcpyHostToDevice));
    ENS_HIP(tsat_launch_gg_pack(dR, grav->gm, dGT, (int64_t)nB, s.stream));
  }
  if (sens) {
    if (sens->sensor) ENS_HIP(hipMemcpy(dSens, sens->sensor, nS * SNW * 8, hipMemcpyHostToDevice));
    ENS_HIP(tsat_launch_sensed_pack(dSens, dSN, T, M, Mp, s.stream));
  }
  if (dST) {                                                 // sun rows [rows][3] -> [rows][4]: the pack of the field rows
    ENS_HIP(hipMemcpy(dS, filt->Stab, nB * 3 * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(tsat_ensemble_pack_bt_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, s.stream, (int64_t)nB, dS, dST);
    ENS_HIP(hipGetLastError());
  }
  if (dXH) ENS_HIP(hipMemsetAsync(dXH, 0, nS * N * 7 * 8, s.stream));   // the last row of every horizon and all beyond it stay zero
  ENS_HIP(hipEventRecord(s.ev[0], s.stream));
  // ---- 5. the gains kernel (TVLQR): one wavefront per slew runs the gain half of the tracking kernel ------------------
  if (c.tv) {
    auto kern = cls == 2 ? tsat_ensemble_gains_kernel<double, 2>
                         : (cls == 1 ? tsat_ensemble_gains_kernel<double, 1> : tsat_ensemble_gains_kernel<double, 0>);
    hipLaunchKernelGGL(kern, dim3((unsigned)T), dim3(64), 0, s.stream, dP, dBT, dbi, dnk, dXU, dKD, N, n_tab, o->u_scale,
                       o->linearize_dt_sq);
    ENS_HIP(hipGetLastError());
    ENS_HIP(hipEventRecord(s.ev[1], s.stream));
  }
  // ---- 6. the roll-out: grid (T, ceil((M + 1) / 64)), the extra realisation is the noise-free plant -------------------
  {
    const EnsArgs<double> a = ens_args<EnsArgs<double>>(*o, T, M, dP, dBT, dbi, dnk, dXU, dKD, dX0, dnid, dXS, dst, dsn);
    const DispArgs<double> d{a, dPL, Mp, dSat, dClip};
    SensArgs<double> sa;
    if (sens) sa = sens_args(*sens->s, *o, dSN, Mp);
    if (c.tv) ENS_HIP(launch_tvlqr(a, disp ? &d : nullptr, dGT, sens ? &sa : nullptr, filt, dXH, dFF, dST, cls, nw, s.stream));
    else ENS_HIP(launch_pd({d, dGT, dGain, dX0N, c.pd->feedforward, c.pd->limit_mode}, sens ? &sa : nullptr, filt, dXH, dFF, dST, nw,
                         s.stream, aplqr));
  }
  ENS_HIP(hipEventRecord(s.ev[c.tv ? 2 : 1], s.stream));
  if (K_lqr) {
    const int64_t n = T * (int64_t)(N - 1);
    hipLaunchKernelGGL(tsat_ensemble_export_k_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, n, dKD, dK);
    ENS_HIP(hipGetLastError());
  }
  ENS_HIP(hipStreamSynchronize(s.stream));
  // ---- 7. download; `summary` is formed on the host in realisation order -----------------------------------------------
  ENS_HIP(hipMemcpy(c.stats, dst, nS * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (c.stats_nominal) ENS_HIP(hipMemcpy(c.stats_nominal, dsn, Tn * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (K_lqr) ENS_HIP(hipMemcpy(K_lqr, dK, Tn * (size_t)(N - 1) * 18 * 8, hipMemcpyDeviceToHost));
  if (c.X_sim) ENS_HIP(hipMemcpy(c.X_sim, dXS, nXS * 8, hipMemcpyDeviceToHost));
  if (dClip) ENS_HIP(hipMemcpy(disp->n_clipped, dClip, nS * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (dXH) ENS_HIP(hipMemcpy(filt->X_hat, dXH, nS * N * 7 * 8, hipMemcpyDeviceToHost));
  if (dFF) ENS_HIP(hipMemcpy(filt->filt_final, dFF, nS * filt->final_w() * 8, hipMemcpyDeviceToHost));
  ensemble_summary(T, M, c.stats, c.summary);
  if (const char* v = std::getenv("TSAT_ENSEMBLE_TIMING")) {   // diagnostic (tools/*_timing.py): HIP-event times of the kernels
    if (v[0] == '1') {
      float p = 0, g = 0, e = 0;
      if (c.pd) {
        (void)hipEventElapsedTime(&e, s.ev[0], s.ev[1]);
        std::fprintf(stderr, "%s: pd_kernel_ms %.4f\n", c.name, e);
      } else {
        (void)hipEventElapsedTime(&g, s.ev[0], s.ev[1]);
        (void)hipEventElapsedTime(&e, s.ev[1], s.ev[2]);
        if (disp) {
          (void)hipEventElapsedTime(&p, s.ev[3], s.ev[0]);
          std::fprintf(stderr, "%s: pack_kernel_ms %.4f gains_kernel_ms %.4f ensemble_kernel_ms %.4f\n", c.name, p, g, e);
        } else {
          std::fprintf(stderr, "tsat_tvlqr_ensemble: gains_kernel_ms %.4f ensemble_kernel_ms %.4f\n", g, e);
        }
      }
    }
  }
  return 0;
}

// tsat_aplqr_gains: checks, the handle's GPU, the parameter records and the tables up, one wavefront per slew, the results down
int run_aplqr_gains(tsat_handle* h, int64_t T, int64_t n_btab, int32_t n_tab, const double* xf, const double* Btab, const int32_t* btab_idx,
                    const int32_t* avg_lo, const int32_t* avg_hi, const double* Jmat, const double* qd, const double* rd,
                    const double* alpha, double res_tol, double* Kg, double* P_ss, double* Gamma, void* info) {
  g_err.clear();
  if (!h) return efail(-1, "null handle");
  const std::string bad = check_aplqr_gains(T, n_btab, n_tab, xf, Btab, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha, res_tol, Kg, info);
  if (!bad.empty()) return efail(-1, bad);
  ENS_HIP(hipSetDevice(tsat_handle_device(h)));
  const std::vector<double> gp = pack_aplqr_gains(T, n_tab, xf, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha);
  const size_t Tn = (size_t)T, nB = (size_t)n_btab * n_tab * 3;
  EnsScope s;
  double *dGP = nullptr, *dB = nullptr, *dKg = nullptr, *dP = nullptr, *dGam = nullptr;
  tsat_aplqr_info* dInfo = nullptr;
  if (!(s.alloc(&dGP, gp.size()) && s.alloc(&dB, nB) && s.alloc(&dKg, Tn * 18) && s.alloc(&dP, Tn * 36) && s.alloc(&dGam, Tn * 9) &&
        s.alloc(&dInfo, Tn)))
    return efail(-10, "device allocation failed in tsat_aplqr_gains");
  ENS_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) ENS_HIP(hipEventCreate(&s.ev[i]));
  ENS_HIP(hipMemcpy(dGP, gp.data(), gp.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dB, Btab, nB * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipEventRecord(s.ev[0], s.stream));
  ENS_HIP(tsat_launch_aplqr_gains({dGP, dB, n_tab, res_tol, dKg, dP, dGam, dInfo}, T, s.stream));
  ENS_HIP(hipEventRecord(s.ev[1], s.stream));
  ENS_HIP(hipStreamSynchronize(s.stream));
  ENS_HIP(hipMemcpy(Kg, dKg, Tn * 18 * 8, hipMemcpyDeviceToHost));
  if (P_ss) ENS_HIP(hipMemcpy(P_ss, dP, Tn * 36 * 8, hipMemcpyDeviceToHost));
  if (Gamma) ENS_HIP(hipMemcpy(Gamma, dGam, Tn * 9 * 8, hipMemcpyDeviceToHost));
  ENS_HIP(hipMemcpy(info, dInfo, Tn * sizeof(tsat_aplqr_info), hipMemcpyDeviceToHost));
  if (const char* v = std::getenv("TSAT_ENSEMBLE_TIMING")) {   // diagnostic (tools/aplqr_timing.py)
    if (v[0] == '1') {
      float e = 0;
      (void)hipEventElapsedTime(&e, s.ev[0], s.ev[1]);
      std::fprintf(stderr, "tsat_aplqr_gains: gains_kernel_ms %.4f\n", e);
    }
  }
  return 0;
}
#undef ENS_HIP

}  // namespace

extern "C" {

int tsat_pd_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                     const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                     const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                     int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                     const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats, double* summary,
                     tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm) {
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  Call c{"tsat_pd_ensemble", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats,
         summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g;
  return run_call(c);
}

int tsat_aplqr_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                        const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                        const double* dtau, const double* dt, const double* Jmat, const double* Kg, const double* rd, int32_t feedforward,
                        int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                        const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats, double* summary,
                        tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm) {
  const PdPart law{nullptr, nullptr, feedforward, limit_mode, x0_nom, Kg, rd, true};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  Call c{"tsat_aplqr_ensemble", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats,
         summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g;
  return run_call(c);
}

int tsat_aplqr_gains(tsat_handle* h, int64_t T, int64_t n_btab, int32_t n_tab, const double* xf, const double* Btab,
                     const int32_t* btab_idx, const int32_t* avg_lo, const int32_t* avg_hi, const double* Jmat, const double* qd,
                     const double* rd, const double* alpha, double res_tol, double* Kg, double* P_ss, double* Gamma, void* info) {
  return run_aplqr_gains(h, T, n_btab, n_tab, xf, Btab, btab_idx, avg_lo, avg_hi, Jmat, qd, rd, alpha, res_tol, Kg, P_ss, Gamma, info);
}

int tsat_pd_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                            const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                            const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                            int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                            const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                            tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped,
                            const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor) {
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  Call c{"tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats,
         summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se;
  return run_call(c);
}

int tsat_pd_ensemble_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                              const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                              const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                              int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                              const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                              tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped,
                              const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor,
                              const tsat_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{f, X_hat, filt_final};
  Call c{f ? "tsat_pd_ensemble_filtered" : "tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat,
         x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_pd_ensemble_model_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                    const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                    const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                    int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                    const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                    const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                    double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                    const double* sensor, const tsat_model_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, f};
  Call c{f ? "tsat_pd_ensemble_model_filtered" : "tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt,
         Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_pd_ensemble_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                  const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                  const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                  int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                  const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                  const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                  double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                  const double* sensor, const tsat_mag_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, f};
  Call c{f ? "tsat_pd_ensemble_mag_filtered" : "tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt,
         Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_pd_ensemble_mag_bias_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                       const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                       const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                       int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                       const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                       const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                       double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                       const double* sensor, const tsat_mag_bias_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, nullptr, f};
  Call c{f ? "tsat_pd_ensemble_mag_bias_filtered" : "tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt,
         Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_pd_ensemble_model_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                        const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                        const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                                        int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom,
                                        const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
                                        const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                                        double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                        const double* sensor, const tsat_model_mag_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, nullptr, nullptr, f};
  Call c{f ? "tsat_pd_ensemble_model_mag_filtered" : "tsat_pd_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt,
         Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

void tsat_model_mag_filter_default_options(tsat_model_mag_filter_options* f) {
  if (!f) return;
  const double pi = 3.14159265358979323846;
  f->sigma_v = 0.0; f->sigma_w = 0.0; f->sigma_u = 0.0;       // sigma_w: the caller's choice, as for the model filter
  f->sigma_g = 0.38 * pi / 180.0;
  f->sigma_m = 0.0;                                            // in the units of the caller's table: no default, and 0 is rejected
  f->p0_att = pi / 180.0; f->p0_bias = 0.0;
  f->reserved = 0;
}

void tsat_mag_bias_filter_default_options(tsat_mag_bias_filter_options* f) {
  if (!f) return;
  tsat_mag_filter_options g;
  tsat_mag_filter_default_options(&g);                         // the mag filter's figures, sigma_m left 0 and rejected at 0
  f->sigma_v = g.sigma_v; f->sigma_u = g.sigma_u; f->sigma_m = g.sigma_m; f->p0_att = g.p0_att; f->p0_bias = g.p0_bias;
  f->sigma_c = 0.0; f->p0_mag = 0.0;                           // in the units of the caller's table: no bias state without them
  f->reserved = 0;
}

void tsat_mag_filter_default_options(tsat_mag_filter_options* f) {
  if (!f) return;
  const double pi = 3.14159265358979323846;
  f->sigma_v = 0.38 * pi / 180.0; f->sigma_u = 0.0;             // the levels tsat_filter_default_options takes
  f->sigma_m = 0.0;                                            // in the units of the caller's table: no default, and 0 is rejected
  f->p0_att = pi / 180.0; f->p0_bias = 0.0;
  f->reserved = 0;
}

void tsat_model_filter_default_options(tsat_model_filter_options* f) {
  if (!f) return;
  const double pi = 3.14159265358979323846;
  f->sigma_v = 0.0; f->sigma_w = 0.0; f->sigma_u = 0.0;       // sigma_w has no default that could be derived: the caller's choice
  f->sigma_a = pi / 180.0; f->sigma_g = 0.38 * pi / 180.0;     // the levels tsat_filter_default_options takes
  f->p0_att = pi / 180.0; f->p0_bias = 0.0;
  f->reserved = 0;
}

void tsat_filter_default_options(tsat_filter_options* f) {
  if (!f) return;
  const double pi = 3.14159265358979323846;
  f->sigma_v = 0.38 * pi / 180.0; f->sigma_u = 0.0; f->sigma_a = pi / 180.0;   // the levels examples/sensed_slew.py flies
  f->p0_att = pi / 180.0; f->p0_bias = 0.0;
  f->reserved = 0;
}

void tsat_sensor_default_options(tsat_sensor_options* s) {
  if (!s) return;
  s->sigma_gyro = 0.0; s->sigma_att = 0.0; s->sigma_mag = 0.0;
  s->latency = 0; s->reserved = 0;
}

const char* tsat_ensemble_last_error(void) { return g_err.c_str(); }

int tsat_tvlqr_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                        const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                        const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                        const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                        tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr,
                        double* X_sim) {
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  Call c{"tsat_tvlqr_ensemble", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats,
         summary, stats_nominal, X_sim};
  c.tv = &law;
  return run_call(c);
}

int tsat_tvlqr_ensemble_dispersed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                  const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                  const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                  const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                  const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                                  double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim,
                                  int32_t* n_clipped) {
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  Call c{"tsat_tvlqr_ensemble_dispersed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots,
         stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d;
  return run_call(c);
}

int tsat_tvlqr_ensemble_gg(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                           const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                           const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                           const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                           const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                           double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                           const double* Rtab, double gm) {
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  Call c{"tsat_tvlqr_ensemble_gg", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats,
         summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g;
  return run_call(c);
}

int tsat_tvlqr_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                               const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                               const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                               const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                               const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                               double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                               const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor) {
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  Call c{"tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0, n_knots,
         stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se;
  return run_call(c);
}

int tsat_tvlqr_ensemble_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                 const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                 const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                 const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                 const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                                 double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                                 const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor,
                                 const tsat_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{f, X_hat, filt_final};
  Call c{f ? "tsat_tvlqr_ensemble_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt,
         Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_tvlqr_ensemble_model_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                       const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                       const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                       const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                       const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                       tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr,
                                       double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                       const double* sensor, const tsat_model_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, f};
  Call c{f ? "tsat_tvlqr_ensemble_model_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau,
         dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_tvlqr_ensemble_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                     const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                     const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                     const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                     const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                                     double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                                     const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor,
                                     const tsat_mag_filter_options* f, double* X_hat, double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, f};
  Call c{f ? "tsat_tvlqr_ensemble_mag_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau,
         dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_tvlqr_ensemble_mag_bias_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                          const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                          const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                          const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                          const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                          tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr,
                                          double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                          const double* sensor, const tsat_mag_bias_filter_options* f, double* X_hat,
                                          double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, nullptr, f};
  Call c{f ? "tsat_tvlqr_ensemble_mag_bias_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0,
         dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

int tsat_tvlqr_ensemble_model_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                           const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                           const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                                           const double* Qfd, const double* Rd, const double* x0_sim, const int64_t* noise_id0,
                                           const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                                           tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr,
                                           double* X_sim, int32_t* n_clipped, const double* Rtab, double gm, const tsat_sensor_options* sn,
                                           const double* sensor, const tsat_model_mag_filter_options* f, double* X_hat,
                                           double* filt_final) {
  if (!f && unfiltered_outputs(X_hat, filt_final)) return -1;
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, nullptr, nullptr, nullptr, f};
  Call c{f ? "tsat_tvlqr_ensemble_model_mag_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0,
         dtau, dt, Jmat, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = f ? &fl : nullptr;
  return run_call(c);
}

void tsat_model_mag_sun_filter_default_options(tsat_model_mag_sun_filter_options* f) {
  if (!f) return;
  tsat_model_mag_filter_options g;
  tsat_model_mag_filter_default_options(&g);
  f->sigma_v = g.sigma_v; f->sigma_w = g.sigma_w; f->sigma_u = g.sigma_u; f->sigma_g = g.sigma_g; f->sigma_m = g.sigma_m;
  f->sigma_s = 0.0;                                            // the caller's sensor: no default, and 0 is rejected with a sun table
  f->p0_att = g.p0_att; f->p0_bias = g.p0_bias;
  f->reserved = 0;
}

int tsat_tvlqr_ensemble_model_mag_sun_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                                               const double* X, const double* U, const double* xf, const double* Btab,
                                               const int32_t* btab_idx, const double* tau0, const double* dtau, const double* dt,
                                               const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                                               const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                                               const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats, double* summary,
                                               tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                                               const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor,
                                               const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final,
                                               const double* Stab, double sigma_sun) {
  if (no_sun_arguments(f != nullptr, Stab, sigma_sun)) return -1;
  if (!Stab) {   // no sun table: the parent on the seven shared options (f == NULL: its sensed call), byte for byte
    tsat_model_mag_filter_options g;
    if (f) g = model_mag_options_of(*f);
    return tsat_tvlqr_ensemble_model_mag_filtered(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim,
                                                  noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, K_lqr, X_sim,
                                                  n_clipped, Rtab, gm, sn, sensor, f ? &g : nullptr, X_hat, filt_final);
  }
  const TvlqrPart law{Qd, Qfd, Rd, K_lqr};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  Filtering fl{nullptr, X_hat, filt_final};
  fl.ms = f; fl.Stab = Stab; fl.sigma_sun = sigma_sun; fl.sun_rows = o ? n_btab * (int64_t)o->n_tab : 0;
  Call c{"tsat_tvlqr_ensemble_model_mag_sun_filtered", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0,
         n_knots, stats, summary, stats_nominal, X_sim};
  c.tv = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = &fl;
  return run_call(c);
}

int tsat_pd_ensemble_model_mag_sun_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                                            const double* X, const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                                            const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* kd,
                                            const double* kp, int32_t feedforward, int32_t limit_mode, const double* x0_sim,
                                            const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots, const double* plant,
                                            const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats, double* summary,
                                            tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                                            const tsat_sensor_options* sn, const double* sensor,
                                            const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final,
                                            const double* Stab, double sigma_sun) {
  if (no_sun_arguments(f != nullptr, Stab, sigma_sun)) return -1;
  if (!Stab) {   // no sun table: the parent on the seven shared options (f == NULL: its sensed call), byte for byte
    tsat_model_mag_filter_options g;
    if (f) g = model_mag_options_of(*f);
    return tsat_pd_ensemble_model_mag_filtered(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward,
                                               limit_mode, x0_sim, x0_nom, noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary,
                                               stats_nominal, X_sim, n_clipped, Rtab, gm, sn, sensor, f ? &g : nullptr, X_hat, filt_final);
  }
  const PdPart law{kd, kp, feedforward, limit_mode, x0_nom};
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  Filtering fl{nullptr, X_hat, filt_final};
  fl.ms = f; fl.Stab = Stab; fl.sigma_sun = sigma_sun; fl.sun_rows = o ? n_btab * (int64_t)o->n_tab : 0;
  Call c{"tsat_pd_ensemble_model_mag_sun_filtered", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, x0_sim, noise_id0,
         n_knots, stats, summary, stats_nominal, X_sim};
  c.pd = &law; c.disp = &d; c.grav = &g; c.sens = &se; c.filt = &fl;
  return run_call(c);
}

}  // extern "C"
