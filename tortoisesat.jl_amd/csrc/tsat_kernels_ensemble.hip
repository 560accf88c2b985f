// tsat_kernels_ensemble.hip — tsat_tvlqr_ensemble (include/tortoise_hip.h): TVLQR gains once per slew, then M noisy plants per
// slew with lane = realisation (tsat_ensemble.hpp). A translation unit of its own, built on the public ABI: `struct tsat_handle`
// is private to tsat_kernels.hip, so the call keeps its own buffers and stream.
//
// Host side of one call (all of it synchronous):
//   1. argument checks; a one-slew, two-knot call of tsat_tvlqr_batch validates the handle and the options block with the
//      library's own checks and leaves the handle's GPU current on the calling thread;
//   2. X, U and the field tables go up AS THEY ARE (no host-side repacking of 10 N T doubles) and are packed into knot records
//      and padded table rows by two copy kernels on the device;
//   3. the gains kernel: one wavefront per slew runs the gain half of the tracking kernel — the same device functions
//      (tv_jacobian_chunk, riccati_chunk), so K is what tsat_tvlqr_batch returns, and it never leaves the device unless asked for;
//   4. the ensemble kernel: grid (T, ceil((M + 1) / 64)); the extra realisation is the noise-free plant from the plan's own
//      first state (stats_nominal);
//   5. statistics (and K / X_sim when asked for) come down; `summary` is formed on the host in realisation order.
//
// tsat_tvlqr_ensemble_dispersed is the same call with a plant per realisation and limits on the command (tsat_dispersed.hpp):
// the host validates the plants, a pack kernel forms inv(Jp) and the per-lane records between steps 2 and 3, and step 4
// launches the dispersed kernel instead. tsat_tvlqr_ensemble_gg is the dispersed call under gravity-gradient torque
// (tsat_gg.hpp): the host validates the orbit table, a pack kernel turns it into gravity rows in a grow-only workspace of the
// handle, and step 4 launches the kernel of tsat_kernels_gg.hip. Steps 1-3 and 5 are one piece of code for all entry points
// (run_ensemble).
//
// tsat_pd_ensemble (tsat_pd.hpp) flies the projection PD law on the same plants (run_pd): no step 1 and no step 3 — there are no
// gains —, the plan goes up only when the call tracks one (X == NULL regulates to xf and uploads nothing of size N), the plant
// pack and the gravity-row pack are the ones above, and step 4 launches a kernel of tsat_kernels_pd.hip.
//
// tsat_tvlqr_ensemble_sensed and tsat_pd_ensemble_sensed (tsat_sensed.hpp) are run_ensemble and run_pd with a `Sensing`: the host
// validates the sensor options and biases (check_sensor), a pack kernel lays the biases out per lane, and step 4 launches a kernel
// of tsat_kernels_sensed.hip. The TVLQR one also takes the model's plant for a NULL plant and no gravity rows for a NULL Rtab.
//
// tsat_tvlqr_ensemble_filtered and tsat_pd_ensemble_filtered (tsat_filtered.hpp) are the sensed calls with a `Filtering`: the host
// validates the filter options (check_filter), zero-fills X_hat when asked for, and step 4 launches a kernel of
// tsat_kernels_filtered.hip. f == NULL is dispatched to the sensed call itself.
//
// tsat_tvlqr_ensemble_model_filtered and tsat_pd_ensemble_model_filtered (tsat_model_filtered.hpp) are the same with a `Filtering`
// that names the nine-state filter's options (check_model_filter, the kernels of tsat_kernels_model_filtered.hip).
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

using namespace tsat;

// pack and roll-out of tsat_tvlqr_ensemble_gg (tsat_kernels_gg.hip); the handle's workspace for the packed gravity rows,
// counted by tsat_workspace_bytes (tsat_kernels.hip)
hipError_t tsat_launch_gg_pack(const double* R, double gm, double* GT, int64_t rows, hipStream_t stream);
hipError_t tsat_launch_ensemble_gg(const GgEnsArgs<double>& g, int waves, hipStream_t stream);
double* tsat_ws_gravity(tsat_handle* h, size_t bytes);
// roll-out of tsat_pd_ensemble (tsat_kernels_pd.hip); the handle's GPU (tsat_kernels.hip)
hipError_t tsat_launch_pd(const PdArgs<double>& a, int waves, hipStream_t stream);
int tsat_handle_device(const tsat_handle* h);
// pack and roll-outs of the sensed calls (tsat_kernels_sensed.hip)
hipError_t tsat_launch_sensed_pack(const double* sensor, double* SN, int64_t T, int M, int Mp, hipStream_t stream);
hipError_t tsat_launch_sensed_tv(const SensedTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_sensed_pd(const SensedPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the filtered calls (tsat_kernels_filtered.hip)
hipError_t tsat_launch_filtered_tv(const FilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_filtered_pd(const FilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the model-filtered calls (tsat_kernels_model_filtered.hip)
hipError_t tsat_launch_model_filtered_tv(const ModelFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_model_filtered_pd(const ModelFilteredPdArgs<double>& a, int waves, hipStream_t stream);

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
  std::string check() const { return mf ? check_model_filter(mf) : check_filter(f); }
  size_t final_w() const { return mf ? (size_t)MFFW : (size_t)FFW; }
};

// every realisation flies the model's plant: (Jmat, G = I, m_res = 0); the pack reads the upper triangle of Jp
std::vector<double> model_plants(const double* Jmat, size_t Tn, int M) {
  std::vector<double> model(Tn * (size_t)M * TSAT_PLANT_W, 0.0);
  for (size_t t = 0; t < Tn; ++t)
    for (int m = 0; m < M; ++m) {
      double* pl = model.data() + (t * M + m) * TSAT_PLANT_W;
      for (int i = 0; i < 9; ++i) pl[i] = Jmat[9 * t + i];
      pl[9] = pl[13] = pl[17] = 1.0;
    }
  return model;
}

// the launch block of the sensor from the options of both calls
SensArgs<double> sens_args(const Sensing& sn, const tsat_tvlqr_options* o, const double* dSN, int Mp) {
  SensArgs<double> a;
  a.SN = dSN; a.Mp = Mp; a.sgy = sn.s->sigma_gyro; a.sat = sn.s->sigma_att; a.smg = sn.s->sigma_mag; a.latency = sn.s->latency;
  a.k0 = (unsigned)(o->noise_seed & 0xFFFFFFFFull); a.k1 = (unsigned)(o->noise_seed >> 32);
  return a;
}

// the launch block of the filter around that of its sensor
FiltArgs<double> filt_args(const Filtering& fl, const SensArgs<double>& sa, const EnsArgs<double>& e, double* dXH, double* dFF) {
  FiltArgs<double> a;
  a.s = sa; a.P = e.P; a.nk = e.nk; a.M = e.M; a.N = e.N;
  a.sv = fl.f->sigma_v; a.su = fl.f->sigma_u; a.sa = fl.f->sigma_a; a.p0a = fl.f->p0_att; a.p0b = fl.f->p0_bias;
  a.XH = dXH; a.FF = dFF;
  return a;
}

// ... and of the nine-state filter, which reads the slew's constants and field rows itself
ModelFiltArgs<double> model_filt_args(const Filtering& fl, const SensArgs<double>& sa, const EnsArgs<double>& e, double* dXH, double* dFF) {
  ModelFiltArgs<double> a;
  const tsat_model_filter_options& o = *fl.mf;
  a.s = sa; a.P = e.P; a.BT = e.BT; a.bidx = e.bidx; a.nk = e.nk; a.M = e.M; a.N = e.N; a.n_tab = e.n_tab; a.us = e.us;
  a.sv = o.sigma_v; a.sw = o.sigma_w; a.su = o.sigma_u; a.sa = o.sigma_a; a.sg = o.sigma_g; a.p0a = o.p0_att; a.p0b = o.p0_bias;
  a.XH = dXH; a.FF = dFF;
  return a;
}

// f == NULL is the sensed parent, which has no X_hat and no filt_final to fill
bool unfiltered_outputs(const double* X_hat, const double* filt_final) {
  if (!X_hat && !filt_final) return false;
  g_err = "f is NULL (the sensed call): X_hat and filt_final must be NULL";
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

// all entry points: `disp` == nullptr is tsat_tvlqr_ensemble, `grav` != nullptr (with `disp`) tsat_tvlqr_ensemble_gg, `sens` != nullptr
// (with both) tsat_tvlqr_ensemble_sensed, `filt` != nullptr (with all three) tsat_tvlqr_ensemble_filtered
int run_ensemble(const char* name, tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                 const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                 const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                 const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                 tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr,
                 double* X_sim, const Dispersion* disp, const Gravity* grav = nullptr, const Sensing* sens = nullptr,
                 const Filtering* filt = nullptr) {
  g_err.clear();
  if (!h || !o) return efail(-1, "null handle or options");
  const std::string why = check_tv_options(*o);
  if (!why.empty()) return efail(-1, why);
  if (o->noise_mode != 1) return efail(-1, "noise_mode must be 1: the ensemble draws its noise in the kernel");
  if (o->rate_as_written != 0) return efail(-1, "rate_as_written must be 0: the statistic is evaluated while the roll-out runs");
  if (M < 1 || M > 65535) return efail(-1, "M must be in [1, 65535]");
  if (T < 1 || T > 0x7fffffff || n_btab < 1) return efail(-1, "bad batch dimensions");
  if (!X || !U || !xf || !Btab || !tau0 || !dtau || !dt || !Jmat || !Qd || !Qfd || !Rd || !x0_sim || !stats || !summary)
    return efail(-1, "null array");
  if (!btab_idx && n_btab != T) return efail(-1, "btab_idx is NULL but n_btab != T");
  const int N = o->n_knots, n_tab = o->n_tab;
  const size_t Tn = (size_t)T;
  std::vector<int> bi(Tn);
  for (int64_t t = 0; t < T; ++t) {
    const int64_t v = btab_idx ? btab_idx[t] : t;
    if (v < 0 || v >= n_btab) return efail(-1, "btab_idx out of range");
    if (!(dt[t] > 0.0)) return efail(-1, "dt must be positive");
    if (n_knots && (n_knots[t] < 2 || n_knots[t] > N)) return efail(-1, "n_knots[t] must be in [2, N]");
    bi[(size_t)t] = (int)v;
  }
  if (disp) {   // the sensed call takes the model's plant for a NULL plant
    const std::string bad = (sens && !disp->plant) ? check_limits(disp->sat_lo, disp->sat_hi, T) : check_dispersion(*disp, T, M);
    if (!bad.empty()) return efail(-1, bad);
  }
  if (grav && sens && !grav->Rtab) {   // ... and the kernel without the gravity rows for a NULL Rtab
    if (!(grav->gm == 0.0)) return efail(-1, "Rtab is NULL but gm != 0: the gravity-gradient term needs the orbit table");
    grav = nullptr;
  }
  if (grav) {
    const std::string bad = check_gravity(grav->Rtab, grav->gm, n_btab * (int64_t)o->n_tab);
    if (!bad.empty()) return efail(-1, bad);
  }
  if (sens) {
    const std::string bad = check_sensor(sens->s, sens->sensor, T, M);
    if (!bad.empty()) return efail(-1, bad);
  }
  if (filt) {
    const std::string bad = filt->check();
    if (!bad.empty()) return efail(-1, bad);
  }
  // ---- 1. the handle: the library's own checks on slew 0 cut to two knots; its GPU becomes the thread's current device ----
  {
    tsat_tvlqr_options op = *o;
    op.n_knots = 2; op.noise_mode = 0;
    tsat_tvlqr_stats probe;
    const int rc = tsat_tvlqr_batch(h, &op, 1, 1, X, U, xf, Btab + (size_t)bi[0] * n_tab * 3, nullptr, tau0, dtau, dt, Jmat, Qd, Qfd,
                                    Rd, X, nullptr, nullptr, nullptr, nullptr, &probe, nullptr, nullptr);
    if (rc) return efail(rc, std::string("tsat_tvlqr_batch: ") + tsat_last_error(h));
  }
  // ---- 2. upload ---------------------------------------------------------------------------------------------------
  const int nw = ensemble_waves(M);
  const size_t nX = Tn * N * 7, nU = Tn * (size_t)(N - 1) * 3, nB = (size_t)n_btab * n_tab, nXU = Tn * N * XUW,
               nKD = Tn * (size_t)(N - 1) * KDW, nS = Tn * (size_t)M, nXS = X_sim ? nS * N * 7 : 0;
  std::vector<double> P(Tn * PSTRIDE), x0n(Tn * 7);
  for (size_t t = 0; t < Tn; ++t)
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = X[t * N * 7 + i];
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, P.data());
  const int cls = inertia_class(T, Jmat);
  EnsScope s;
  double *dP = nullptr, *dX = nullptr, *dU = nullptr, *dB = nullptr, *dBT = nullptr, *dXU = nullptr, *dKD = nullptr, *dX0 = nullptr,
         *dXS = nullptr, *dK = nullptr;
  int *dbi = nullptr, *dnk = nullptr;
  long long* dnid = nullptr;
  tsat_tvlqr_stats *dst = nullptr, *dsn = nullptr;
  bool ok = s.alloc(&dP, P.size()) && s.alloc(&dX, nX) && s.alloc(&dU, nU) && s.alloc(&dB, nB * 3) && s.alloc(&dBT, nB * 4) &&
            s.alloc(&dXU, nXU) && s.alloc(&dKD, nKD) && s.alloc(&dX0, nS * 7) && s.alloc(&dbi, Tn) && s.alloc(&dst, nS) &&
            s.alloc(&dsn, Tn);
  if (ok && n_knots) ok = s.alloc(&dnk, Tn);
  if (ok && noise_id0) ok = s.alloc(&dnid, Tn);
  if (ok && X_sim) ok = s.alloc(&dXS, nXS);
  if (ok && K_lqr) ok = s.alloc(&dK, Tn * (size_t)(N - 1) * 18);
  // the dispersed call: raw plants, packed per-lane records, limits, clipped-knot counters
  const int Mp = nw * WAVE;
  double *dPlant = nullptr, *dPL = nullptr, *dSat = nullptr;
  int* dClip = nullptr;
  if (ok && disp) ok = s.alloc(&dPlant, nS * TSAT_PLANT_W) && s.alloc(&dPL, Tn * PLW * (size_t)Mp) && s.alloc(&dSat, Tn * SATW);
  if (ok && disp && disp->n_clipped) ok = s.alloc(&dClip, nS);
  // the gravity call: the raw orbit table is the call's, the packed rows are the handle's
  double *dR = nullptr, *dGT = nullptr;
  if (ok && grav) ok = s.alloc(&dR, nB * 3) && (dGT = tsat_ws_gravity(h, nB * 4 * 8)) != nullptr;
  // the sensed call: raw biases (when given) and the per-lane records
  double *dSens = nullptr, *dSN = nullptr;
  if (ok && sens) ok = s.alloc(&dSN, Tn * SNW * (size_t)Mp) && (!sens->sensor || s.alloc(&dSens, nS * SNW));
  // the filtered call: what the law saw and the filter's last state, when asked for
  double *dXH = nullptr, *dFF = nullptr;
  if (ok && filt && filt->X_hat) ok = s.alloc(&dXH, nS * N * 7);
  if (ok && filt && filt->filt_final) ok = s.alloc(&dFF, nS * filt->final_w());
  if (!ok) return efail(-10, std::string("device allocation failed in ") + name);
#define ENS_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return efail(-10, std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)
  ENS_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : s.ev) ENS_HIP(hipEventCreate(&e));
  ENS_HIP(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dX, X, nX * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dU, U, nU * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dB, Btab, nB * 3 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dX0, x0_sim, nS * 7 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dbi, bi.data(), Tn * sizeof(int), hipMemcpyHostToDevice));
  if (n_knots) ENS_HIP(hipMemcpy(dnk, n_knots, Tn * sizeof(int), hipMemcpyHostToDevice));
  if (noise_id0) ENS_HIP(hipMemcpy(dnid, noise_id0, Tn * sizeof(long long), hipMemcpyHostToDevice));
  // ---- 3. pack on the device, gains, 4. ensemble ---------------------------------------------------------------------
  const int64_t n_rec = T * (int64_t)N;
  hipLaunchKernelGGL(tsat_ensemble_pack_xu_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s.stream, n_rec, N, dX, dU, dXU);
  hipLaunchKernelGGL(tsat_ensemble_pack_bt_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, s.stream, (int64_t)nB, dB, dBT);
  ENS_HIP(hipGetLastError());
  if (n_knots) {   // ragged: the slabs beyond a slew's own horizon stay zero
    ENS_HIP(hipMemsetAsync(dKD, 0, nKD * 8, s.stream));
    if (X_sim) ENS_HIP(hipMemsetAsync(dXS, 0, nXS * 8, s.stream));
  }
  if (disp) {
    const std::vector<double> sat = pack_limits(disp->sat_lo, disp->sat_hi, T);
    const std::vector<double> model = disp->plant ? std::vector<double>() : model_plants(Jmat, Tn, M);
    ENS_HIP(hipMemcpy(dPlant, disp->plant ? disp->plant : model.data(), nS * TSAT_PLANT_W * 8, hipMemcpyHostToDevice));
    ENS_HIP(hipMemcpy(dSat, sat.data(), sat.size() * 8, hipMemcpyHostToDevice));
    ENS_HIP(hipEventRecord(s.ev[3], s.stream));
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
  if (dXH) ENS_HIP(hipMemsetAsync(dXH, 0, nS * N * 7 * 8, s.stream));   // the last row of every horizon and all beyond it stay zero
  ENS_HIP(hipEventRecord(s.ev[0], s.stream));
  {
    auto kern = cls == 2 ? tsat_ensemble_gains_kernel<double, 2>
                         : (cls == 1 ? tsat_ensemble_gains_kernel<double, 1> : tsat_ensemble_gains_kernel<double, 0>);
    hipLaunchKernelGGL(kern, dim3((unsigned)T), dim3(64), 0, s.stream, dP, dBT, dbi, dnk, dXU, dKD, N, n_tab, o->u_scale,
                       o->linearize_dt_sq);
    ENS_HIP(hipGetLastError());
  }
  ENS_HIP(hipEventRecord(s.ev[1], s.stream));
  {
    EnsArgs<double> a;
    a.T = (int)T; a.N = N; a.n_tab = n_tab; a.M = M; a.us = o->u_scale;
    fill_ens_options(*o, a);
    a.P = dP; a.BT = dBT; a.bidx = dbi; a.nk = dnk; a.XUR = dXU; a.KD = dKD; a.X0 = dX0;
    a.nid0 = dnid;
    a.XS = dXS; a.stats = dst; a.stats_nom = dsn;
    if (disp) {
      DispArgs<double> d;
      d.e = a; d.PL = dPL; d.Mp = Mp; d.SAT = dSat; d.nclip = dClip;
      if (filt && filt->mf) {
        ModelFilteredTvArgs<double> fa;
        fa.g.d = d; fa.g.GT = dGT;
        fa.f = model_filt_args(*filt, sens_args(*sens, o, dSN, Mp), a, dXH, dFF);
        ENS_HIP(tsat_launch_model_filtered_tv(fa, nw, s.stream));
      } else if (filt) {
        FilteredTvArgs<double> fa;
        fa.g.d = d; fa.g.GT = dGT;
        fa.f = filt_args(*filt, sens_args(*sens, o, dSN, Mp), a, dXH, dFF);
        ENS_HIP(tsat_launch_filtered_tv(fa, nw, s.stream));
      } else if (sens) {
        SensedTvArgs<double> sa;
        sa.g.d = d; sa.g.GT = dGT;
        sa.s = sens_args(*sens, o, dSN, Mp);
        ENS_HIP(tsat_launch_sensed_tv(sa, nw, s.stream));
      } else if (grav) {
        GgEnsArgs<double> g;
        g.d = d; g.GT = dGT;
        ENS_HIP(tsat_launch_ensemble_gg(g, nw, s.stream));
      } else {
        hipLaunchKernelGGL(tsat_dispersed_kernel<double>, dim3((unsigned)T, (unsigned)nw), dim3(64), 0, s.stream, d);
      }
    } else {
      auto kern = cls == 2 ? tsat_ensemble_kernel<double, 2> : (cls == 1 ? tsat_ensemble_kernel<double, 1> : tsat_ensemble_kernel<double, 0>);
      hipLaunchKernelGGL(kern, dim3((unsigned)T, (unsigned)nw), dim3(64), 0, s.stream, a);
    }
    ENS_HIP(hipGetLastError());
  }
  ENS_HIP(hipEventRecord(s.ev[2], s.stream));
  if (K_lqr) {
    const int64_t n = T * (int64_t)(N - 1);
    hipLaunchKernelGGL(tsat_ensemble_export_k_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, n, dKD, dK);
    ENS_HIP(hipGetLastError());
  }
  ENS_HIP(hipStreamSynchronize(s.stream));
  // ---- 5. download ---------------------------------------------------------------------------------------------------
  ENS_HIP(hipMemcpy(stats, dst, nS * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (stats_nominal) ENS_HIP(hipMemcpy(stats_nominal, dsn, Tn * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (K_lqr) ENS_HIP(hipMemcpy(K_lqr, dK, Tn * (size_t)(N - 1) * 18 * 8, hipMemcpyDeviceToHost));
  if (X_sim) ENS_HIP(hipMemcpy(X_sim, dXS, nXS * 8, hipMemcpyDeviceToHost));
  if (dClip) ENS_HIP(hipMemcpy(disp->n_clipped, dClip, nS * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (dXH) ENS_HIP(hipMemcpy(filt->X_hat, dXH, nS * N * 7 * 8, hipMemcpyDeviceToHost));
  if (dFF) ENS_HIP(hipMemcpy(filt->filt_final, dFF, nS * filt->final_w() * 8, hipMemcpyDeviceToHost));
  ensemble_summary(T, M, stats, summary);
  if (const char* v = std::getenv("TSAT_ENSEMBLE_TIMING")) {   // diagnostic (tools/ensemble_timing.py): HIP-event times of the two kernels
    if (v[0] == '1') {
      float g = 0, e = 0;
      (void)hipEventElapsedTime(&g, s.ev[0], s.ev[1]);
      (void)hipEventElapsedTime(&e, s.ev[1], s.ev[2]);
      if (disp) {
        float p = 0;
        (void)hipEventElapsedTime(&p, s.ev[3], s.ev[0]);
        std::fprintf(stderr, "%s: pack_kernel_ms %.4f gains_kernel_ms %.4f ensemble_kernel_ms %.4f\n", name, p, g, e);
      } else {
        std::fprintf(stderr, "tsat_tvlqr_ensemble: gains_kernel_ms %.4f ensemble_kernel_ms %.4f\n", g, e);
      }
    }
  }
#undef ENS_HIP
  return 0;
}

// tsat_pd_ensemble: steps 2, 4 and 5 of run_ensemble around the kernels of tsat_kernels_pd.hip; `sens` != nullptr is
// tsat_pd_ensemble_sensed, `filt` != nullptr (with it) tsat_pd_ensemble_filtered
int run_pd(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
           const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau, const double* dt,
           const double* Jmat, const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode, const double* x0_sim,
           const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots, const double* plant, const double* sat_lo,
           const double* sat_hi, tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim,
           int32_t* n_clipped, const double* Rtab, double gm, const Sensing* sens = nullptr, const Filtering* filt = nullptr) {
  g_err.clear();
  if (!h) return efail(-1, "null handle or options");
  const std::string why = check_pd(o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode,
                                   x0_sim, x0_nom, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, Rtab, gm);
  if (!why.empty()) return efail(-1, why);
  if (sens) {
    const std::string bad = check_sensor(sens->s, sens->sensor, T, M);
    if (!bad.empty()) return efail(-1, bad);
  }
  if (filt) {
    const std::string bad = filt->check();
    if (!bad.empty()) return efail(-1, bad);
  }
#define ENS_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return efail(-10, std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)
  ENS_HIP(hipSetDevice(tsat_handle_device(h)));
  const int N = o->n_knots, n_tab = o->n_tab;
  const size_t Tn = (size_t)T;
  // ---- 2. upload: the plan only when the call tracks one --------------------------------------------------------------
  const int nw = ensemble_waves(M), Mp = nw * WAVE;
  const size_t nX = Tn * N * 7, nU = Tn * (size_t)(N - 1) * 3, nB = (size_t)n_btab * n_tab, nXU = Tn * N * XUW, nS = Tn * (size_t)M,
               nXS = X_sim ? nS * N * 7 : 0;
  std::vector<double> P(Tn * PSTRIDE), x0n(Tn * 7), zero(Tn * 6, 0.0), gain(Tn * PDGW), model;
  const std::vector<double> sat = pack_limits(sat_lo, sat_hi, T);
  std::vector<int> bi(Tn);
  for (size_t t = 0; t < Tn; ++t) {
    bi[t] = btab_idx ? btab_idx[t] : (int)t;
    for (int i = 0; i < 7; ++i) x0n[7 * t + i] = x0_nom ? x0_nom[7 * t + i] : (X ? X[t * N * 7 + i] : xf[7 * t + i]);
    for (int c = 0; c < 3; ++c) {
      gain[PDGW * t + c] = kd[3 * t + c];
      gain[PDGW * t + 3 + c] = kp[3 * t + c];
    }
  }
  pack_tv_params<double>(T, x0n.data(), xf, tau0, dtau, dt, Jmat, zero.data(), zero.data(), zero.data(), P.data());
  if (!plant) {
    model = model_plants(Jmat, Tn, M);
    plant = model.data();
  }
  EnsScope s;
  double *dP = nullptr, *dX = nullptr, *dU = nullptr, *dB = nullptr, *dBT = nullptr, *dXU = nullptr, *dX0 = nullptr, *dX0N = nullptr,
         *dXS = nullptr, *dGain = nullptr, *dPlant = nullptr, *dPL = nullptr, *dSat = nullptr, *dR = nullptr, *dGT = nullptr;
  int *dbi = nullptr, *dnk = nullptr, *dClip = nullptr;
  long long* dnid = nullptr;
  tsat_tvlqr_stats *dst = nullptr, *dsn = nullptr;
  bool ok = s.alloc(&dP, P.size()) && s.alloc(&dB, nB * 3) && s.alloc(&dBT, nB * 4) && s.alloc(&dX0, nS * 7) && s.alloc(&dX0N, Tn * 7) &&
            s.alloc(&dbi, Tn) && s.alloc(&dst, nS) && s.alloc(&dsn, Tn) && s.alloc(&dGain, gain.size()) &&
            s.alloc(&dPlant, nS * TSAT_PLANT_W) && s.alloc(&dPL, Tn * PLW * (size_t)Mp) && s.alloc(&dSat, sat.size());
  if (ok && X) ok = s.alloc(&dX, nX) && s.alloc(&dU, nU) && s.alloc(&dXU, nXU);
  if (ok && n_knots) ok = s.alloc(&dnk, Tn);
  if (ok && noise_id0) ok = s.alloc(&dnid, Tn);
  if (ok && X_sim) ok = s.alloc(&dXS, nXS);
  if (ok && n_clipped) ok = s.alloc(&dClip, nS);
  if (ok && Rtab) ok = s.alloc(&dR, nB * 3) && (dGT = tsat_ws_gravity(h, nB * 4 * 8)) != nullptr;
  double *dSens = nullptr, *dSN = nullptr;
  if (ok && sens) ok = s.alloc(&dSN, Tn * SNW * (size_t)Mp) && (!sens->sensor || s.alloc(&dSens, nS * SNW));
  // the filtered call: what the law saw and the filter's last state, when asked for
  double *dXH = nullptr, *dFF = nullptr;
  if (ok && filt && filt->X_hat) ok = s.alloc(&dXH, nS * N * 7);
  if (ok && filt && filt->filt_final) ok = s.alloc(&dFF, nS * filt->final_w());
  if (!ok) return efail(-10, "device allocation failed in tsat_pd_ensemble");
  ENS_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : s.ev) ENS_HIP(hipEventCreate(&e));
  ENS_HIP(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dB, Btab, nB * 3 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dX0, x0_sim, nS * 7 * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dX0N, x0n.data(), x0n.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dbi, bi.data(), Tn * sizeof(int), hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dGain, gain.data(), gain.size() * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dPlant, plant, nS * TSAT_PLANT_W * 8, hipMemcpyHostToDevice));
  ENS_HIP(hipMemcpy(dSat, sat.data(), sat.size() * 8, hipMemcpyHostToDevice));
  if (n_knots) ENS_HIP(hipMemcpy(dnk, n_knots, Tn * sizeof(int), hipMemcpyHostToDevice));
  if (noise_id0) ENS_HIP(hipMemcpy(dnid, noise_id0, Tn * sizeof(long long), hipMemcpyHostToDevice));
  if (X) {
    ENS_HIP(hipMemcpy(dX, X, nX * 8, hipMemcpyHostToDevice));
    if (feedforward) ENS_HIP(hipMemcpy(dU, U, nU * 8, hipMemcpyHostToDevice));
    else ENS_HIP(hipMemset(dU, 0, nU * 8));                  // U is not read without feed-forward: the records carry zeros
    const int64_t n_rec = T * (int64_t)N;
    hipLaunchKernelGGL(tsat_ensemble_pack_xu_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s.stream, n_rec, N, dX, dU, dXU);
  }
  hipLaunchKernelGGL(tsat_ensemble_pack_bt_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, s.stream, (int64_t)nB, dB, dBT);
  ENS_HIP(hipGetLastError());
  if (n_knots && X_sim) ENS_HIP(hipMemsetAsync(dXS, 0, nXS * 8, s.stream));   // ragged: zero beyond a slew's own horizon
  {
    const int64_t n = T * (int64_t)(M + 1);
    hipLaunchKernelGGL(tsat_dispersed_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, dPlant, dP, o->u_scale, dPL,
                       T, M, Mp);
    ENS_HIP(hipGetLastError());
  }
  if (Rtab) {
    ENS_HIP(hipMemcpy(dR, Rtab, nB * 3 * 8, hipMemcpyHostToDevice));
    ENS_HIP(tsat_launch_gg_pack(dR, gm, dGT, (int64_t)nB, s.stream));
  }
  if (sens) {
    if (sens->sensor) ENS_HIP(hipMemcpy(dSens, sens->sensor, nS * SNW * 8, hipMemcpyHostToDevice));
    ENS_HIP(tsat_launch_sensed_pack(dSens, dSN, T, M, Mp, s.stream));
  }
  if (dXH) ENS_HIP(hipMemsetAsync(dXH, 0, nS * N * 7 * 8, s.stream));   // the last row of every horizon and all beyond it stay zero
  // ---- 4. the roll-out ------------------------------------------------------------------------------------------------
  ENS_HIP(hipEventRecord(s.ev[0], s.stream));
  {
    PdArgs<double> pa;
    EnsArgs<double>& a = pa.d.e;
    a.T = (int)T; a.N = N; a.n_tab = n_tab; a.M = M; a.us = o->u_scale;
    fill_ens_options(*o, a);
    a.P = dP; a.BT = dBT; a.bidx = dbi; a.nk = dnk; a.XUR = dXU; a.KD = nullptr; a.X0 = dX0;
    a.nid0 = dnid;
    a.XS = dXS; a.stats = dst; a.stats_nom = dsn;
    pa.d.PL = dPL; pa.d.Mp = Mp; pa.d.SAT = dSat; pa.d.nclip = dClip;
    pa.GT = dGT; pa.GAIN = dGain; pa.X0N = dX0N; pa.feedforward = feedforward; pa.limit_mode = limit_mode;
    if (filt && filt->mf) {
      ModelFilteredPdArgs<double> fa;
      fa.p = pa;
      fa.f = model_filt_args(*filt, sens_args(*sens, o, dSN, Mp), a, dXH, dFF);
      ENS_HIP(tsat_launch_model_filtered_pd(fa, nw, s.stream));
    } else if (filt) {
      FilteredPdArgs<double> fa;
      fa.p = pa;
      fa.f = filt_args(*filt, sens_args(*sens, o, dSN, Mp), a, dXH, dFF);
      ENS_HIP(tsat_launch_filtered_pd(fa, nw, s.stream));
    } else if (sens) {
      SensedPdArgs<double> sa;
      sa.p = pa;
      sa.s = sens_args(*sens, o, dSN, Mp);
      ENS_HIP(tsat_launch_sensed_pd(sa, nw, s.stream));
    } else {
      ENS_HIP(tsat_launch_pd(pa, nw, s.stream));
    }
  }
  ENS_HIP(hipEventRecord(s.ev[1], s.stream));
  ENS_HIP(hipStreamSynchronize(s.stream));
  // ---- 5. download ----------------------------------------------------------------------------------------------------
  ENS_HIP(hipMemcpy(stats, dst, nS * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (stats_nominal) ENS_HIP(hipMemcpy(stats_nominal, dsn, Tn * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (X_sim) ENS_HIP(hipMemcpy(X_sim, dXS, nXS * 8, hipMemcpyDeviceToHost));
  if (dClip) ENS_HIP(hipMemcpy(n_clipped, dClip, nS * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (dXH) ENS_HIP(hipMemcpy(filt->X_hat, dXH, nS * N * 7 * 8, hipMemcpyDeviceToHost));
  if (dFF) ENS_HIP(hipMemcpy(filt->filt_final, dFF, nS * filt->final_w() * 8, hipMemcpyDeviceToHost));
  ensemble_summary(T, M, stats, summary);
  if (const char* v = std::getenv("TSAT_ENSEMBLE_TIMING")) {   // diagnostic (tools/pd_timing.py): HIP-event time of the roll-out
    if (v[0] == '1') {
      float e = 0;
      (void)hipEventElapsedTime(&e, s.ev[0], s.ev[1]);
      std::fprintf(stderr, "%s: pd_kernel_ms %.4f\n", filt ? (filt->mf ? "tsat_pd_ensemble_model_filtered" : "tsat_pd_ensemble_filtered") : (sens ? "tsat_pd_ensemble_sensed" : "tsat_pd_ensemble"), e);
    }
  }
#undef ENS_HIP
  return 0;
}

}  // namespace

extern "C" {

int tsat_pd_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                     const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                     const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                     int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                     const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats, double* summary,
                     tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm) {
  return run_pd(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom,
                noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm);
}

int tsat_pd_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                            const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                            const double* dtau, const double* dt, const double* Jmat, const double* kd, const double* kp,
                            int32_t feedforward, int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int64_t* noise_id0,
                            const int32_t* n_knots, const double* plant, const double* sat_lo, const double* sat_hi,
                            tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal, double* X_sim, int32_t* n_clipped,
                            const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor) {
  const Sensing se{sn, sensor};
  return run_pd(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom,
                noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, &se);
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
  const Sensing se{sn, sensor};
  const Filtering fl{f, X_hat, filt_final};
  return run_pd(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom,
                noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, &se,
                f ? &fl : nullptr);
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
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, f};
  return run_pd(h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, kd, kp, feedforward, limit_mode, x0_sim, x0_nom,
                noise_id0, n_knots, plant, sat_lo, sat_hi, stats, summary, stats_nominal, X_sim, n_clipped, Rtab, gm, &se,
                f ? &fl : nullptr);
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
  return run_ensemble("tsat_tvlqr_ensemble", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim,
                      noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, nullptr);
}

int tsat_tvlqr_ensemble_dispersed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                                  const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                                  const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                  const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                                  const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                                  double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim,
                                  int32_t* n_clipped) {
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  return run_ensemble("tsat_tvlqr_ensemble_dispersed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd,
                      x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, &d);
}

int tsat_tvlqr_ensemble_gg(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                           const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                           const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                           const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                           const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                           double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                           const double* Rtab, double gm) {
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  return run_ensemble("tsat_tvlqr_ensemble_gg", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim,
                      noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, &d, &g);
}

int tsat_tvlqr_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X,
                               const double* U, const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                               const double* dtau, const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                               const double* Rd, const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                               const double* plant, const double* sat_lo, const double* sat_hi, tsat_tvlqr_stats* stats,
                               double* summary, tsat_tvlqr_stats* stats_nominal, double* K_lqr, double* X_sim, int32_t* n_clipped,
                               const double* Rtab, double gm, const tsat_sensor_options* sn, const double* sensor) {
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  return run_ensemble("tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd,
                      x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, &d, &g, &se);
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
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{f, X_hat, filt_final};
  return run_ensemble(f ? "tsat_tvlqr_ensemble_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx, tau0,
                      dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, &d, &g, &se,
                      f ? &fl : nullptr);
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
  const Dispersion d{plant, sat_lo, sat_hi, n_clipped};
  const Gravity g{Rtab, gm};
  const Sensing se{sn, sensor};
  const Filtering fl{nullptr, X_hat, filt_final, f};
  return run_ensemble(f ? "tsat_tvlqr_ensemble_model_filtered" : "tsat_tvlqr_ensemble_sensed", h, o, T, n_btab, M, X, U, xf, Btab, btab_idx,
                      tau0, dtau, dt, Jmat, Qd, Qfd, Rd, x0_sim, noise_id0, n_knots, stats, summary, stats_nominal, K_lqr, X_sim, &d, &g,
                      &se, f ? &fl : nullptr);
}

}  // extern "C"
