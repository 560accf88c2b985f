// tsat_kernels.hip — gfx950 kernels + the C ABI of include/tortoise_hip.h (libtortoise_hip.so).
//
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared tsat_kernels.hip -o libtortoise_hip.so
// One wavefront (a 64-thread workgroup) owns one trajectory for the whole AL-iLQR solve; see tsat_device.hpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed on first use (tsat_comm_*), never linked
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "tsat_host_pack.hpp"
#include "tsat_mpc_held.hpp"
#include "tsat_gg.hpp"
#include "tsat_mpc_sensed.hpp"
#include "tsat_mpc_filtered.hpp"
#include "tsat_mpc_model_filtered.hpp"
#include "tsat_mpc_model_mag_filtered.hpp"

using namespace tsat;

// every build of the solve kernel but the wide one lives in a translation unit of its own (tsat_kernels_dense.hip,
// tsat_kernels_packed*.hip, ..._mixed.hip: options.precision = 32); the list of builds is TSAT_SOLVE_BUILDS (tsat_device.hpp)
using solve_launch_t = hipError_t (*)(const KArgs<double>& a, int rk4, int inertia_class, int error_state, hipStream_t stream);
#define TSAT_SOLVE_PROTO(id, layout, tail)                                                                                   \
  hipError_t tsat_launch_solve_##layout##tail(const KArgs<double>&, int, int, int, hipStream_t);                             \
  hipError_t tsat_launch_solve_##layout##_mixed##tail(const KArgs<double>&, int, int, int, hipStream_t);
TSAT_SOLVE_BUILDS(TSAT_SOLVE_PROTO)
#undef TSAT_SOLVE_PROTO

// the plant step of tsat_mpc_run_dispersed (tsat_kernels_mpc_dispersed.hip); step 0 also packs the call's plant records
hipError_t tsat_launch_mpc_dispersed(const MpcDispArgs<double>& a, const double* plant, hipStream_t stream);
// the pack, the hold, and the plan shift that follows whichever hold ran, of tsat_mpc_run_held (tsat_kernels_mpc_held.hip)
hipError_t tsat_launch_mpc_held_pack(const MpcHeldArgs<double>& a, const double* plant, hipStream_t stream);
hipError_t tsat_launch_mpc_held(const MpcHeldArgs<double>& a, int error_state, hipStream_t stream);
hipError_t tsat_launch_mpc_held_shift(const MpcArgs<double>& m, int r, hipStream_t stream);
// the pack of the orbit table and the hold under gravity-gradient torque of tsat_mpc_run_held_gg (tsat_kernels_gg.hip)
hipError_t tsat_launch_gg_pack(const double* R, double gm, double* GT, int64_t rows, hipStream_t stream);
hipError_t tsat_launch_mpc_held_gg(const MpcHeldGgArgs<double>& a, int error_state, hipStream_t stream);
// the pack (bias records, first measurement) and the hold commanding from measurements of tsat_mpc_run_held_sensed
// (tsat_kernels_mpc_sensed.hip)
hipError_t tsat_launch_mpc_sensed_pack(const MpcSensedArgs<double>& a, const double* sensor, hipStream_t stream);
hipError_t tsat_launch_mpc_sensed(const MpcSensedArgs<double>& a, int error_state, hipStream_t stream);
// the pack (that of the sensed loop, then the first estimate) and the hold commanding from the filter's estimate of
// tsat_mpc_run_held_filtered (tsat_kernels_mpc_filtered.hip)
hipError_t tsat_launch_mpc_filtered_pack(const MpcFilteredArgs<double>& a, const double* sensor, int given, hipStream_t stream);
hipError_t tsat_launch_mpc_filtered(const MpcFilteredArgs<double>& a, int error_state, hipStream_t stream);
// tsat_mpc_run_held_model_filtered (tsat_kernels_mpc_model_filtered.hip)
hipError_t tsat_launch_mpc_model_filtered_pack(const MpcModelFilteredArgs<double>& a, const double* sensor, int given, hipStream_t stream);
hipError_t tsat_launch_mpc_model_filtered(const MpcModelFilteredArgs<double>& a, int error_state, hipStream_t stream);
// tsat_mpc_run_held_model_mag_filtered (tsat_kernels_mpc_model_mag_filtered.hip)
hipError_t tsat_launch_mpc_model_mag_filtered_pack(const MpcModelMagFilteredArgs<double>& a, const double* sensor, int given, hipStream_t stream);
hipError_t tsat_launch_mpc_model_mag_filtered(const MpcModelMagFilteredArgs<double>& a, int error_state, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
template <typename real, int INTEG, int DIAGJ, int ES>
__global__ __launch_bounds__(64) void tsat_solve_kernel(KArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  solve_trajectory<real, INTEG, DIAGJ, ES>(a, traj);
}

template <typename real, int DIAGJ>
__global__ __launch_bounds__(64) void tsat_tvlqr_kernel(TvArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  tvlqr_trajectory<real, DIAGJ>(a, traj);
}

template <typename real, int DIAGJ>
__global__ __launch_bounds__(64) void tsat_mpc_advance_kernel(MpcArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  mpc_advance_trajectory<real, DIAGJ>(a, traj);
}

template <typename real>
__global__ __launch_bounds__(64) void tsat_btable_kernel(BtArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  btable_trajectory<real>(a, traj);
}

template <typename real>
__global__ __launch_bounds__(64) void tsat_horizon_kernel(HzArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  horizon_trajectory<real>(a, traj);
}

// resident field tables [T][rows][3] (tsat_btable_batch) -> the solver's padded tables [T][n_tab][4], first n_tab rows
__global__ __launch_bounds__(256) void tsat_pack_tables_kernel(int64_t n, int rows, int n_tab, const double* B, double* BT) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t t = e / n_tab;
  const int r = (int)(e - t * n_tab);
  const double* src = B + ((size_t)t * rows + r) * 3;
  double* dst = BT + (size_t)e * 4;
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = 0.0;
}
template <typename real>
__global__ __launch_bounds__(256) void tsat_export_kernel(int64_t n_rec, int N, const int* nk, const real* XU,
                                                          const real* KD, double* X, double* U, double* K) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_rec) export_record<real>(e, N, nk, XU, KD, X, U, K);
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct tsat_handle {
  int dev = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;
  // reserved batch
  int64_t T = 0, n_btab = 0;
  int N = 0, n_tab = 0, max_ls = 0, trace_rows = 0;
  int slots = 0;              // candidate slabs reserved per trajectory (tsat_batch_reserve): what every launch gets as a.max_ls
  int store_few = N_FEW, store_hold = LS_HOLD;     // keep rule of the one-trajectory builds (tsat_set_store_policy)
  bool uploaded = false, solved = false;
  int inertia_class = 0;      // 0 full, 1 every uploaded inertia tensor diagonal, 2 every one isotropic -> DIAGJ variant
  double *P = nullptr, *BT = nullptr, *U0 = nullptr, *XU = nullptr, *KD = nullptr, *LAM = nullptr, *CAND = nullptr;
  int* bidx = nullptr;
  int* nk = nullptr;          // per-trajectory knot counts (ragged batch) or null
  bool ragged = false;
  tsat_stats* stats = nullptr;
  double* trace = nullptr;
  int64_t bytes = 0;
  int endgame = -1;           // packed builds: park the last trajectories for a one-per-wavefront launch; -1 automatic, 0 never, n: at n live
  int variant = 0;            // solve-kernel build: 0 automatic (dense above 1024 trajectories), 1 wide, 2 dense
  // host copies of the small per-trajectory inputs of the last upload (26 doubles each), for tsat_tvlqr_resident
  std::vector<double> hx0, hxf, htau0, hdtau, hdt, hJ;
  int64_t bt_T = 0;      // field tables left on the device by the last tsat_btable_batch: [bt_T][bt_rows][3] in slot WS_BT_B
  int bt_rows = 0;
  int64_t bt_gen = 0;    // bumped by every tsat_btable_batch call that touches the resident tables (tsat_btable_generation)
  // grow-only device workspaces of the stages around the solve (tracking, horizon, field tables, MPC history, export):
  // allocated on first use and kept for the life of the handle, so repeated calls pay no hipMalloc / hipFree
  enum { WS_TV_NZ, WS_TV_KD, WS_TV_XS, WS_TV_NID, WS_TV_ST, WS_TV_P, WS_TVB_P, WS_TVB_BT, WS_TVB_XUR, WS_TVB_BI, WS_TVB_NK,
         WS_HZ_B, WS_HZ_DT, WS_HZ_CUT, WS_HZ_C, WS_HZ_I, WS_BT_COEF, WS_BT_KEP, WS_BT_T0, WS_BT_TF, WS_BT_POS, WS_BT_B,
         WS_JW, WS_MPC_HX, WS_MPC_HU,
         WS_DL_X, WS_DL_U, WS_DL_K, WS_AG_X, WS_AG_U, WS_AG_ST, WS_AG_XA, WS_AG_UA, WS_AG_STA,   // staging: WS_DL_X .. WS_AG_STA (tsat_workspace_trim)
         WS_AG_CHK, WS_MPC_TALLY, WS_ENDGAME,
         WS_MPCD_PLANT, WS_MPCD_PL, WS_MPCD_SAT, WS_MPCD_NID, WS_MPCD_REC, WS_MPCD_ST, WS_MPCD_CLIP,   // tsat_mpc_run_dispersed
         WS_GG_GT,             // packed gravity rows of tsat_tvlqr_ensemble_gg / tsat_mpc_run_held_gg
         WS_MPCS_XT, WS_MPCS_SN, WS_MPCS_IN, WS_MPCS_Y,   // tsat_mpc_run_held_sensed: true state + last measurement [14][T], biases
                               // [9][T], the uploaded sensor array, Y_hist
         WS_MPCF_FL,           // tsat_mpc_run_held_filtered: the filter's records [31][T]
         WS_MPCMF_FL,          // tsat_mpc_run_held_model_filtered and _model_mag_filtered: the nine-state filter's records [58][T]
         WS_MPCMM_HB,          // tsat_mpc_run_held_model_mag_filtered: the last field sample [3][T]
         WS_SUN_ST,            // packed sun rows of the model-mag-sun-filtered ensembles
         WS_COUNT };
  void* ws[WS_COUNT] = {};
  size_t ws_bytes[WS_COUNT] = {};
  // RCCL communicator of the sweep (tsat_comm_init): one rank per handle / GPU
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  int64_t comm_T = -1; int comm_N = -1;
  int64_t mpc_tally_T = 0;   // trajectories covered by the tally of the last tsat_mpc_run (slot WS_MPC_TALLY)   // shard shape every rank of the communicator was last found to agree on
};

namespace {

int fail(tsat_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}
#define TSAT_HIP(h, call)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail((h), -10, std::string(#call) + ": " + hipGetErrorString(e_));                \
  } while (0)

void release(tsat_handle* h) {
  void* ptrs[] = {h->P, h->BT, h->U0, h->XU, h->KD, h->LAM, h->CAND, h->bidx, h->nk, h->stats, h->trace};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  h->P = h->BT = h->U0 = h->XU = h->KD = h->LAM = h->CAND = nullptr;
  h->bidx = nullptr; h->nk = nullptr; h->ragged = false; h->stats = nullptr; h->trace = nullptr;
  h->T = 0; h->bytes = 0; h->uploaded = h->solved = false;
}

// workspace `slot` with room for `bytes` (grow-only; contents are not preserved across a growth); nullptr on failure
void* ws_get(tsat_handle* h, int slot, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (h->ws[slot] && h->ws_bytes[slot] >= bytes) return h->ws[slot];
  if (h->ws[slot]) { (void)hipFree(h->ws[slot]); h->ws[slot] = nullptr; h->ws_bytes[slot] = 0; }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  h->ws[slot] = p;
  h->ws_bytes[slot] = bytes;
  return p;
}
void ws_release(tsat_handle* h) {
  for (int i = 0; i < tsat_handle::WS_COUNT; ++i)
    if (h->ws[i]) { (void)hipFree(h->ws[i]); h->ws[i] = nullptr; h->ws_bytes[i] = 0; }
}

template <typename Tp>
int dev_alloc(tsat_handle* h, Tp** p, size_t n) {
  const size_t b = n * sizeof(Tp);
  TSAT_HIP(h, hipMalloc(reinterpret_cast<void**>(p), b ? b : 16));
  h->bytes += (int64_t)b;
  return 0;
}

}  // namespace

// the packed gravity rows of the gravity-gradient entry points: the handle's grow-only slot, for the ensemble's translation
// unit too (to which `struct tsat_handle` is opaque); nullptr on failure
double* tsat_ws_gravity(tsat_handle* h, size_t bytes) { return (double*)ws_get(h, tsat_handle::WS_GG_GT, bytes); }
// ... and the packed sun rows of the model-mag-sun-filtered ensembles, likewise
double* tsat_ws_sun(tsat_handle* h, size_t bytes) { return (double*)ws_get(h, tsat_handle::WS_SUN_ST, bytes); }
// the handle's GPU, for an entry point of that unit which makes no call into this one before it allocates (tsat_pd_ensemble)
int tsat_handle_device(const tsat_handle* h) { return h->dev; }

extern "C" {

int tsat_version(void) { return 300; }

void tsat_default_options(tsat_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->integrator = 3; o->precision = 64;
  o->max_outer = 20; o->max_inner = 50;            // src/TortoiseSat.jl:195-196
  o->max_linesearch = 20; o->dj_counter_limit = 10;
  o->cost_tol = 1e-4; o->grad_tol = 1e-5; o->constraint_tol = 1e-3;
  o->penalty_init = 1.0; o->penalty_scale = 10.0; o->penalty_max = 1e8; o->dual_max = 1e8;
  o->reg_init = 0.0; o->reg_scale = 1.6; o->reg_min = 1e-8; o->reg_max = 1e8; o->reg_fp = 10.0;
  o->ls_lower = 1e-8; o->ls_upper = 10.0; o->max_state = 1e8;
  o->u_scale = 1e-2;                               // src/DerivFunction.jl:37
  o->terminal_mask = 0x7f; o->error_state = 0;
}

int tsat_create(tsat_handle** out, int device_id) {
  if (!out) return -1;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -2;  // no GPU: there is no CPU fallback
  if (device_id < 0 || device_id >= n) return -3;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return -4;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return -5;  // code object is gfx950-only
  if (hipSetDevice(device_id) != hipSuccess) return -6;
  tsat_handle* h = new tsat_handle();
  h->dev = device_id;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
    delete h;
    return -7;
  }
  *out = h;
  return 0;
}

int tsat_destroy(tsat_handle* h) {
  if (!h) return -1;
  (void)hipSetDevice(h->dev);
  (void)tsat_comm_destroy(h);
  release(h);
  ws_release(h);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

const char* tsat_last_error(const tsat_handle* h) { return h ? h->err.c_str() : "null handle"; }

int64_t tsat_batch_bytes(const tsat_handle* h) { return h ? h->bytes : 0; }

int64_t tsat_workspace_bytes(const tsat_handle* h) {
  int64_t b = 0;
  if (h)
    for (int i = 0; i < tsat_handle::WS_COUNT; ++i) b += (int64_t)h->ws_bytes[i];
  return b;
}

int tsat_workspace_trim(tsat_handle* h, int32_t what) {
  if (!h) return -1;
  if (what != 0 && what != 1) return fail(h, -1, "what must be 0 (staging buffers of downloads and gathers) or 1 (every workspace)");
  TSAT_HIP(h, hipSetDevice(h->dev));
  TSAT_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < tsat_handle::WS_COUNT; ++i) {
    const bool staging = i >= tsat_handle::WS_DL_X && i <= tsat_handle::WS_AG_STA;
    if (!h->ws[i] || !(what == 1 || staging)) continue;
    (void)hipFree(h->ws[i]);
    h->ws[i] = nullptr; h->ws_bytes[i] = 0;
    if (i == tsat_handle::WS_BT_B) { h->bt_T = 0; h->bt_rows = 0; h->bt_gen++; }     // the resident field tables are gone
  }
  return 0;
}

int64_t tsat_btable_generation(const tsat_handle* h) { return h ? h->bt_gen : 0; }

int tsat_batch_reserve(tsat_handle* h, int64_t T, int32_t n_knots, int32_t n_tab, int64_t n_btab,
                       int32_t max_linesearch) {
  if (!h) return -1;
  if (T < 1 || n_knots < 2 || n_tab < 1 || n_btab < 1) return fail(h, -1, "bad batch dimensions");
  if (max_linesearch < 1 || max_linesearch > TSAT_MAX_LINESEARCH) return fail(h, -1, "max_linesearch must be in [1,32]");
  TSAT_HIP(h, hipSetDevice(h->dev));
  if (h->T == T && h->N == n_knots && h->n_tab == n_tab && h->n_btab == n_btab && h->max_ls == max_linesearch)
    return 0;
  const int trows = h->trace_rows;
  release(h);
  const size_t N = (size_t)n_knots, Tn = (size_t)T;
  int rc = 0;
  rc |= dev_alloc(h, &h->P, Tn * PSTRIDE);
  rc |= dev_alloc(h, &h->BT, (size_t)n_btab * n_tab * 4);
  rc |= dev_alloc(h, &h->bidx, Tn);
  rc |= dev_alloc(h, &h->nk, Tn);
  rc |= dev_alloc(h, &h->U0, Tn * (N - 1) * 3);
  rc |= dev_alloc(h, &h->XU, Tn * N * XUW);
  rc |= dev_alloc(h, &h->KD, Tn * (N - 1) * KDW);
  rc |= dev_alloc(h, &h->LAM, Tn * (N - 1) * LMW);
  // stored candidates (tsat_device.hpp): one slab for every candidate where the automatic choice runs a one-trajectory build, so
  // that no line search repeats a sweep; the large batches of the packed builds (which keep PK_STORE at most) stay at NSTORE
  const int slots = reserved_slots(T, max_linesearch);
  rc |= dev_alloc(h, &h->CAND, Tn * (size_t)slots * N * XUW);
  rc |= dev_alloc(h, &h->stats, Tn);
  if (trows > 0) rc |= dev_alloc(h, &h->trace, Tn * (size_t)trows * 8);
  if (rc) { release(h); return -10; }
  h->T = T; h->N = n_knots; h->n_tab = n_tab; h->n_btab = n_btab; h->max_ls = max_linesearch;
  h->slots = slots;
  h->trace_rows = trows;
  return 0;
}

int tsat_batch_trace(tsat_handle* h, int32_t rows) {
  if (!h || rows < 0) return -1;
  TSAT_HIP(h, hipSetDevice(h->dev));
  if (h->trace) { (void)hipFree(h->trace); h->trace = nullptr; }
  h->trace_rows = rows;
  if (rows > 0 && h->T > 0) {
    if (dev_alloc(h, &h->trace, (size_t)h->T * rows * 8)) return -10;
  }
  return 0;
}

int tsat_batch_upload(tsat_handle* h, const double* x0, const double* xf, const double* Btab,
                      const int32_t* btab_idx, const double* tau0, const double* dtau, const double* dt,
                      const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                      const double* ulo, const double* uhi, const double* U0) {
  if (!h) return -1;
  if (h->T < 1) return fail(h, -1, "tsat_batch_reserve has not been called");
  if (!x0 || !xf || !tau0 || !dtau || !dt || !Jmat || !Qd || !Qfd || !Rd || !ulo || !uhi || !U0)
    return fail(h, -1, "null input array");
  if (!Btab && (h->bt_T != h->T || h->n_btab != h->T || h->n_tab > h->bt_rows))
    return fail(h, -1, "Btab is NULL but the field tables left by the last tsat_btable_batch do not cover this batch "
                       "(need one table per trajectory, n_btab = T, and n_tab <= its 2 n_half rows)");
  if (!btab_idx && h->n_btab != h->T) return fail(h, -1, "btab_idx is NULL but n_btab != T");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const int64_t T = h->T;
  std::vector<int> bi((size_t)T);
  for (int64_t t = 0; t < T; ++t) {
    const int64_t v = btab_idx ? btab_idx[t] : t;
    if (v < 0 || v >= h->n_btab) return fail(h, -1, "btab_idx out of range");
    bi[(size_t)t] = (int)v;
  }
  const std::string bad = check_inputs(T, x0, xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi);
  if (!bad.empty()) return fail(h, -1, bad);
  h->inertia_class = inertia_class(T, Jmat);
  std::vector<double> P((size_t)T * PSTRIDE);
  pack_params<double>(T, x0, xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, P.data());
  TSAT_HIP(h, hipMemcpy(h->P, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));
  if (Btab) {
    std::vector<double> BT((size_t)h->n_btab * h->n_tab * 4);
    pack_btab<double>(h->n_btab, h->n_tab, Btab, BT.data());
    TSAT_HIP(h, hipMemcpy(h->BT, BT.data(), BT.size() * sizeof(double), hipMemcpyHostToDevice));
  } else {   // device to device: the tables tsat_btable_batch left in its workspace, padded to the solver's row layout
    const int64_t n = T * (int64_t)h->n_tab;
    const double* B = (const double*)ws_get(h, tsat_handle::WS_BT_B, (size_t)h->bt_T * h->bt_rows * 3 * 8);
    if (!B) return fail(h, -10, "resident field tables are gone");
    hipLaunchKernelGGL(tsat_pack_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, h->bt_rows, h->n_tab, B, h->BT);
    TSAT_HIP(h, hipGetLastError());
    TSAT_HIP(h, hipStreamSynchronize(h->stream));
  }
  TSAT_HIP(h, hipMemcpy(h->bidx, bi.data(), bi.size() * sizeof(int), hipMemcpyHostToDevice));
  TSAT_HIP(h, hipMemcpy(h->U0, U0, (size_t)T * (h->N - 1) * 3 * sizeof(double), hipMemcpyHostToDevice));
  h->hx0.assign(x0, x0 + 7 * T); h->hxf.assign(xf, xf + 7 * T); h->htau0.assign(tau0, tau0 + T);
  h->hdtau.assign(dtau, dtau + T); h->hdt.assign(dt, dt + T); h->hJ.assign(Jmat, Jmat + 9 * T);
  h->uploaded = true;
  h->solved = false;
  h->ragged = false;   // a fresh upload is a uniform batch until tsat_batch_knots says otherwise
  return 0;
}

int tsat_batch_knots(tsat_handle* h, const int32_t* n_knots) {
  if (!h) return -1;
  if (!h->uploaded) return fail(h, -1, "tsat_batch_upload has not been called");
  if (!n_knots) { h->ragged = false; return 0; }
  for (int64_t t = 0; t < h->T; ++t)
    if (n_knots[t] < 2 || n_knots[t] > h->N) return fail(h, -1, "n_knots[t] must be in [2, N]");
  TSAT_HIP(h, hipSetDevice(h->dev));
  TSAT_HIP(h, hipMemcpy(h->nk, n_knots, (size_t)h->T * sizeof(int), hipMemcpyHostToDevice));
  h->ragged = true;
  h->solved = false;
  return 0;
}

namespace {
using solve_kern_t = void (*)(KArgs<double>);
// kernel variant: integrator x inertia class (full / diagonal / isotropic) x error-state mode. LDS is a static
// module-level array (tsat_device.hpp): nothing dynamic to request at launch.
solve_kern_t solve_variant(const tsat_handle* h, const tsat_options* o) {
  static const solve_kern_t variants[2][3][2] = TSAT_VARIANT_TABLE(tsat_solve_kernel);
  return variants[o->integrator == 4 ? 1 : 0][h->inertia_class][o->error_state ? 1 : 0];
}

// Build by batch size (measured on one MI355X, profiles/r04/build_by_batch_size.txt): one wavefront per SIMD and trajectory (wide
// build) while the batch fits the GPU that way — 256 CUs x 4 SIMDs; two wavefronts per SIMD (dense build) up to twice that; from
// there the packed builds at ONE wavefront per SIMD, whose wavefronts own several trajectories (40 KB of LDS keep twelve of a
// backward pass's sixteen knot records on the chip, all sixteen float ones): four per wavefront up to one round of the 1024 SIMDs
// (packed4w, 2048 .. 4096), eight per wavefront up to one round (packed8w, .. 8192), sixteen from one full round on (packed16w);
// between 8192 and 16384, and from there on with a long iteration budget, eight per wavefront at two wavefronts per SIMD
// (packed8: selected_build). packed (four per wavefront at two per SIMD) is no longer chosen automatically.
constexpr int64_t TSAT_WIDE_MAX_T = 1024;
constexpr int64_t TSAT_PACKED4W_MAX_T = 4096;     // (TSAT_PACKED_MIN_T = 2048: tsat_host_pack.hpp, which sizes the candidate slabs by it)
constexpr int64_t TSAT_PACKED8W_MAX_T = 8192;
constexpr int64_t TSAT_PACKED16W_MIN_T = 16384, TSAT_LONG_BUDGET = 100;     // (budget = max_outer x max_inner)
// the build (1 wide, 2 dense, 3 packed, 4 packed8, 5 packed8w, 6 packed16w, 7 packed4w) that (h->variant, batch size, precision) selects.
// precision = 32 — the mixed-precision builds — has no wide layout: below 2048 trajectories its dense build runs (59-knot Jacobian
// passes in the 20 KB of two wavefronts per SIMD, which the double records do not allow)
int selected_build(const tsat_handle* h, int precision, int64_t budget) {
  if (h->variant >= 3) return h->variant;
  // from one full round on: sixteen per wavefront — unless the iteration budget is long enough to spread the trajectories' iteration
  // counts widely (3 x 50 on the inclination sweep: 30 ... 150), where a wavefront lasts as long as the slowest of its trajectories
  // and eight per wavefront on 2048 wavefront slots lose less (65536 trajectories: 3.91 s against 4.27 s; 5 x 10: 0.47 against 0.43 s)
  if (h->variant == 0 && h->T >= TSAT_PACKED16W_MIN_T) return budget >= TSAT_LONG_BUDGET ? 4 : 6;
  if (h->variant == 0 && h->T > TSAT_PACKED8W_MAX_T) return 4;
  if (h->variant == 0 && h->T > TSAT_PACKED4W_MAX_T) return 5;
  if (h->variant == 0 && h->T >= TSAT_PACKED_MIN_T) return 7;
  if (precision == 32) return 2;
  return (h->variant == 2 || (h->variant != 1 && h->T > TSAT_WIDE_MAX_T)) ? 2 : 1;
}
// at[mixed precision][build id]; null: the wide build, launched from this unit (selected_build never gives it at precision 32)
struct SolveLaunchers {
  solve_launch_t at[2][8] = {};
  constexpr SolveLaunchers() {
#define TSAT_SOLVE_ENTRY(id, layout, tail) at[0][id] = tsat_launch_solve_##layout##tail; at[1][id] = tsat_launch_solve_##layout##_mixed##tail;
    TSAT_SOLVE_BUILDS(TSAT_SOLVE_ENTRY)
#undef TSAT_SOLVE_ENTRY
  }
};
hipError_t launch_solve(const tsat_handle* h, const tsat_options* o, const KArgs<double>& a) {
  static constexpr SolveLaunchers launchers;
  const int build = selected_build(h, o->precision, (int64_t)o->max_outer * o->max_inner), rk4 = o->integrator == 4;
  if (const solve_launch_t launch = launchers.at[o->precision == 32][build]) return launch(a, rk4, h->inertia_class, o->error_state, h->stream);
  hipLaunchKernelGGL(solve_variant(h, o), dim3((unsigned)h->T), dim3(64), 0, h->stream, a);
  return hipGetLastError();
}

// Jacobian-record workspace of the packed builds (one block per wavefront, i.e. per four trajectories at most), persistent in
// the handle; sized for double records, the mixed-precision builds (float records) use half of it
void* packed_workspace(tsat_handle* h) {
  return ws_get(h, tsat_handle::WS_JW, (size_t)((h->T + 3) / 4) * TSAT_JW_REALS_PER_4 * sizeof(double));
}

// does the build that (h->variant, batch size, precision) selects need the packed builds' Jacobian workspace a.JW?
bool uses_packed_build(const tsat_handle* h, int precision) { return selected_build(h, precision, 0) >= 3; }     // (whatever the budget)

// Endgame of a packed launch (tsat_packed.hpp, suspend_if_endgame). Automatic: once an eighth of the batch (profiles/r04/endgame_sweep.txt), at most the 2048
// wavefront slots of the machine (256 CUs x 4 SIMDs x 2), is all that still iterates — and only for iteration budgets long
// enough to spread the trajectories (the 1 x 3 budget of the receding-horizon loop ends all of them together).
// One block for both precisions: two counters, then T ids, then T Resume records (sized for doubles).
struct EndgameArgs { int suspend_at = 0; int *live = nullptr, *susp_n = nullptr, *susp_ids = nullptr; void* susp_state = nullptr; };
int endgame_threshold(const tsat_handle* h, const tsat_options* o) {
  int at = h->endgame;
  if (at < 0) at = ((int64_t)o->max_outer * o->max_inner >= 20) ? (int)std::min<int64_t>(2048, h->T / 8) : 0;
  return at <= 0 ? 0 : (int)std::min<int64_t>(at, h->T);
}
EndgameArgs endgame_args(tsat_handle* h, const tsat_options* o) {
  EndgameArgs a;
  const int at = endgame_threshold(h, o);
  if (at <= 0) return a;
  const size_t T = (size_t)h->T, ids_at = 16, st_at = (ids_at + T * sizeof(int) + 15) / 16 * 16;
  char* w = (char*)ws_get(h, tsat_handle::WS_ENDGAME, st_at + T * sizeof(Resume<double>));
  if (!w) return a;     // no endgame then: the packed kernel runs every trajectory to its end, as before
  a.suspend_at = (int)std::min<int64_t>(at, h->T);
  a.live = (int*)w; a.susp_n = (int*)w + 1; a.susp_ids = (int*)(w + ids_at); a.susp_state = w + st_at;
  return a;
}

KArgs<double> solve_args(tsat_handle* h, const tsat_options* o) {
  KArgs<double> a;
  a.T = (int)h->T; a.N = h->N; a.n_tab = h->n_tab; a.max_ls = h->slots; a.opt = *o;
  a.ls_few = h->store_few; a.ls_hold = h->store_hold;
  a.P = h->P; a.BT = h->BT; a.bidx = h->bidx; a.nk = h->ragged ? h->nk : nullptr; a.U0 = h->U0;
  a.XU = h->XU; a.KD = h->KD; a.LAM = h->LAM; a.CAND = h->CAND;
  a.stats = h->stats; a.trace = h->trace; a.trace_rows = h->trace ? h->trace_rows : 0;
  a.JW = uses_packed_build(h, 64) ? (double*)packed_workspace(h) : nullptr;
  if (a.JW) {
    const EndgameArgs e = endgame_args(h, o);
    a.suspend_at = e.suspend_at; a.live = e.live; a.susp_n = e.susp_n; a.susp_ids = e.susp_ids; a.susp_state = e.susp_state;
  }
  return a;
}

}  // namespace

int tsat_batch_run(tsat_handle* h, const tsat_options* o, float* kernel_ms) {
  if (!h || !o) return -1;
  if (!h->uploaded) return fail(h, -1, "tsat_batch_upload has not been called");
  const std::string why = check_options(*o, h->N, h->n_tab, h->max_ls);
  if (!why.empty()) return fail(h, -1, why);
  TSAT_HIP(h, hipSetDevice(h->dev));
  const KArgs<double> a = solve_args(h, o);
  if (!a.JW && uses_packed_build(h, 64))
    return fail(h, -10, "device allocation of the packed builds' Jacobian workspace failed");
  if (h->trace) TSAT_HIP(h, hipMemsetAsync(h->trace, 0, (size_t)h->T * h->trace_rows * 8 * sizeof(double), h->stream));
  TSAT_HIP(h, hipEventRecord(h->ev0, h->stream));
  TSAT_HIP(h, launch_solve(h, o, a));
  TSAT_HIP(h, hipEventRecord(h->ev1, h->stream));
  TSAT_HIP(h, hipStreamSynchronize(h->stream));
  if (kernel_ms) TSAT_HIP(h, hipEventElapsedTime(kernel_ms, h->ev0, h->ev1));
  h->solved = true;
  return 0;
}

int tsat_set_kernel_variant(tsat_handle* h, int32_t variant) {
  if (!h) return -1;
  if (!(variant >= 0 && variant <= 7))
    return fail(h, -1, "variant must be 0 (automatic), 1 (wide), 2 (dense), 3 (packed: 4 trajectories per wavefront), 4 (packed8), 5 (packed8w: 8, one wavefront per SIMD) or 6 (packed16w) or 7 (packed4w: 4, one wavefront per SIMD)");
  h->variant = variant;
  return 0;
}

int tsat_selected_build(tsat_handle* h, const tsat_options* o, int32_t* build, int32_t* endgame_at) {
  if (!h || !o) return -1;
  if (h->T <= 0) return fail(h, -1, "tsat_batch_reserve has not been called");
  const int b = selected_build(h, o->precision, (int64_t)o->max_outer * o->max_inner);
  if (build) *build = b;
  if (endgame_at) *endgame_at = b >= 3 ? endgame_threshold(h, o) : 0;
  return 0;
}

int tsat_set_endgame(tsat_handle* h, int32_t suspend_at) {
  if (!h) return -1;
  if (suspend_at < -1) return fail(h, -1, "suspend_at must be -1 (automatic), 0 (never) or the live count at which the packed builds park their trajectories");
  h->endgame = suspend_at;
  return 0;
}

int tsat_set_store_policy(tsat_handle* h, int32_t few, int32_t hold) {
  if (!h) return -1;
  const std::string why = check_store_policy(few);
  if (!why.empty()) return fail(h, -1, why);
  h->store_few = few;
  h->store_hold = hold;
  return 0;
}

namespace {
// the end of both receding-horizon loops, once their launches are queued (rc: what queueing them returned): wait, bring the
// history and the last solve's statistics down, refresh the host mirrors of x0 / tau0
int mpc_collect(tsat_handle* h, int rc, const char* name, const double* dHX, const double* dHU, size_t nX, size_t nU, double* X_hist,
                double* U_hist, tsat_stats* stats_last, float* solve_ms) {
  const size_t T = (size_t)h->T;
  if (!rc && (hipEventRecord(h->ev1, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)) rc = -10;
  if (!rc && solve_ms && hipEventElapsedTime(solve_ms, h->ev0, h->ev1) != hipSuccess) rc = -10;
  if (!rc && hipMemcpy(X_hist, dHX, nX * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && hipMemcpy(U_hist, dHU, nU * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && stats_last && hipMemcpy(stats_last, h->stats, T * sizeof(tsat_stats), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  // the loop advanced x0 and tau0 inside the device parameter records: refresh the host mirrors tsat_tvlqr_resident packs
  // its own records from, so that tracking after an MPC run linearises against the field rows the last plan was solved on
  std::vector<double> Pb(T * PSTRIDE);
  if (!rc && hipMemcpy(Pb.data(), h->P, Pb.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (rc) { h->solved = false; return fail(h, rc, std::string("launch or copy failed in ") + name); }
  for (size_t t = 0; t < T; ++t) {
    for (int i = 0; i < 7; ++i) h->hx0[7 * t + i] = Pb[t * PSTRIDE + P_X0 + i];
    h->htau0[t] = Pb[t * PSTRIDE + P_TAU0];
  }
  h->solved = true;
  return 0;
}
}  // namespace

int tsat_mpc_run(tsat_handle* h, const tsat_options* o, int32_t n_steps, int32_t plant_integrator, double* X_hist,
                 double* U_hist, tsat_stats* stats_last, float* solve_ms) {
  if (!h || !o) return -1;
  if (!h->uploaded) return fail(h, -1, "tsat_batch_upload has not been called");
  const std::string why = check_options(*o, h->N, h->n_tab, h->max_ls);
  if (!why.empty()) return fail(h, -1, why);
  if (n_steps < 1) return fail(h, -1, "n_steps must be >= 1");
  if (o->precision != 64) return fail(h, -1, "tsat_mpc_run runs the fp64 build only (precision must be 64)");
  if (plant_integrator != 3 && plant_integrator != 4) return fail(h, -1, "plant_integrator must be 3 (rk3) or 4 (rk4)");
  if (!X_hist || !U_hist) return fail(h, -1, "null array");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const size_t T = (size_t)h->T, nX = T * ((size_t)n_steps + 1) * 7, nU = T * (size_t)n_steps * 3;
  double* dHX = (double*)ws_get(h, tsat_handle::WS_MPC_HX, nX * 8);
  double* dHU = (double*)ws_get(h, tsat_handle::WS_MPC_HU, nU * 8);
  long long* dTally = (long long*)ws_get(h, tsat_handle::WS_MPC_TALLY, T * 4 * sizeof(long long));
  if (!dHX || !dHU || !dTally) return fail(h, -10, "device allocation failed in tsat_mpc_run");
  TSAT_HIP(h, hipMemsetAsync(dTally, 0, T * 4 * sizeof(long long), h->stream));
  h->mpc_tally_T = (int64_t)T;
  const KArgs<double> a = solve_args(h, o);
  if (!a.JW && uses_packed_build(h, 64))     // a packed kernel launched with JW = nullptr would fault on the device
    return fail(h, -10, "device allocation of the packed builds' Jacobian workspace failed");
  MpcArgs<double> m;
  m.T = (int)h->T; m.N = h->N; m.n_tab = h->n_tab; m.plant_integ = plant_integrator; m.n_steps = n_steps; m.us = o->u_scale;
  m.P = h->P; m.BT = h->BT; m.bidx = h->bidx; m.nk = h->ragged ? h->nk : nullptr; m.XU = h->XU; m.U0 = h->U0;
  m.HX = dHX; m.HU = dHU; m.stats = h->stats; m.tally = dTally;
  auto adv = h->inertia_class == 2 ? tsat_mpc_advance_kernel<double, 2>
                                   : (h->inertia_class == 1 ? tsat_mpc_advance_kernel<double, 1> : tsat_mpc_advance_kernel<double, 0>);
  int rc = 0;
  if (hipEventRecord(h->ev0, h->stream) != hipSuccess) rc = -10;
  for (int s = 0; s < n_steps && !rc; ++s) {   // 2 n_steps launches queued back to back; the stream orders them
    if (launch_solve(h, o, a) != hipSuccess) rc = -10;
    m.step = s;
    hipLaunchKernelGGL(adv, dim3((unsigned)h->T), dim3(64), 0, h->stream, m);
    if (hipGetLastError() != hipSuccess) rc = -10;
  }
  return mpc_collect(h, rc, "tsat_mpc_run", dHX, dHU, nX, nU, X_hist, U_hist, stats_last, solve_ms);
}

int tsat_mpc_tally(tsat_handle* h, int64_t* tally) {
  if (!h || !tally) return -1;
  if (h->mpc_tally_T != h->T || h->T < 1 || !h->ws[tsat_handle::WS_MPC_TALLY]) return fail(h, -1, "tsat_mpc_run has not been called on this batch");
  TSAT_HIP(h, hipSetDevice(h->dev));
  static_assert(sizeof(long long) == sizeof(int64_t), "tally element");
  TSAT_HIP(h, hipMemcpy(tally, h->ws[tsat_handle::WS_MPC_TALLY], (size_t)h->T * 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return 0;
}

namespace {
// the loop of tsat_mpc_run_dispersed (replan_every = 0: a solve and the one-wavefront-per-trajectory step kernel per control step)
// and of tsat_mpc_run_held (replan_every >= 1: a solve, the lane-per-trajectory hold and the plan shift per block); with
// `gravity` the hold is the one of tsat_mpc_run_held_gg (Rtab [n_btab][n_tab][3] of the resident batch, gm); with `sc` the hold of
// tsat_mpc_run_held_sensed, which reads measurements (tsat_mpc_sensed.hpp) — through the gravity rows when `gravity`; with `fc`
// besides, the hold of tsat_mpc_run_held_filtered, which reads the filter's estimates (tsat_mpc_filtered.hpp); with `mc` besides
// `sc`, the hold of tsat_mpc_run_held_model_filtered, which reads the nine-state filter's (tsat_mpc_model_filtered.hpp); with `gc`
// besides `sc`, the hold of tsat_mpc_run_held_model_mag_filtered, which reads that filter's updated by the magnetometer
// (tsat_mpc_model_mag_filtered.hpp): the parent's record, and the field's one-sample memory beside it
struct SensedCall {
  const tsat_sensor_options* s;
  const double* sensor;      // 9 x T or null
  double* Y_hist;            // 7 x n_steps x T or null
};
struct FilteredCall {
  const tsat_filter_options* f;
  const double* filt_init;   // 31 x T or null
  double* filt_state;        // 31 x T or null
  double* filt_final;        // 9 x T or null
};
struct ModelFilteredCall {
  const tsat_model_filter_options* f;
  const double* filt_init;   // 58 x T or null
  double* filt_state;        // 58 x T or null
  double* filt_final;        // 12 x T or null
};
struct ModelMagFilteredCall {
  const tsat_model_mag_filter_options* f;
  const double* filt_init;   // 58 x T or null
  double* filt_state;        // 58 x T or null
  double* filt_final;        // 12 x T or null
};
int mpc_plant_loop(tsat_handle* h, const char* name, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps,
                   int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                   const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last,
                   tsat_tvlqr_stats* stats, int32_t* n_clipped, float* solve_ms, bool gravity = false, const double* Rtab = nullptr,
                   double gm = 0.0, const SensedCall* sc = nullptr, const FilteredCall* fc = nullptr,
                   const ModelFilteredCall* mc = nullptr, const ModelMagFilteredCall* gc = nullptr) {
  if (!h || !o || !po) return -1;
  const bool held = replan_every != 0;
  if (!h->uploaded) return fail(h, -1, "tsat_batch_upload has not been called");
  const std::string why = check_options(*o, h->N, h->n_tab, h->max_ls);
  if (!why.empty()) return fail(h, -1, why);
  if (o->precision != 64) return fail(h, -1, std::string(name) + " runs the fp64 build only (precision must be 64)");
  const std::string bad = check_mpc_dispersed(*po, n_steps, step0, plant, sat_lo, sat_hi, h->T);
  if (!bad.empty()) return fail(h, -1, bad);
  const size_t n_rows = (size_t)h->n_btab * (size_t)h->n_tab;
  if (gravity) {
    const std::string badg = check_gravity(Rtab, gm, (int64_t)n_rows);
    if (!badg.empty()) return fail(h, -1, badg);
  }
  if (sc) {
    const std::string bads = check_mpc_sensed(sc->s, sc->sensor, h->T, Rtab, gm);
    if (!bads.empty()) return fail(h, -1, bads);
  }
  if (fc) {
    const std::string badf = check_mpc_filtered(fc->f, fc->filt_init, fc->filt_state, fc->filt_final, h->T);
    if (!badf.empty()) return fail(h, -1, badf);
  }
  if (mc) {
    const std::string badm = check_mpc_model_filtered(mc->f, mc->filt_init, mc->filt_state, mc->filt_final, h->T);
    if (!badm.empty()) return fail(h, -1, badm);
  }
  if (gc) {
    const std::string badg = check_mpc_model_mag_filtered(gc->f, gc->filt_init, gc->filt_state, gc->filt_final, h->T);
    if (!badg.empty()) return fail(h, -1, badg);
  }
  // the nine-state record is one: whichever of the two filters the call flies
  const double* nine_init = mc ? mc->filt_init : (gc ? gc->filt_init : nullptr);
  double* nine_state = mc ? mc->filt_state : (gc ? gc->filt_state : nullptr);
  double* nine_final = mc ? mc->filt_final : (gc ? gc->filt_final : nullptr);
  if (!X_hist || !U_hist) return fail(h, -1, "null array");
  TSAT_HIP(h, hipSetDevice(h->dev));
  if (held) {
    int min_nk = h->N;
    if (h->ragged) {
      std::vector<int> nk((size_t)h->T);
      TSAT_HIP(h, hipMemcpy(nk.data(), h->nk, nk.size() * sizeof(int), hipMemcpyDeviceToHost));
      min_nk = *std::min_element(nk.begin(), nk.end());
    }
    const std::string hold = check_mpc_held(replan_every, feedback, min_nk);
    if (!hold.empty()) return fail(h, -1, hold);
  }
  const size_t T = (size_t)h->T, nX = T * ((size_t)n_steps + 1) * 7, nU = T * (size_t)n_steps * 3;
  double* dHX = (double*)ws_get(h, tsat_handle::WS_MPC_HX, nX * 8);
  double* dHU = (double*)ws_get(h, tsat_handle::WS_MPC_HU, nU * 8);
  long long* dTally = (long long*)ws_get(h, tsat_handle::WS_MPC_TALLY, T * 4 * sizeof(long long));
  double* dPlant = plant ? (double*)ws_get(h, tsat_handle::WS_MPCD_PLANT, T * TSAT_PLANT_W * 8) : nullptr;
  double* dPL = (double*)ws_get(h, tsat_handle::WS_MPCD_PL, T * (held ? HELD_W : PLW) * 8);
  double* dSat = (double*)ws_get(h, tsat_handle::WS_MPCD_SAT, T * SATW * 8);
  long long* dNid = noise_id ? (long long*)ws_get(h, tsat_handle::WS_MPCD_NID, T * sizeof(long long)) : nullptr;
  MpcDispRec* dRec = (MpcDispRec*)ws_get(h, tsat_handle::WS_MPCD_REC, T * sizeof(MpcDispRec));
  tsat_tvlqr_stats* dSt = (tsat_tvlqr_stats*)ws_get(h, tsat_handle::WS_MPCD_ST, T * sizeof(tsat_tvlqr_stats));
  int* dClip = (int*)ws_get(h, tsat_handle::WS_MPCD_CLIP, T * sizeof(int));
  double *dXT = nullptr, *dSN = nullptr, *dSIn = nullptr, *dY = nullptr;
  if (sc) {
    dXT = (double*)ws_get(h, tsat_handle::WS_MPCS_XT, T * MSX_W * 8);
    dSN = (double*)ws_get(h, tsat_handle::WS_MPCS_SN, T * SNW * 8);
    dSIn = sc->sensor ? (double*)ws_get(h, tsat_handle::WS_MPCS_IN, T * SNW * 8) : nullptr;
    dY = (double*)ws_get(h, tsat_handle::WS_MPCS_Y, nU / 3 * 7 * 8);
    if (!dXT || !dSN || (sc->sensor && !dSIn) || !dY) return fail(h, -10, std::string("device allocation failed in ") + name);
  }
  double* dFL = fc ? (double*)ws_get(h, tsat_handle::WS_MPCF_FL, T * FLW * 8) : nullptr;
  if (fc && !dFL) return fail(h, -10, std::string("device allocation failed in ") + name);
  double* dMFL = (mc || gc) ? (double*)ws_get(h, tsat_handle::WS_MPCMF_FL, T * MFLW * 8) : nullptr;
  if ((mc || gc) && !dMFL) return fail(h, -10, std::string("device allocation failed in ") + name);
  double* dHB = gc ? (double*)ws_get(h, tsat_handle::WS_MPCMM_HB, T * 3 * 8) : nullptr;
  if (gc && !dHB) return fail(h, -10, std::string("device allocation failed in ") + name);
  // the gravity call: the packed rows are the handle's, the raw orbit table lives until the pack has run
  double* dGT = gravity ? tsat_ws_gravity(h, n_rows * 4 * 8) : nullptr;
  struct Raw {
    double* p = nullptr;
    ~Raw() { if (p) (void)hipFree(p); }
  } dR;
  if (gravity && (!dGT || hipMalloc((void**)&dR.p, n_rows * 3 * 8) != hipSuccess))
    return fail(h, -10, std::string("device allocation failed in ") + name);
  if (!dHX || !dHU || !dTally || (plant && !dPlant) || !dPL || !dSat || (noise_id && !dNid) || !dRec || !dSt || !dClip)
    return fail(h, -10, std::string("device allocation failed in ") + name);
  const std::vector<double> sat = pack_limits(sat_lo, sat_hi, (int64_t)T);
  TSAT_HIP(h, hipMemcpy(dSat, sat.data(), sat.size() * 8, hipMemcpyHostToDevice));
  if (plant) TSAT_HIP(h, hipMemcpy(dPlant, plant, T * TSAT_PLANT_W * 8, hipMemcpyHostToDevice));
  if (noise_id) TSAT_HIP(h, hipMemcpy(dNid, noise_id, T * sizeof(long long), hipMemcpyHostToDevice));
  if (gravity) TSAT_HIP(h, hipMemcpy(dR.p, Rtab, n_rows * 3 * 8, hipMemcpyHostToDevice));
  if (dSIn) TSAT_HIP(h, hipMemcpy(dSIn, sc->sensor, T * SNW * 8, hipMemcpyHostToDevice));
  std::vector<double> flh(fc ? T * FLW : 0);   // the filter's records, component-major as the device holds them
  if (fc && fc->filt_init) {
    filt_records_pack(fc->filt_init, flh.data(), (int64_t)T);
    TSAT_HIP(h, hipMemcpy(dFL, flh.data(), flh.size() * 8, hipMemcpyHostToDevice));
  }
  std::vector<double> mflh((mc || gc) ? T * MFLW : 0);   // the nine-state filter's records, likewise
  if (nine_init) {
    model_filt_records_pack(nine_init, mflh.data(), (int64_t)T);
    TSAT_HIP(h, hipMemcpy(dMFL, mflh.data(), mflh.size() * 8, hipMemcpyHostToDevice));
  }
  TSAT_HIP(h, hipMemsetAsync(dTally, 0, T * 4 * sizeof(long long), h->stream));
  h->mpc_tally_T = (int64_t)T;
  const KArgs<double> a = solve_args(h, o);
  if (!a.JW && uses_packed_build(h, 64))     // a packed kernel launched with JW = nullptr would fault on the device
    return fail(h, -10, "device allocation of the packed builds' Jacobian workspace failed");
  MpcHeldArgs<double> mh = {};
  MpcDispArgs<double>& md = mh.s;
  MpcArgs<double>& m = md.m;
  m.T = (int)h->T; m.N = h->N; m.n_tab = h->n_tab; m.plant_integ = 4; m.n_steps = n_steps; m.us = o->u_scale;
  m.P = h->P; m.BT = h->BT; m.bidx = h->bidx; m.nk = h->ragged ? h->nk : nullptr; m.XU = h->XU; m.U0 = h->U0;
  m.HX = dHX; m.HU = dHU; m.stats = h->stats; m.tally = dTally;
  md.d.PL = dPL; md.d.Mp = 1; md.d.SAT = dSat; md.d.nclip = dClip;
  EnsArgs<double>& e = md.d.e;
  fill_ens_options(*po, e);
  e.nid0 = dNid; e.stats = dSt;
  md.noisy = po->noise_mode; md.step0 = (long long)step0; md.rec = dRec;
  mh.KD = h->KD; mh.feedback = feedback;
  MpcHeldGgArgs<double> mg = {};
  MpcSensedArgs<double> ms = {};
  if (sc) {
    ms.GT = gravity ? dGT : nullptr; ms.XT = dXT; ms.HY = dY;
    ms.s.SN = dSN; ms.s.Mp = (int)T; ms.s.sgy = sc->s->sigma_gyro; ms.s.sat = sc->s->sigma_att; ms.s.smg = sc->s->sigma_mag;
    ms.s.latency = sc->s->latency; ms.s.k0 = e.k0; ms.s.k1 = e.k1;
  }
  MpcFilteredArgs<double> mf = {};
  if (fc) {
    mf.FL = dFL;
    mf.f.s = ms.s; mf.f.P = h->P; mf.f.nk = m.nk; mf.f.M = 1; mf.f.N = h->N;
    mf.f.sv = fc->f->sigma_v; mf.f.su = fc->f->sigma_u; mf.f.sa = fc->f->sigma_a; mf.f.p0a = fc->f->p0_att; mf.f.p0b = fc->f->p0_bias;
  }
  MpcModelFilteredArgs<double> mm = {};
  if (mc) {
    mm.FL = dMFL;
    mm.f.s = ms.s; mm.f.P = h->P; mm.f.M = 1; mm.f.N = h->N; mm.f.n_tab = h->n_tab; mm.f.us = o->u_scale;
    mm.f.sv = mc->f->sigma_v; mm.f.sw = mc->f->sigma_w; mm.f.su = mc->f->sigma_u; mm.f.sa = mc->f->sigma_a; mm.f.sg = mc->f->sigma_g;
    mm.f.p0a = mc->f->p0_att; mm.f.p0b = mc->f->p0_bias;
  }
  MpcModelMagFilteredArgs<double> mg9 = {};
  if (gc) {
    ModelFiltArgs<double>& g = mg9.f.m;
    mg9.FL = dMFL; mg9.HB = dHB; mg9.f.sm = gc->f->sigma_m;
    g.s = ms.s; g.P = h->P; g.M = 1; g.N = h->N; g.n_tab = h->n_tab; g.us = o->u_scale;
    g.sv = gc->f->sigma_v; g.sw = gc->f->sigma_w; g.su = gc->f->sigma_u; g.sa = 0.0; g.sg = gc->f->sigma_g;
    g.p0a = gc->f->p0_att; g.p0b = gc->f->p0_bias;
  }
  int rc = 0;
  if (hipEventRecord(h->ev0, h->stream) != hipSuccess) rc = -10;
  if (held) {   // the pack, then solve, hold and shift per block queued back to back; the stream orders them
    if (tsat_launch_mpc_held_pack(mh, dPlant, h->stream) != hipSuccess) rc = -10;
    if (!rc && gravity && tsat_launch_gg_pack(dR.p, gm, dGT, (int64_t)n_rows, h->stream) != hipSuccess) rc = -10;
    if (sc) {   // biases, the true state to its own record, the first measurement into the record the solve reads
      ms.h = mh;
      if (fc) {
        mf.ms = ms;
        if (!rc && tsat_launch_mpc_filtered_pack(mf, dSIn, fc->filt_init != nullptr, h->stream) != hipSuccess) rc = -10;
      } else if (mc) {
        mm.ms = ms;
        if (!rc && tsat_launch_mpc_model_filtered_pack(mm, dSIn, mc->filt_init != nullptr, h->stream) != hipSuccess) rc = -10;
      } else if (gc) {
        mg9.ms = ms;
        if (!rc && tsat_launch_mpc_model_mag_filtered_pack(mg9, dSIn, gc->filt_init != nullptr, h->stream) != hipSuccess) rc = -10;
      } else {
        if (!rc && tsat_launch_mpc_sensed_pack(ms, dSIn, h->stream) != hipSuccess) rc = -10;
      }
    }
    for (int s = 0; s < n_steps && !rc; s += replan_every) {
      if (launch_solve(h, o, a) != hipSuccess) rc = -10;
      m.step = s;
      mh.r = std::min<int>(replan_every, n_steps - s);
      if (fc) {        // the hold on the filter's estimates (with or without the gravity rows)
        ms.h = mh; mf.ms = ms;
        if (!rc && tsat_launch_mpc_filtered(mf, o->error_state, h->stream) != hipSuccess) rc = -10;
      } else if (mc) { // the hold on the nine-state filter's estimates (with or without the gravity rows)
        ms.h = mh; mm.ms = ms;
        if (!rc && tsat_launch_mpc_model_filtered(mm, o->error_state, h->stream) != hipSuccess) rc = -10;
      } else if (gc) { // the hold on the magnetometer-updated nine-state filter's estimates (likewise)
        ms.h = mh; mg9.ms = ms;
        if (!rc && tsat_launch_mpc_model_mag_filtered(mg9, o->error_state, h->stream) != hipSuccess) rc = -10;
      } else if (sc) {        // the hold on measurements (with or without the gravity rows)
        ms.h = mh;
        if (!rc && tsat_launch_mpc_sensed(ms, o->error_state, h->stream) != hipSuccess) rc = -10;
      } else if (gravity) {   // the hold through the gravity rows
        mg.h = mh; mg.GT = dGT;
        if (!rc && tsat_launch_mpc_held_gg(mg, o->error_state, h->stream) != hipSuccess) rc = -10;
      } else {
        if (!rc && tsat_launch_mpc_held(mh, o->error_state, h->stream) != hipSuccess) rc = -10;
      }
      if (!rc && tsat_launch_mpc_held_shift(m, mh.r, h->stream) != hipSuccess) rc = -10;
    }
  } else {
    for (int s = 0; s < n_steps && !rc; ++s) {   // 2 n_steps launches (+ the pack) queued back to back; the stream orders them
      if (launch_solve(h, o, a) != hipSuccess) rc = -10;
      m.step = s;
      if (!rc && tsat_launch_mpc_dispersed(md, dPlant, h->stream) != hipSuccess) rc = -10;
    }
  }
  rc = mpc_collect(h, rc, name, dHX, dHU, nX, nU, X_hist, U_hist, stats_last, solve_ms);
  if (rc) return rc;
  if (stats) TSAT_HIP(h, hipMemcpy(stats, dSt, T * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost));
  if (n_clipped) TSAT_HIP(h, hipMemcpy(n_clipped, dClip, T * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (sc && sc->Y_hist) TSAT_HIP(h, hipMemcpy(sc->Y_hist, dY, nU / 3 * 7 * 8, hipMemcpyDeviceToHost));
  if (fc && (fc->filt_state || fc->filt_final)) {
    TSAT_HIP(h, hipMemcpy(flh.data(), dFL, flh.size() * 8, hipMemcpyDeviceToHost));
    filt_records_unpack(flh.data(), (int64_t)T, fc->filt_state, fc->filt_final);
  }
  if (nine_state || nine_final) {
    TSAT_HIP(h, hipMemcpy(mflh.data(), dMFL, mflh.size() * 8, hipMemcpyDeviceToHost));
    model_filt_records_unpack(mflh.data(), (int64_t)T, nine_state, nine_final);
  }
  return 0;
}
}  // namespace

int tsat_mpc_run_dispersed(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                           const double* plant, const double* sat_lo, const double* sat_hi, const int64_t* noise_id,
                           double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped,
                           float* solve_ms) {
  return mpc_plant_loop(h, "tsat_mpc_run_dispersed", o, po, n_steps, step0, 0, 0, plant, sat_lo, sat_hi, noise_id, X_hist, U_hist,
                        stats_last, stats, n_clipped, solve_ms);
}

int tsat_mpc_run_held(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                      int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                      const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                      int32_t* n_clipped, float* solve_ms) {
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  return mpc_plant_loop(h, "tsat_mpc_run_held", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id, X_hist,
                        U_hist, stats_last, stats, n_clipped, solve_ms);
}

int tsat_mpc_run_held_gg(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                         int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                         const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                         int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm) {
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  return mpc_plant_loop(h, "tsat_mpc_run_held_gg", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id,
                        X_hist, U_hist, stats_last, stats, n_clipped, solve_ms, true, Rtab, gm);
}

int tsat_mpc_run_held_sensed(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                             int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                             const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                             int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm, const tsat_sensor_options* s,
                             const double* sensor, double* Y_hist) {
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  const SensedCall sc = {s, sensor, Y_hist};
  return mpc_plant_loop(h, "tsat_mpc_run_held_sensed", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id,
                        X_hist, U_hist, stats_last, stats, n_clipped, solve_ms, Rtab != nullptr, Rtab, gm, &sc);
}

int tsat_mpc_run_held_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                               int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                               const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                               int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm, const tsat_sensor_options* s,
                               const double* sensor, double* Y_hist, const tsat_filter_options* f, const double* filt_init,
                               double* filt_state, double* filt_final) {
  if (!f) {   // the sensed call itself
    const std::string bad = check_mpc_filtered(f, filt_init, filt_state, filt_final, 0);
    if (!bad.empty()) return fail(h, -1, bad);
    return tsat_mpc_run_held_sensed(h, o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id, X_hist, U_hist,
                                    stats_last, stats, n_clipped, solve_ms, Rtab, gm, s, sensor, Y_hist);
  }
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  const SensedCall sc = {s, sensor, Y_hist};
  const FilteredCall fc = {f, filt_init, filt_state, filt_final};
  return mpc_plant_loop(h, "tsat_mpc_run_held_filtered", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id,
                        X_hist, U_hist, stats_last, stats, n_clipped, solve_ms, Rtab != nullptr, Rtab, gm, &sc, &fc);
}

int tsat_mpc_run_held_model_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                                     int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                                     const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist,
                                     tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped, float* solve_ms,
                                     const double* Rtab, double gm, const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                                     const tsat_model_filter_options* f, const double* filt_init, double* filt_state,
                                     double* filt_final) {
  if (!f) {   // the sensed call itself
    const std::string bad = check_mpc_model_filtered(f, filt_init, filt_state, filt_final, 0);
    if (!bad.empty()) return fail(h, -1, bad);
    return tsat_mpc_run_held_sensed(h, o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id, X_hist, U_hist,
                                    stats_last, stats, n_clipped, solve_ms, Rtab, gm, s, sensor, Y_hist);
  }
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  const SensedCall sc = {s, sensor, Y_hist};
  const ModelFilteredCall mc = {f, filt_init, filt_state, filt_final};
  return mpc_plant_loop(h, "tsat_mpc_run_held_model_filtered", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi,
                        noise_id, X_hist, U_hist, stats_last, stats, n_clipped, solve_ms, Rtab != nullptr, Rtab, gm, &sc, nullptr, &mc);
}

int tsat_mpc_run_held_model_mag_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps,
                                         int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                                         const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist,
                                         tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped, float* solve_ms,
                                         const double* Rtab, double gm, const tsat_sensor_options* s, const double* sensor,
                                         double* Y_hist, const tsat_model_mag_filter_options* f, const double* filt_init,
                                         double* filt_state, double* filt_final) {
  if (!f) {   // the sensed call itself
    const std::string bad = check_mpc_model_mag_filtered(f, filt_init, filt_state, filt_final, 0);
    if (!bad.empty()) return fail(h, -1, bad);
    return tsat_mpc_run_held_sensed(h, o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi, noise_id, X_hist, U_hist,
                                    stats_last, stats, n_clipped, solve_ms, Rtab, gm, s, sensor, Y_hist);
  }
  if (replan_every < 1) return fail(h, -1, check_mpc_held(replan_every, feedback, 2));
  const SensedCall sc = {s, sensor, Y_hist};
  const ModelMagFilteredCall gc = {f, filt_init, filt_state, filt_final};
  return mpc_plant_loop(h, "tsat_mpc_run_held_model_mag_filtered", o, po, n_steps, step0, replan_every, feedback, plant, sat_lo, sat_hi,
                        noise_id, X_hist, U_hist, stats_last, stats, n_clipped, solve_ms, Rtab != nullptr, Rtab, gm, &sc, nullptr, nullptr,
                        &gc);
}

int tsat_batch_export_device(tsat_handle* h, void* X_dev, void* U_dev, void* K_dev, void* stats_dev) {
  if (!h) return -1;
  if (!h->solved) return fail(h, -1, "tsat_batch_run has not been called");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const int64_t n_rec = h->T * (int64_t)h->N;
  if (X_dev || U_dev || K_dev) {
    const unsigned blocks = (unsigned)((n_rec + 255) / 256);
    hipLaunchKernelGGL(tsat_export_kernel<double>, dim3(blocks), dim3(256), 0, h->stream, n_rec, h->N,
                       h->ragged ? h->nk : nullptr, h->XU, h->KD,
                       (double*)X_dev, (double*)U_dev, (double*)K_dev);
    TSAT_HIP(h, hipGetLastError());
  }
  if (stats_dev)
    TSAT_HIP(h, hipMemcpyAsync(stats_dev, h->stats, (size_t)h->T * sizeof(tsat_stats), hipMemcpyDeviceToDevice, h->stream));
  TSAT_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int tsat_batch_download(tsat_handle* h, double* X, double* U, double* K, tsat_stats* stats) {
  if (!h) return -1;
  if (!h->solved) return fail(h, -1, "tsat_batch_run has not been called");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const size_t T = (size_t)h->T, N = (size_t)h->N;
  double *dX = nullptr, *dU = nullptr, *dK = nullptr;
  int rc = 0;
  if (X && !(dX = (double*)ws_get(h, tsat_handle::WS_DL_X, T * N * 7 * sizeof(double)))) rc = -10;
  if (!rc && U && !(dU = (double*)ws_get(h, tsat_handle::WS_DL_U, T * (N - 1) * 3 * sizeof(double)))) rc = -10;
  if (!rc && K && !(dK = (double*)ws_get(h, tsat_handle::WS_DL_K, T * (N - 1) * 21 * sizeof(double)))) rc = -10;
  if (!rc) rc = tsat_batch_export_device(h, dX, dU, dK, nullptr);
  if (!rc && X && hipMemcpy(X, dX, T * N * 7 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && U && hipMemcpy(U, dU, T * (N - 1) * 3 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && K && hipMemcpy(K, dK, T * (N - 1) * 21 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && stats && hipMemcpy(stats, h->stats, T * sizeof(tsat_stats), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (rc == -10) h->err = "device allocation or copy failed in tsat_batch_download";
  return rc;
}

int tsat_batch_trace_download(tsat_handle* h, double* trace) {
  if (!h || !trace) return -1;
  if (!h->trace) return fail(h, -1, "tracing is disabled");
  TSAT_HIP(h, hipSetDevice(h->dev));
  TSAT_HIP(h, hipMemcpy(trace, h->trace, (size_t)h->T * h->trace_rows * 8 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int tsat_solve_batch(tsat_handle* h, const tsat_options* o, int64_t T, int64_t n_btab, const double* x0,
                     const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0,
                     const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                     const double* Qfd, const double* Rd, const double* ulo, const double* uhi, const double* U0,
                     double* X, double* U, double* K, tsat_stats* stats) {
  if (!h || !o) return -1;
  int rc = tsat_batch_reserve(h, T, o->n_knots, o->n_tab, n_btab, o->max_linesearch);
  if (rc) return rc;
  rc = tsat_batch_upload(h, x0, xf, Btab, btab_idx, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, U0);
  if (rc) return rc;
  rc = tsat_batch_run(h, o, nullptr);
  if (rc) return rc;
  return tsat_batch_download(h, X, U, K, stats);
}

void tsat_tvlqr_default_options(tsat_tvlqr_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->linearize_dt_sq = 1;   // `dt = S[end]^2`, src/attitude_controller.jl:137
  o->min_steps = 10; o->u_scale = 1e-2; o->w_tol = 0.05; o->angle_tol = 0.08727;   // src/monte_carlo.jl:70-71,251
  tv_noise_defaults(*o);
}

namespace {
// launch + read-back shared by tsat_tvlqr_batch (everything uploaded for the call) and tsat_tvlqr_resident (reference
// records, tables and knot counts are the resident solved batch)
int run_tvlqr(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int N, int n_tab, int cls, const double* dP,
              const double* dBT, const int* dbi, const int* dnk, const double* dXUR, const double* noise,
              const int64_t* noise_id, double* X_sim, double* U_sim, double* K_lqr, tsat_tvlqr_stats* stats) {
  const size_t Tn = (size_t)T;
  const size_t nNZ = Tn * (size_t)(N - 1) * 36, nKD = Tn * (size_t)(N - 1) * KDW, nXS = Tn * N * XUW;
  double *dNZ = nullptr, *dKD = nullptr, *dXS = nullptr;
  long long* dnid = nullptr;
  tsat_tvlqr_stats* dst = nullptr;
  int rc = 0;
  auto A = [&](void** p, int slot, size_t bytes) { if (!rc && !(*p = ws_get(h, slot, bytes))) rc = -10; };
  auto C = [&](void* d, const void* s, size_t bytes) { if (!rc && hipMemcpy(d, s, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -10; };
  if (noise) { A((void**)&dNZ, tsat_handle::WS_TV_NZ, nNZ * 8); C(dNZ, noise, nNZ * 8); }
  A((void**)&dKD, tsat_handle::WS_TV_KD, nKD * 8); A((void**)&dXS, tsat_handle::WS_TV_XS, nXS * 8);
  A((void**)&dst, tsat_handle::WS_TV_ST, Tn * sizeof(tsat_tvlqr_stats));
  if ((o->noise_mode == 1 || o->rate_as_written) && noise_id) { A((void**)&dnid, tsat_handle::WS_TV_NID, Tn * sizeof(long long)); C(dnid, noise_id, Tn * sizeof(long long)); }
  // ragged batch: the slabs beyond a trajectory's own horizon stay zero
  if (dnk && !rc && (hipMemsetAsync(dKD, 0, nKD * 8, h->stream) != hipSuccess || hipMemsetAsync(dXS, 0, nXS * 8, h->stream) != hipSuccess)) rc = -10;
  if (!rc) {
    TvArgs<double> a;
    a.T = (int)T; a.N = N; a.n_tab = n_tab; a.lin_sq = o->linearize_dt_sq; a.min_steps = o->min_steps;
    a.us = o->u_scale; a.w_tol = o->w_tol; a.ang_tol = o->angle_tol;
    fill_tv_noise<double>(*o, dnid, a);
    a.P = dP; a.BT = dBT; a.bidx = dbi; a.nk = dnk; a.XUR = dXUR; a.NZ = dNZ; a.KD = dKD; a.XS = dXS; a.stats = dst;
    auto kern = cls == 2 ? tsat_tvlqr_kernel<double, 2> : (cls == 1 ? tsat_tvlqr_kernel<double, 1> : tsat_tvlqr_kernel<double, 0>);
    hipLaunchKernelGGL(kern, dim3((unsigned)T), dim3(64), 0, h->stream, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) rc = -10;
  }
  const bool want_traj = X_sim || U_sim || K_lqr;       // the statistic alone travels when no trajectory is asked for
  std::vector<double> XS(want_traj ? nXS : 0), KD(K_lqr ? nKD : 0);     // the gains travel only when asked for
  if (!rc && want_traj && hipMemcpy(XS.data(), dXS, nXS * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && K_lqr && hipMemcpy(KD.data(), dKD, nKD * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && hipMemcpy(stats, dst, Tn * sizeof(tsat_tvlqr_stats), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && want_traj) unpack_tv<double>(T, N, XS.data(), KD.data(), X_sim, U_sim, K_lqr);
  return rc;
}
}  // namespace

int tsat_tvlqr_batch(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, const double* X,
                     const double* U, const double* xf, const double* Btab, const int32_t* btab_idx,
                     const double* tau0, const double* dtau, const double* dt, const double* Jmat, const double* Qd,
                     const double* Qfd, const double* Rd, const double* x0_sim, const double* noise, double* X_sim,
                     double* U_sim, double* K_lqr, tsat_tvlqr_stats* stats, const int32_t* n_knots, const int64_t* noise_id) {
  if (!h || !o) return -1;
  const std::string why = check_tv_options(*o);
  if (!why.empty()) return fail(h, -1, why);
  if (T < 1 || n_btab < 1) return fail(h, -1, "bad batch dimensions");
  if (!X || !U || !xf || !Btab || !tau0 || !dtau || !dt || !Jmat || !Qd || !Qfd || !Rd || !x0_sim || !stats)
    return fail(h, -1, "null array");
  if (!btab_idx && n_btab != T) return fail(h, -1, "btab_idx is NULL but n_btab != T");
  if (o->noise_mode == 1 && noise) return fail(h, -1, "noise_mode = 1 draws the noise in the kernel: pass noise = NULL");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const int N = o->n_knots, n_tab = o->n_tab;
  const size_t Tn = (size_t)T;
  std::vector<int> bi(Tn);
  for (int64_t t = 0; t < T; ++t) {
    const int64_t v = btab_idx ? btab_idx[t] : t;
    if (v < 0 || v >= n_btab) return fail(h, -1, "btab_idx out of range");
    if (!(dt[t] > 0.0)) return fail(h, -1, "dt must be positive");
    if (n_knots && (n_knots[t] < 2 || n_knots[t] > N)) return fail(h, -1, "n_knots[t] must be in [2, N]");
    bi[(size_t)t] = (int)v;
  }
  std::vector<double> P(Tn * PSTRIDE), BT((size_t)n_btab * n_tab * 4), XUR(Tn * N * XUW);
  pack_tv_params<double>(T, x0_sim, xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, P.data());
  pack_btab<double>(n_btab, n_tab, Btab, BT.data());
  pack_xu_records<double>(T, N, X, U, XUR.data());
  double *dP = nullptr, *dBT = nullptr, *dXUR = nullptr;
  int *dbi = nullptr, *dnk = nullptr;
  int rc = 0;
  auto A = [&](void** p, int slot, size_t bytes) { if (!rc && !(*p = ws_get(h, slot, bytes))) rc = -10; };
  auto C = [&](void* d, const void* s, size_t bytes) { if (!rc && hipMemcpy(d, s, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -10; };
  A((void**)&dP, tsat_handle::WS_TVB_P, P.size() * 8); A((void**)&dBT, tsat_handle::WS_TVB_BT, BT.size() * 8);
  A((void**)&dXUR, tsat_handle::WS_TVB_XUR, XUR.size() * 8); A((void**)&dbi, tsat_handle::WS_TVB_BI, Tn * sizeof(int));
  C(dP, P.data(), P.size() * 8); C(dBT, BT.data(), BT.size() * 8); C(dXUR, XUR.data(), XUR.size() * 8); C(dbi, bi.data(), Tn * sizeof(int));
  if (n_knots) { A((void**)&dnk, tsat_handle::WS_TVB_NK, Tn * sizeof(int)); C(dnk, n_knots, Tn * sizeof(int)); }
  if (!rc) rc = run_tvlqr(h, o, T, N, n_tab, inertia_class(T, Jmat), dP, dBT, dbi, dnk, dXUR, noise, noise_id, X_sim, U_sim, K_lqr, stats);
  if (rc) h->err = "device allocation, copy or launch failed in tsat_tvlqr_batch";
  return rc;
}

int tsat_tvlqr_resident(tsat_handle* h, const tsat_tvlqr_options* o, const double* Qd, const double* Qfd, const double* Rd,
                        const double* x0_sim, const double* noise, double* X_sim, double* U_sim, double* K_lqr,
                        tsat_tvlqr_stats* stats, const int64_t* noise_id) {
  if (!h || !o) return -1;
  if (!h->solved) return fail(h, -1, "tsat_batch_run has not been called");
  tsat_tvlqr_options oo = *o;
  oo.n_knots = h->N; oo.n_tab = h->n_tab;
  const std::string why = check_tv_options(oo);
  if (!why.empty()) return fail(h, -1, why);
  if (!Qd || !Qfd || !Rd || !x0_sim || !stats) return fail(h, -1, "null array");
  if (oo.noise_mode == 1 && noise) return fail(h, -1, "noise_mode = 1 draws the noise in the kernel: pass noise = NULL");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const int64_t T = h->T;
  std::vector<double> P((size_t)T * PSTRIDE);
  pack_tv_params<double>(T, x0_sim, h->hxf.data(), h->htau0.data(), h->hdtau.data(), h->hdt.data(), h->hJ.data(), Qd, Qfd, Rd, P.data());
  double* dP = (double*)ws_get(h, tsat_handle::WS_TV_P, P.size() * 8);
  if (!dP) return fail(h, -10, "device allocation failed in tsat_tvlqr_resident");
  int rc = hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : -10;
  const double* dXUR = h->XU;
  if (!rc) rc = run_tvlqr(h, &oo, T, h->N, h->n_tab, h->inertia_class, dP, h->BT, h->bidx, h->ragged ? h->nk : nullptr, dXUR,
                          noise, noise_id, X_sim, U_sim, K_lqr, stats);
  if (rc) h->err = "device allocation, copy or launch failed in tsat_tvlqr_resident";
  return rc;
}

int tsat_horizon_batch(tsat_handle* h, int64_t T, int32_t n_rows, const double* Btab, const double* dt_row,
                       const double* cutoff, int32_t* tf_index, double* cond_at) {
  if (!h) return -1;
  if (T < 1 || n_rows < 1) return fail(h, -1, "bad dimensions");
  if (!dt_row || !cutoff || !tf_index) return fail(h, -1, "null array");
  if (!Btab && (h->bt_T != T || h->bt_rows != n_rows))
    return fail(h, -1, "Btab is NULL but the field tables left by the last tsat_btable_batch are not T x n_rows");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const size_t Tn = (size_t)T, nB = Tn * (size_t)n_rows * 3;
  double *dB = nullptr, *ddt = nullptr, *dcut = nullptr, *dc = nullptr;
  int* di = nullptr;
  int rc = 0;
  auto A = [&](void** p, int slot, size_t bytes) { if (!rc && !(*p = ws_get(h, slot, bytes))) rc = -10; };
  if (Btab) A((void**)&dB, tsat_handle::WS_HZ_B, nB * 8);
  else dB = (double*)ws_get(h, tsat_handle::WS_BT_B, nB * 8);       // same size as allocated: the resident tables themselves
  A((void**)&ddt, tsat_handle::WS_HZ_DT, Tn * 8); A((void**)&dcut, tsat_handle::WS_HZ_CUT, Tn * 8);
  A((void**)&dc, tsat_handle::WS_HZ_C, Tn * 8); A((void**)&di, tsat_handle::WS_HZ_I, Tn * sizeof(int));
  auto Cp = [&](void* d, const void* s, size_t bytes) { if (!rc && hipMemcpy(d, s, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -10; };
  if (Btab) Cp(dB, Btab, nB * 8);
  Cp(ddt, dt_row, Tn * 8); Cp(dcut, cutoff, Tn * 8);
  if (!rc) {
    HzArgs<double> a;
    a.T = (int)T; a.n_rows = n_rows; a.BT = dB; a.dt_row = ddt; a.cutoff = dcut; a.tf_index = di; a.cond_at = dc;
    hipLaunchKernelGGL(tsat_horizon_kernel<double>, dim3((unsigned)T), dim3(64), 0, h->stream, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) rc = -10;
  }
  if (!rc && hipMemcpy(tf_index, di, Tn * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && cond_at && hipMemcpy(cond_at, dc, Tn * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (rc) h->err = "device allocation, copy or launch failed in tsat_horizon_batch";
  return rc;
}

// ------------------------------------------------------------------------------------------------
// Sweep exchange: the RCCL all-gather of every rank's converged trajectories (north_star). RCCL is loaded on
// first use — a single-GPU host never needs it — and called on the handle's own stream right behind the export kernel.
// ------------------------------------------------------------------------------------------------
}  // extern "C"
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
};
RcclApi& rccl() {
  static RcclApi api;
  if (api.lib || !api.why.empty()) return api;
  // a host that already carries an RCCL (PyTorch-ROCm bundles one) keeps using that copy; otherwise the system library
  const char* env = std::getenv("TSAT_RCCL_LIB");
  const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names)
    if (n && *n && (api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
  if (!api.lib)
    for (const char* n : names)
      if (n && *n && (api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
  if (!api.lib) { api.why = "librccl.so.1 not found (set TSAT_RCCL_LIB)"; return api; }
  api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
  api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
  api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
  api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather) { api.why = "RCCL symbols missing"; api.lib = nullptr; }
  return api;
}
int rccl_fail(tsat_handle* h, const char* what, ncclResult_t r) {
  RcclApi& a = rccl();
  return fail(h, -11, std::string(what) + ": " + (a.GetErrorString ? a.GetErrorString(r) : "RCCL error"));
}
}  // namespace
extern "C" {

int tsat_comm_available(void) { return rccl().lib ? 0 : -11; }

int tsat_comm_unique_id(void* id_out) {
  if (!id_out) return -1;
  RcclApi& a = rccl();
  if (!a.lib) return -11;
  static_assert(sizeof(ncclUniqueId) == TSAT_COMM_ID_BYTES, "unique-id size");
  ncclUniqueId id;
  if (a.GetUniqueId(&id) != ncclSuccess) return -11;
  std::memcpy(id_out, &id, sizeof(id));
  return 0;
}

int tsat_comm_init(tsat_handle* h, const void* id_in, int32_t rank, int32_t world) {
  if (!h || !id_in) return -1;
  if (world < 1 || rank < 0 || rank >= world) return fail(h, -1, "need 0 <= rank < world");
  RcclApi& a = rccl();
  if (!a.lib) return fail(h, -11, "RCCL unavailable: " + a.why);
  TSAT_HIP(h, hipSetDevice(h->dev));
  (void)tsat_comm_destroy(h);
  ncclUniqueId id;
  std::memcpy(&id, id_in, sizeof(id));
  ncclComm_t c = nullptr;
  const ncclResult_t r = a.CommInitRank(&c, world, id, rank);
  if (r != ncclSuccess) return rccl_fail(h, "ncclCommInitRank", r);
  h->comm = c; h->comm_rank = rank; h->comm_world = world;
  h->comm_T = -1; h->comm_N = -1;
  return 0;
}

int tsat_comm_destroy(tsat_handle* h) {
  if (!h) return -1;
  if (h->comm) {
    (void)hipSetDevice(h->dev);
    (void)hipStreamSynchronize(h->stream);
    (void)rccl().CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr; h->comm_rank = 0; h->comm_world = 1;
    h->comm_T = -1; h->comm_N = -1;
  }
  return 0;
}

int tsat_sweep_allgather(tsat_handle* h, void* X_all, void* U_all, void* stats_all, int32_t on_device) {
  if (!h) return -1;
  if (!h->solved) return fail(h, -1, "tsat_batch_run has not been called");
  if (!h->comm) return fail(h, -1, "tsat_comm_init has not been called");
  TSAT_HIP(h, hipSetDevice(h->dev));
  RcclApi& a = rccl();
  const size_t T = (size_t)h->T, N = (size_t)h->N, W = (size_t)h->comm_world;
  const size_t nX = T * N * 7, nU = T * (N - 1) * 3, nS = T * sizeof(tsat_stats);
  // Every rank must hold a shard of the same shape (T, N): the receive buffers are sized world x this rank's shard and the
  // collective sends this rank's count. Checked by a 16-byte all-gather of (T, N) whenever the shape is new to the communicator;
  // every rank sees the same gathered list, so a mismatch fails on all of them alike instead of corrupting memory on some.
  if (h->comm_T != h->T || h->comm_N != h->N) {
    int64_t* chk = (int64_t*)ws_get(h, tsat_handle::WS_AG_CHK, (W + 1) * 2 * sizeof(int64_t));
    if (!chk) return fail(h, -10, "device allocation failed in tsat_sweep_allgather");
    const int64_t mine[2] = {h->T, (int64_t)h->N};
    std::vector<int64_t> all(2 * W);
    TSAT_HIP(h, hipMemcpyAsync(chk + 2 * W, mine, sizeof(mine), hipMemcpyHostToDevice, h->stream));
    const ncclResult_t rc0 = a.AllGather(chk + 2 * W, chk, 2, ncclInt64, (ncclComm_t)h->comm, h->stream);
    if (rc0 != ncclSuccess) return rccl_fail(h, "ncclAllGather (shard shapes)", rc0);
    TSAT_HIP(h, hipMemcpyAsync(all.data(), chk, 2 * W * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    TSAT_HIP(h, hipStreamSynchronize(h->stream));
    for (size_t r = 0; r < W; ++r)
      if (all[2 * r] != h->T || all[2 * r + 1] != h->N)
        return fail(h, -1, "tsat_sweep_allgather: rank " + std::to_string(r) + " holds a " + std::to_string(all[2 * r]) + " x " +
                               std::to_string(all[2 * r + 1]) + " shard, this rank " + std::to_string(h->T) + " x " + std::to_string(h->N) +
                               ": shards must have equal shapes (pad the last one)");
    h->comm_T = h->T; h->comm_N = h->N;
  }
  // this rank's shard in the ABI layout (export kernel, device to device), then one ncclAllGather per array on the same
  // stream; with host outputs the gathered arrays land in library workspaces and are copied down afterwards
  double* dX = X_all ? (double*)ws_get(h, tsat_handle::WS_AG_X, nX * 8) : nullptr;
  double* dU = U_all ? (double*)ws_get(h, tsat_handle::WS_AG_U, nU * 8) : nullptr;
  void* dS = stats_all ? ws_get(h, tsat_handle::WS_AG_ST, nS) : nullptr;
  if ((X_all && !dX) || (U_all && !dU) || (stats_all && !dS)) return fail(h, -10, "device allocation failed in tsat_sweep_allgather");
  void *gX = X_all, *gU = U_all, *gS = stats_all;
  if (!on_device) {
    gX = X_all ? ws_get(h, tsat_handle::WS_AG_XA, W * nX * 8) : nullptr;
    gU = U_all ? ws_get(h, tsat_handle::WS_AG_UA, W * nU * 8) : nullptr;
    gS = stats_all ? ws_get(h, tsat_handle::WS_AG_STA, W * nS) : nullptr;
    if ((X_all && !gX) || (U_all && !gU) || (stats_all && !gS)) return fail(h, -10, "device allocation failed in tsat_sweep_allgather");
  }
  const int64_t n_rec = h->T * (int64_t)h->N;
  if (dX || dU) {
    hipLaunchKernelGGL(tsat_export_kernel<double>, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, h->stream, n_rec, h->N,
                       h->ragged ? h->nk : nullptr, h->XU, h->KD, dX, dU, (double*)nullptr);
    TSAT_HIP(h, hipGetLastError());
  }
  if (dS) TSAT_HIP(h, hipMemcpyAsync(dS, h->stats, nS, hipMemcpyDeviceToDevice, h->stream));
  ncclResult_t r = ncclSuccess;
  if (dS && r == ncclSuccess) r = a.AllGather(dS, gS, nS, ncclUint8, (ncclComm_t)h->comm, h->stream);
  if (dX && r == ncclSuccess) r = a.AllGather(dX, gX, nX, ncclFloat64, (ncclComm_t)h->comm, h->stream);
  if (dU && r == ncclSuccess) r = a.AllGather(dU, gU, nU, ncclFloat64, (ncclComm_t)h->comm, h->stream);
  if (r != ncclSuccess) return rccl_fail(h, "ncclAllGather", r);
  if (!on_device) {
    if (gX) TSAT_HIP(h, hipMemcpyAsync(X_all, gX, W * nX * 8, hipMemcpyDeviceToHost, h->stream));
    if (gU) TSAT_HIP(h, hipMemcpyAsync(U_all, gU, W * nU * 8, hipMemcpyDeviceToHost, h->stream));
    if (gS) TSAT_HIP(h, hipMemcpyAsync(stats_all, gS, W * nS, hipMemcpyDeviceToHost, h->stream));
  }
  TSAT_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

void tsat_btable_default_options(tsat_btable_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->n_half = 5000;                          // src/TortoiseSat.jl:61
  o->mjd = 58155.0;                          // src/TortoiseSat.jl:44
  o->gm = 3.986004418e14 * 1e-9;             // km^3/s^2, src/input_parameters.jl:26
  o->r_igrf_km = 400.0 + 6371.0;             // alt + R_E, src/magnetic_toolbox.jl:44,81
  o->date = 2019.0;                          // src/magnetic_toolbox.jl:81
}

// Host-side script arithmetic, batched: Bryson weights of the versine eigen-axis guess for T slews that differ only in their
// horizon (src/eigen_axis_slew.jl:1-38 + src/monte_carlo.jl:161-176 in the loop body of the Monte-Carlo script). No GPU work.
int tsat_bryson_eigen_axis_batch(int64_t T, const int32_t* n_knots, double t0, double dt, double theta_f, const double* axis,
                                 const double* Jrm, double alpha, double beta, double* Qd, double* Qfd, double* Rd) {
  if (T < 1 || !n_knots || !axis || !Jrm || !Qd || !Qfd || !Rd || !(dt > 0)) return -1;
  for (int64_t t = 0; t < T; ++t)
    if (n_knots[t] < 3) return -1;
  std::atomic<int> bad{0};
  auto work = [&](int64_t lo, int64_t hi) {
    std::vector<double> d;
    for (int64_t j = lo; j < hi; ++j) {
      const int n = n_knots[j];
      const double a = 3.14159265358979323846 / (t0 + dt * (double)(n - 1));        // alpha = pi / t[end]
      const double h = (t0 + dt * 1.0) - (t0 + dt * 0.0);                             // t[2] - t[1]
      d.resize((size_t)n - 1);
      double th0 = theta_f * 0.5 * (1.0 - std::cos(a * (t0 + dt * 0.0)));
      for (int k = 0; k < n - 1; ++k) {                                              // d_theta = diff(theta) / (t[2] - t[1])
        const double th1 = theta_f * 0.5 * (1.0 - std::cos(a * (t0 + dt * (double)(k + 1))));
        d[(size_t)k] = (th1 - th0) / h;
        th0 = th1;
      }
      double wmax = 0.0, taumax = -1.0 / 0.0;
      for (int k = 0; k < n - 1; ++k)
        for (int c = 0; c < 3; ++c) wmax = std::max(wmax, std::fabs(d[(size_t)k] * axis[c]));
      // w has n rows (the last rate repeated): diff(w) has n - 1 rows, the last one zero; tau = J dw / dt, signed maximum
      for (int k = 0; k < n - 1; ++k) {
        double dw[3];
        for (int c = 0; c < 3; ++c) dw[c] = (k < n - 2) ? d[(size_t)k + 1] * axis[c] - d[(size_t)k] * axis[c] : 0.0;
        for (int r = 0; r < 3; ++r) taumax = std::max(taumax, ((Jrm[3 * r] * dw[0] + Jrm[3 * r + 1] * dw[1]) + Jrm[3 * r + 2] * dw[2]) / dt);
      }
      if (!(wmax > 0.0) || !(taumax > 0.0)) { bad = 1; continue; }
      const double mmax = taumax / 1.0e-5 * 1.0e2;
      for (int i = 0; i < 7; ++i) { Qd[7 * j + i] = (i < 3) ? alpha / (wmax * wmax) : alpha * beta; Qfd[7 * j + i] = 10.0 * Qd[7 * j + i]; }
      for (int c = 0; c < 3; ++c) Rd[3 * j + c] = 1.0 / (mmax * mmax);
    }
  };
  const int nth = (int)std::min<int64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), (T + 63) / 64);
  std::vector<std::thread> th;
  for (int i = 0; i < nth; ++i) th.emplace_back(work, T * i / nth, T * (i + 1) / nth);
  for (auto& x : th) x.join();
  return bad ? -2 : 0;
}

int tsat_btable_batch(tsat_handle* h, const tsat_btable_options* o, int64_t T, const double* kep, const double* t0,
                      const double* tf, double* Btab, double* pos) {
  if (!h || !o) return -1;
  // whatever happens below, the tables of an earlier call are no longer "the last call's": a consumer with Btab = NULL must
  // never pick up stale ones by shape alone (a failed call leaves none)
  h->bt_T = 0; h->bt_rows = 0; h->bt_gen++;
  if (T < 1 || o->n_half < 1) return fail(h, -1, "bad dimensions");
  if (!(o->date >= 2015.0 && o->date < 2020.0)) return fail(h, -1, "date must be in [2015, 2020): IGRF-12 epoch 2015 + secular variation");
  if (!kep || !t0 || !tf) return fail(h, -1, "null array");
  for (int64_t t = 0; t < T; ++t)
    if (!(kep[6 * t] >= 0.0 && kep[6 * t] < 1.0) || !(kep[6 * t + 1] > 0.0) || !(tf[t] > t0[t]))
      return fail(h, -1, "need 0 <= e < 1, a > 0 and tf > t0");
  TSAT_HIP(h, hipSetDevice(h->dev));
  const int N = o->n_half;
  const size_t Tn = (size_t)T, nP = Tn * 3 * (2 * (size_t)N + 1), nB = Tn * 3 * 2 * (size_t)N;
  std::vector<double> coef;
  igrf_records(o->date, o->r_igrf_km, coef);
  double *dc = nullptr, *dk = nullptr, *d0 = nullptr, *d1 = nullptr, *dP = nullptr, *dB = nullptr;
  int rc = 0;
  auto A = [&](void** p, int slot, size_t bytes) { if (!rc && !(*p = ws_get(h, slot, bytes))) rc = -10; };
  A((void**)&dc, tsat_handle::WS_BT_COEF, coef.size() * 8); A((void**)&dk, tsat_handle::WS_BT_KEP, Tn * 6 * 8);
  A((void**)&d0, tsat_handle::WS_BT_T0, Tn * 8); A((void**)&d1, tsat_handle::WS_BT_TF, Tn * 8);
  A((void**)&dP, tsat_handle::WS_BT_POS, nP * 8); A((void**)&dB, tsat_handle::WS_BT_B, nB * 8);
  auto Cp = [&](void* d, const void* s, size_t bytes) { if (!rc && hipMemcpy(d, s, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = -10; };
  Cp(dc, coef.data(), coef.size() * 8); Cp(dk, kep, Tn * 6 * 8); Cp(d0, t0, Tn * 8); Cp(d1, tf, Tn * 8);
  if (!rc) {
    BtArgs<double> a;
    a.T = (int)T; a.n_half = N; a.mjd = o->mjd; a.gm = o->gm; a.r_igrf_km = o->r_igrf_km;
    a.tab = dc; a.kep = dk; a.t0 = d0; a.tf = d1; a.pos = dP; a.B = dB;
    hipLaunchKernelGGL(tsat_btable_kernel<double>, dim3((unsigned)T), dim3(64), 0, h->stream, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) rc = -10;
  }
  if (!rc && Btab && hipMemcpy(Btab, dB, nB * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (!rc && pos && hipMemcpy(pos, dP, nP * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  if (rc) h->err = "device allocation, copy or launch failed in tsat_btable_batch";
  h->bt_T = rc ? 0 : T; h->bt_rows = rc ? 0 : 2 * N;     // the tables stay resident for tsat_horizon_batch / tsat_batch_upload
  return rc;
}

}  // extern "C"
