// tsat_kernels_mpc_dispersed.hip — the plant step of tsat_mpc_run_dispersed (include/tortoise_hip.h; tsat_mpc_dispersed.hpp). The host loop
// in tsat_kernels.hip owns the handle's buffers and calls the one launcher below once per control step, where tsat_mpc_run launches
// its advance kernel.
#include <hip/hip_runtime.h>
#include "tsat_mpc_dispersed.hpp"

using namespace tsat;

__global__ __launch_bounds__(64) void tsat_mpc_dispersed_kernel(MpcDispArgs<double> a) {
  const int traj = blockIdx.x;
  if (traj >= a.m.T) return;
  mpc_dispersed_trajectory<double>(a, traj);
}

// plants 21 x T (or null: the model's) -> packed records [T][PLW], running records zeroed; one thread per trajectory
__global__ __launch_bounds__(256) void tsat_mpc_dispersed_pack_kernel(const double* plant, const double* P, double us, double* PL,
                                                                      MpcDispRec* rec, int64_t T) {
  mpc_dispersed_pack<double>(plant, P, us, PL, rec, T, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// step a.m.step of the loop on `stream`; step 0 first packs the call's plant records from `plant` (device, 21 x T, or null)
hipError_t tsat_launch_mpc_dispersed(const MpcDispArgs<double>& a, const double* plant, hipStream_t stream) {
  const int64_t T = a.m.T;
  if (a.m.step == 0) {
    hipLaunchKernelGGL(tsat_mpc_dispersed_pack_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, plant, (const double*)a.m.P,
                       a.m.us, (double*)a.d.PL, a.rec, T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tsat_mpc_dispersed_kernel, dim3((unsigned)T), dim3(64), 0, stream, a);
  return hipGetLastError();
}
