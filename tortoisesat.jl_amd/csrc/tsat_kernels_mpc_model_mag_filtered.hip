// tsat_kernels_mpc_model_mag_filtered.hip — the kernels of tsat_mpc_run_held_model_mag_filtered (include/tortoise_hip.h;
// tsat_mpc_model_mag_filtered.hpp): the hold of the re-planning loop commanding and re-planning from the estimate of the
// magnetometer-updated nine-state filter, with and without the gravity rows, and the pack that makes the bias records, the call's
// first measurement, its first field sample and the first estimate. The host loop in tsat_kernels.hip owns the handle's buffers and
// calls the launchers below.
#include <hip/hip_runtime.h>
#include "tsat_mpc_model_mag_filtered.hpp"

using namespace tsat;

// lane = trajectory: the mapping of tsat_mpc_sensed_kernel
template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_model_mag_filtered_kernel(MpcModelMagFilteredArgs<double> a) {
  mpc_model_mag_filtered_traj<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_model_mag_filtered_gg_kernel(MpcModelMagFilteredArgs<double> a) {
  mpc_model_mag_filtered_gg_traj<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

// the pack of tsat_mpc_sensed_pack_kernel, then sample 0 through the filter: `given` — FL already holds the caller's records
__global__ __launch_bounds__(64) void tsat_mpc_model_mag_filtered_pack_kernel(MpcModelMagFilteredArgs<double> a, const double* sensor, int given) {
  mpc_model_mag_filtered_pack<double>(a, sensor, given, (int64_t)blockIdx.x * 64 + threadIdx.x);
}

// after tsat_launch_mpc_held_pack (the plant records and the zeroed running records), before the first solve
hipError_t tsat_launch_mpc_model_mag_filtered_pack(const MpcModelMagFilteredArgs<double>& a, const double* sensor, int given, hipStream_t stream) {
  const unsigned T = (unsigned)a.ms.h.s.m.T;
  hipLaunchKernelGGL(tsat_mpc_model_mag_filtered_pack_kernel, dim3((T + 63) / 64), dim3(64), 0, stream, a, sensor, given);
  return hipGetLastError();
}

// the block of a.ms.h.r control steps, as tsat_launch_mpc_model_filtered; a.ms.GT == null: the instantiation without the gravity rows
hipError_t tsat_launch_mpc_model_mag_filtered(const MpcModelMagFilteredArgs<double>& a, int error_state, hipStream_t stream) {
  const unsigned T = (unsigned)a.ms.h.s.m.T;
  auto k = a.ms.GT ? (error_state ? tsat_mpc_model_mag_filtered_gg_kernel<1> : tsat_mpc_model_mag_filtered_gg_kernel<0>)
                   : (error_state ? tsat_mpc_model_mag_filtered_kernel<1> : tsat_mpc_model_mag_filtered_kernel<0>);
  hipLaunchKernelGGL(k, dim3((T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}
