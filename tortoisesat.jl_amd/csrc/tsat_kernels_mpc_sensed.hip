// tsat_kernels_mpc_sensed.hip — the kernels of tsat_mpc_run_held_sensed (include/tortoise_hip.h; tsat_mpc_sensed.hpp): the hold of
// the re-planning loop commanding and re-planning from a measurement, with and without the gravity rows, and the pack that makes
// the bias records and the call's first measurement. The host loop in tsat_kernels.hip owns the handle's buffers and calls the
// launchers below.
#include <hip/hip_runtime.h>
#include "tsat_mpc_sensed.hpp"

using namespace tsat;

// lane = trajectory: the mapping of tsat_mpc_held_kernel
template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_sensed_kernel(MpcSensedArgs<double> a) {
  mpc_sensed_traj<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_sensed_gg_kernel(MpcSensedArgs<double> a) {
  mpc_sensed_gg_traj<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

// biases 9 x T (or null) -> [SNW][T]; the true state to its record, the first measurement into the parameter record
__global__ __launch_bounds__(64) void tsat_mpc_sensed_pack_kernel(MpcSensedArgs<double> a, const double* sensor) {
  mpc_sensed_pack<double>(a, sensor, (int64_t)blockIdx.x * 64 + threadIdx.x);
}

// after tsat_launch_mpc_held_pack (the plant records and the zeroed running records), before the first solve
hipError_t tsat_launch_mpc_sensed_pack(const MpcSensedArgs<double>& a, const double* sensor, hipStream_t stream) {
  const unsigned T = (unsigned)a.h.s.m.T;
  hipLaunchKernelGGL(tsat_mpc_sensed_pack_kernel, dim3((T + 63) / 64), dim3(64), 0, stream, a, sensor);
  return hipGetLastError();
}

// the block of a.h.r control steps, as tsat_launch_mpc_held; a.GT == null: the instantiation without the gravity rows
hipError_t tsat_launch_mpc_sensed(const MpcSensedArgs<double>& a, int error_state, hipStream_t stream) {
  const unsigned T = (unsigned)a.h.s.m.T;
  auto k = a.GT ? (error_state ? tsat_mpc_sensed_gg_kernel<1> : tsat_mpc_sensed_gg_kernel<0>)
                : (error_state ? tsat_mpc_sensed_kernel<1> : tsat_mpc_sensed_kernel<0>);
  hipLaunchKernelGGL(k, dim3((T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}
