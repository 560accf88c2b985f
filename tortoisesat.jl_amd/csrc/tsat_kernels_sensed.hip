// tsat_kernels_sensed.hip — the kernels of tsat_tvlqr_ensemble_sensed and tsat_pd_ensemble_sensed (include/tortoise_hip.h;
// tsat_sensed.hpp): the TVLQR feedback and the projection PD law commanding from a measurement, each on the plants of the
// dispersed ensemble with and without the gravity rows. A translation unit of its own, so that no existing kernel is recompiled
// differently. The host code of the entry points (tsat_kernels_ensemble.hip) owns the buffers and calls the launchers.
#include <hip/hip_runtime.h>
#include "tsat_sensed.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_sensed_tv_kernel(SensedTvArgs<double> a) {
  sensed_tv_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_sensed_tv_gg_kernel(SensedTvArgs<double> a) {
  sensed_tv_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_sensed_pd_kernel(SensedPdArgs<double> a) {
  sensed_pd_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_sensed_pd_gg_kernel(SensedPdArgs<double> a) {
  sensed_pd_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// biases 9 x M x T (or null) -> per-lane records [T][SNW][Mp], slot M and the padding zero; one thread per slot
__global__ __launch_bounds__(256) void tsat_sensed_pack_kernel(const double* sensor, double* SN, int64_t T, int M, int Mp) {
  sensed_pack<double>(sensor, SN, T, M, Mp, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

hipError_t tsat_launch_sensed_pack(const double* sensor, double* SN, int64_t T, int M, int Mp, hipStream_t stream) {
  const int64_t n = T * (int64_t)Mp;
  hipLaunchKernelGGL(tsat_sensed_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sensor, SN, T, M, Mp);
  return hipGetLastError();
}

// a.g.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_sensed_tv(const SensedTvArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.g.GT ? tsat_sensed_tv_gg_kernel : tsat_sensed_tv_kernel, dim3((unsigned)a.g.d.e.T, (unsigned)waves), dim3(64), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t tsat_launch_sensed_pd(const SensedPdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.p.GT ? tsat_sensed_pd_gg_kernel : tsat_sensed_pd_kernel, dim3((unsigned)a.p.d.e.T, (unsigned)waves), dim3(64), 0,
                     stream, a);
  return hipGetLastError();
}
