// tsat_kernels_mag_bias_filtered.hip — the kernels of tsat_tvlqr_ensemble_mag_bias_filtered and tsat_pd_ensemble_mag_bias_filtered
// (include/tortoise_hip.h; tsat_mag_bias_filtered.hpp): the TVLQR feedback and the projection PD law commanding from the estimate of
// the magnetometer-updated EKF that also estimates the magnetometer bias (nine error states), each on the plants of the dispersed
// ensemble with and without the gravity rows. A translation unit of its own, so that no existing kernel is recompiled differently.
// The host code of the entry points (tsat_kernels_ensemble.hip) owns the buffers and calls the launchers; the biases are packed by
// the launch of the sensed unit.
#include <hip/hip_runtime.h>
#include "tsat_mag_bias_filtered.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_mag_bias_filtered_tv_kernel(MagBiasFilteredTvArgs<double> a) {
  mag_bias_filtered_tv_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_mag_bias_filtered_tv_gg_kernel(MagBiasFilteredTvArgs<double> a) {
  mag_bias_filtered_tv_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_mag_bias_filtered_pd_kernel(MagBiasFilteredPdArgs<double> a) {
  mag_bias_filtered_pd_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_mag_bias_filtered_pd_gg_kernel(MagBiasFilteredPdArgs<double> a) {
  mag_bias_filtered_pd_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// a.g.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_mag_bias_filtered_tv(const MagBiasFilteredTvArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.g.GT ? tsat_mag_bias_filtered_tv_gg_kernel : tsat_mag_bias_filtered_tv_kernel,
                     dim3((unsigned)a.g.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t tsat_launch_mag_bias_filtered_pd(const MagBiasFilteredPdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.p.GT ? tsat_mag_bias_filtered_pd_gg_kernel : tsat_mag_bias_filtered_pd_kernel,
                     dim3((unsigned)a.p.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}
