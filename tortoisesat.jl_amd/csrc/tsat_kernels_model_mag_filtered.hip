// tsat_kernels_model_mag_filtered.hip — the kernels of tsat_tvlqr_ensemble_model_mag_filtered and tsat_pd_ensemble_model_mag_filtered
// (include/tortoise_hip.h; tsat_model_mag_filtered.hpp): the TVLQR feedback and the projection PD law commanding from the estimate
// of the nine-state model filter whose attitude update is the magnetometer's, each on the plants of the dispersed ensemble with and
// without the gravity rows. A translation unit of its own, so that no existing kernel is recompiled differently. The host code of
// the entry points (tsat_kernels_ensemble.hip) owns the buffers and calls the launchers; the biases are packed by the launch of the
// sensed unit.
#include <hip/hip_runtime.h>
#include "tsat_model_mag_filtered.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_model_mag_filtered_tv_kernel(ModelMagFilteredTvArgs<double> a) {
  model_mag_filtered_tv_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_filtered_tv_gg_kernel(ModelMagFilteredTvArgs<double> a) {
  model_mag_filtered_tv_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_filtered_pd_kernel(ModelMagFilteredPdArgs<double> a) {
  model_mag_filtered_pd_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_filtered_pd_gg_kernel(ModelMagFilteredPdArgs<double> a) {
  model_mag_filtered_pd_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// a.g.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_model_mag_filtered_tv(const ModelMagFilteredTvArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.g.GT ? tsat_model_mag_filtered_tv_gg_kernel : tsat_model_mag_filtered_tv_kernel,
                     dim3((unsigned)a.g.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t tsat_launch_model_mag_filtered_pd(const ModelMagFilteredPdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.p.GT ? tsat_model_mag_filtered_pd_gg_kernel : tsat_model_mag_filtered_pd_kernel,
                     dim3((unsigned)a.p.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}
