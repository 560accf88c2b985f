// tsat_kernels_model_mag_sun_filtered.hip — the kernels of tsat_tvlqr_ensemble_model_mag_sun_filtered and
// tsat_pd_ensemble_model_mag_sun_filtered (include/tortoise_hip.h; tsat_model_mag_sun_filtered.hpp): the TVLQR feedback and the
// projection PD law commanding from the estimate of the magnetometer-updated model filter with a sun-vector update that eclipse
// switches off, each on the plants of the dispersed ensemble with and without the gravity rows. A translation unit of its own, so
// that no existing kernel is recompiled differently. The host code of the entry points (tsat_kernels_ensemble.hip) owns the buffers,
// packs the sun rows with the pack of the field rows and calls the launchers.
#include <hip/hip_runtime.h>
#include "tsat_model_mag_sun_filtered.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_model_mag_sun_filtered_tv_kernel(ModelMagSunFilteredTvArgs<double> a) {
  model_mag_sun_filtered_tv_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_sun_filtered_tv_gg_kernel(ModelMagSunFilteredTvArgs<double> a) {
  model_mag_sun_filtered_tv_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_sun_filtered_pd_kernel(ModelMagSunFilteredPdArgs<double> a) {
  model_mag_sun_filtered_pd_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_model_mag_sun_filtered_pd_gg_kernel(ModelMagSunFilteredPdArgs<double> a) {
  model_mag_sun_filtered_pd_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// a.g.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_model_mag_sun_filtered_tv(const ModelMagSunFilteredTvArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.g.GT ? tsat_model_mag_sun_filtered_tv_gg_kernel : tsat_model_mag_sun_filtered_tv_kernel,
                     dim3((unsigned)a.g.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t tsat_launch_model_mag_sun_filtered_pd(const ModelMagSunFilteredPdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.p.GT ? tsat_model_mag_sun_filtered_pd_gg_kernel : tsat_model_mag_sun_filtered_pd_kernel,
                     dim3((unsigned)a.p.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}
