// tsat_kernels_pd.hip — the kernels of tsat_pd_ensemble (include/tortoise_hip.h; tsat_pd.hpp): the projection PD law on the plants
// of the dispersed ensemble, with and without the gravity rows. A translation unit of its own, so that no existing kernel is
// recompiled differently. The host code of the entry point (tsat_kernels_ensemble.hip) owns the buffers and calls the launcher.
#include <hip/hip_runtime.h>
#include "tsat_pd.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_pd_kernel(PdArgs<double> a) {
  pd_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_pd_gg_kernel(PdArgs<double> a) {
  pd_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// a.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_pd(const PdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.GT ? tsat_pd_gg_kernel : tsat_pd_kernel, dim3((unsigned)a.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}
