// tsat_kernels_aplqr.hip — the kernels of tsat_aplqr_gains and tsat_aplqr_ensemble (include/tortoise_hip.h; tsat_aplqr.hpp): the
// synthesis of the asymptotic periodic LQR, one wavefront per slew, and its roll-out on the plants of the dispersed ensemble, with
// and without the gravity rows. A translation unit of its own, so that no existing kernel is recompiled differently. The host code
// of the entry points (tsat_kernels_ensemble.hip) owns the buffers and calls the launchers.
#include <hip/hip_runtime.h>
#include "tsat_aplqr.hpp"

using namespace tsat;

// grid (T): averaged Gramian, 6 x 6 CARE, gain
__global__ __launch_bounds__(64) void tsat_aplqr_gains_kernel(AplqrGainArgs a) {
  aplqr_gains_wave(a, (int)blockIdx.x);
}

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_pd_kernel
__global__ __launch_bounds__(64) void tsat_aplqr_kernel(PdArgs<double> a) {
  aplqr_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(64) void tsat_aplqr_gg_kernel(PdArgs<double> a) {
  aplqr_gg_wave<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

hipError_t tsat_launch_aplqr_gains(const AplqrGainArgs& a, int64_t T, hipStream_t stream) {
  hipLaunchKernelGGL(tsat_aplqr_gains_kernel, dim3((unsigned)T), dim3(64), 0, stream, a);
  return hipGetLastError();
}

// a.GT == null: the instantiation on DispersedPlant; otherwise the one on GgPlant
hipError_t tsat_launch_aplqr(const PdArgs<double>& a, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(a.GT ? tsat_aplqr_gg_kernel : tsat_aplqr_kernel, dim3((unsigned)a.d.e.T, (unsigned)waves), dim3(64), 0, stream, a);
  return hipGetLastError();
}
