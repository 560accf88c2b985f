// tsat_kernels_dense.hip — the "dense" build of the solve kernel (build 2 of the table at the head of tsat_device.hpp): the same
// source as the wide build in tsat_kernels.hip, laid out for TWO wavefronts per SIMD. Results are bit-identical (the chunking does
// not touch the arithmetic). This file is the unit of the fp64 build and the body of tsat_kernels_dense_mixed.hip (TSAT_JAC32:
// float linearisation, options.precision = 32).
#ifndef TSAT_BUILD
#define TSAT_BUILD 2
#endif
#include <hip/hip_runtime.h>
#include "tsat_device.hpp"

using namespace tsat;

template <typename real, int INTEG, int DIAGJ, int ES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void TSAT_BUILD_NAME(tsat_solve_kernel_dense)(KArgs<real> a) {
  const int traj = blockIdx.x;
  if (traj >= a.T) return;
  solve_trajectory<real, INTEG, DIAGJ, ES>(a, traj);
}

// called by tsat_kernels.hip; same variant axes as the wide build: integrator x inertia class x error-state mode
hipError_t TSAT_BUILD_NAME(tsat_launch_solve_dense)(const KArgs<double>& a, int rk4, int inertia_class, int error_state, hipStream_t stream) {
  using kern_t = void (*)(KArgs<double>);
  static const kern_t variants[2][3][2] = TSAT_VARIANT_TABLE(TSAT_BUILD_NAME(tsat_solve_kernel_dense));
  hipLaunchKernelGGL(variants[rk4 ? 1 : 0][inertia_class][error_state ? 1 : 0], dim3((unsigned)a.T), dim3(64), 0, stream, a);
  return hipGetLastError();
}
