// tsat_kernels_gg.hip — the kernels of tsat_tvlqr_ensemble_gg and tsat_mpc_run_held_gg (include/tortoise_hip.h; tsat_gg.hpp): the
// dispersed ensemble and the hold under gravity-gradient torque, and the pack of the orbit table. The host code of the two entry
// points (tsat_kernels_ensemble.hip, tsat_kernels.hip) owns the buffers and calls the launchers below.
#include <hip/hip_runtime.h>
#include "tsat_gg.hpp"

using namespace tsat;

// lane = realisation, grid (T, ceil((M + 1) / 64)): the mapping of tsat_dispersed_kernel
__global__ __launch_bounds__(64) void tsat_ensemble_gg_kernel(GgEnsArgs<double> g) {
  gg_wave<double>(g, (int)blockIdx.x, (int)blockIdx.y);
}

// lane = trajectory: the mapping of tsat_mpc_held_kernel
template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_held_gg_kernel(MpcHeldGgArgs<double> a) {
  mpc_held_gg_block<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

// orbit rows [rows][3] (km) -> [rows][4] = [r^, 3 gm / |r|^3]; one thread per row
__global__ __launch_bounds__(256) void tsat_gg_pack_kernel(const double* R, double gm, double* GT, int64_t rows) {
  gg_pack_row<double>(R, gm, GT, rows, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

hipError_t tsat_launch_gg_pack(const double* R, double gm, double* GT, int64_t rows, hipStream_t stream) {
  hipLaunchKernelGGL(tsat_gg_pack_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, R, gm, GT, rows);
  return hipGetLastError();
}

hipError_t tsat_launch_ensemble_gg(const GgEnsArgs<double>& g, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(tsat_ensemble_gg_kernel, dim3((unsigned)g.d.e.T, (unsigned)waves), dim3(64), 0, stream, g);
  return hipGetLastError();
}

// the block of a.h.r control steps, as tsat_launch_mpc_held
hipError_t tsat_launch_mpc_held_gg(const MpcHeldGgArgs<double>& a, int error_state, hipStream_t stream) {
  const unsigned T = (unsigned)a.h.s.m.T;
  hipLaunchKernelGGL(error_state ? tsat_mpc_held_gg_kernel<1> : tsat_mpc_held_gg_kernel<0>, dim3((T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}
