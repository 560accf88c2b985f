// tsat_kernels_mpc_held.hip — the hold and the plan shift of tsat_mpc_run_held (include/tortoise_hip.h; tsat_mpc_held.hpp). The
// host loop in tsat_kernels.hip owns the handle's buffers and calls the launchers below: the pack once per call, then a hold (this
// one, or that of tsat_kernels_gg.hip or tsat_kernels_mpc_sensed.hip) and the shift after every solve.
#include <hip/hip_runtime.h>
#include "tsat_mpc_held.hpp"

using namespace tsat;

// lane = trajectory: thread 64 block + lane flies trajectory 64 block + lane through the block's a.r control steps
template <int ES>
__global__ __launch_bounds__(64) void tsat_mpc_held_kernel(MpcHeldArgs<double> a) {
  mpc_held_block<double, ES>(a, (int)(blockIdx.x * 64 + threadIdx.x));
}

// one wavefront per trajectory, lanes = knots: U0[t][k] <- XU[t][min(k + r, n_t - 2)]
__global__ __launch_bounds__(64) void tsat_mpc_held_shift_kernel(MpcArgs<double> m, int r) {
  const int traj = blockIdx.x;
  if (traj >= m.T) return;
  mpc_held_shift<double>(m, r, traj);
}

// plants 21 x T (or null: the model's), limits [T][SATW] and parameter records -> records [HELD_W][T], running records zeroed
__global__ __launch_bounds__(256) void tsat_mpc_held_pack_kernel(const double* plant, const double* P, const double* SAT, double us,
                                                                 double* HR, MpcDispRec* rec, int64_t T) {
  mpc_held_pack<double>(plant, P, SAT, us, HR, rec, T, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

hipError_t tsat_launch_mpc_held_pack(const MpcHeldArgs<double>& a, const double* plant, hipStream_t stream) {
  const int64_t T = a.s.m.T;
  hipLaunchKernelGGL(tsat_mpc_held_pack_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, plant, (const double*)a.s.m.P,
                     a.s.d.SAT, a.s.m.us, (double*)a.s.d.PL, a.s.rec, T);
  return hipGetLastError();
}

// the plan shifted by r as the next warm start, after whichever hold ran
hipError_t tsat_launch_mpc_held_shift(const MpcArgs<double>& m, int r, hipStream_t stream) {
  hipLaunchKernelGGL(tsat_mpc_held_shift_kernel, dim3((unsigned)m.T), dim3(64), 0, stream, m, r);
  return hipGetLastError();
}

// the block of a.r control steps from step a.s.m.step on `stream`
hipError_t tsat_launch_mpc_held(const MpcHeldArgs<double>& a, int error_state, hipStream_t stream) {
  const unsigned T = (unsigned)a.s.m.T;
  hipLaunchKernelGGL(error_state ? tsat_mpc_held_kernel<1> : tsat_mpc_held_kernel<0>, dim3((T + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}
