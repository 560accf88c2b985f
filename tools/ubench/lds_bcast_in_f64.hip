// What does an LDS read cost a lone wavefront inside an fp64 stream, and what does the DPP form that would replace it cost?
// One wavefront per SIMD (the one-trajectory mapping at T <= 1024), s_memtime ticks, in the style of valu_f64.hip.
//   (a) 100 chain-free v_fma_f64 with k = 0, 4, 8, 12 wave-uniform (broadcast) ds_read_b128 in front of them, issued in one batch and
//       waited for a whole turn later — what fwd_knot_load does with a knot's K, d record;
//   (b) the same stream with ONE lane-indexed ds_read_b128 (address base + 16 (lane & 15)): the record as two doubles per lane;
//   (c) 21 v_fmac_f64_dpp row_newbcast into three accumulators — one accumulator after the other (7 in a row), the three
//       interleaved, and interleaved with 1 or 2 independent fp64 instructions after every DPP FMA — against the same number of
//       chain-free v_fma_f64.
// Only differences inside one part are read: the streams of (a) / (b) carry an s_waitcnt per group of 100 and run ten accumulators
// (4.56 cycles per FMA), the blocks of (c) three to nine (4.10), so a figure of (a) is no baseline for (c) and the other way round.
// Build: hipcc --offload-arch=gfx950 -O3 lds_bcast_in_f64.hip -o lds_bcast_in_f64
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define STR2(x) #x
#define STR(x) STR2(x)
#define REPT 16

__device__ inline unsigned long long now() {
  unsigned long long t = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return t;
}

// 100 chain-free FMAs: ten accumulators, each touched again ten instructions later
#define FMA10 " v_fma_f64 %0, %10, %11, %0\n v_fma_f64 %1, %10, %11, %1\n v_fma_f64 %2, %10, %11, %2\n v_fma_f64 %3, %10, %11, %3\n v_fma_f64 %4, %10, %11, %4\n" \
              " v_fma_f64 %5, %10, %11, %5\n v_fma_f64 %6, %10, %11, %6\n v_fma_f64 %7, %10, %11, %7\n v_fma_f64 %8, %10, %11, %8\n v_fma_f64 %9, %10, %11, %9\n"
#define FMA100 ".rept 10\n" FMA10 ".endr\n"
// read i lands in v[160 + 4 i : 163 + 4 i] (named registers, clobbered: twelve more "+v" operands are more than an asm takes)
#define RD(i, lo, hi, off) " ds_read_b128 v[" #lo ":" #hi "], %12 offset:" #off "\n"
#define RD4A RD(0, 160, 163, 0) RD(1, 164, 167, 16) RD(2, 168, 171, 32) RD(3, 172, 175, 48)
#define RD4B RD(4, 176, 179, 64) RD(5, 180, 183, 80) RD(6, 184, 187, 96) RD(7, 188, 191, 112)
#define RD4C RD(8, 192, 195, 128) RD(9, 196, 199, 144) RD(10, 200, 203, 160) RD(11, 204, 207, 176)
#define C4(a, b, c, d) "v" #a, "v" #b, "v" #c, "v" #d
#define RDCLOB C4(160, 161, 162, 163), C4(164, 165, 166, 167), C4(168, 169, 170, 171), C4(172, 173, 174, 175), C4(176, 177, 178, 179), C4(180, 181, 182, 183), \
               C4(184, 185, 186, 187), C4(188, 189, 190, 191), C4(192, 193, 194, 195), C4(196, 197, 198, 199), C4(200, 201, 202, 203), C4(204, 205, 206, 207)

// K reads per 100 FMAs; LANEIDX: every lane its own 16-byte unit (K = 1) instead of one address for the whole wave
template <int K, int LANEIDX>
__global__ __launch_bounds__(64) void lds_in_fma(double* out, unsigned long long* cyc, int iters) {
  __shared__ __align__(16) double rec[32 * 24];
  const int l = threadIdx.x;
  for (int i = l; i < 32 * 24; i += 64) rec[i] = 1e-3 * i;
  __syncthreads();
  double a0 = 1.0 + 1e-9 * l, a1 = 1.1, a2 = 1.2, a3 = 1.3, a4 = 1.4, a5 = 1.5, a6 = 1.6, a7 = 1.7, a8 = 1.8, a9 = 1.9;
  const double x = 1.0 + 1e-12 * l, y = 1e-13 * (l + 1);
  const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) double*)rec + (LANEIDX ? 16u * (l & 15) : 0u);
  const unsigned long long t0 = now();
  for (int it = 0; it < iters; ++it) {
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(a8), "+v"(a9) \
            : "v"(x), "v"(y), "v"(addr) : "memory", RDCLOB
    if (K == 0) asm volatile(".rept " STR(REPT) "\n s_waitcnt lgkmcnt(0)\n" FMA100 ".endr" OPS);
    if (K == 1) asm volatile(".rept " STR(REPT) "\n s_waitcnt lgkmcnt(0)\n" RD(0, 160, 163, 0) FMA100 ".endr" OPS);
    if (K == 4) asm volatile(".rept " STR(REPT) "\n s_waitcnt lgkmcnt(0)\n" RD4A FMA100 ".endr" OPS);
    if (K == 8) asm volatile(".rept " STR(REPT) "\n s_waitcnt lgkmcnt(0)\n" RD4A RD4B FMA100 ".endr" OPS);
    if (K == 12) asm volatile(".rept " STR(REPT) "\n s_waitcnt lgkmcnt(0)\n" RD4A RD4B RD4C FMA100 ".endr" OPS);
#undef OPS
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const unsigned long long t1 = now();
  if (l == 0) cyc[blockIdx.x] = t1 - t0;
  out[blockIdx.x * 64 + l] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + a8 + a9;
}

// 21 DPP FMAs into three accumulators. ORDER 0: accumulator after accumulator (7 + 7 + 7); 1: the three interleaved;
// FILL independent v_fma_f64 after every DPP FMA. DPPF 0: the control, a chain-free v_fma_f64 in place of every DPP FMA.
#define DPPI(acc, n) " v_fmac_f64_dpp %" STR(acc) ", %10, %11 row_newbcast:" STR(n) " row_mask:0xf bank_mask:0xf\n"
#define PLAIN(acc, n) " v_fma_f64 %" STR(acc) ", %10, %11, %" STR(acc) "\n"
#define F1(a) " v_fma_f64 %" STR(a) ", %10, %11, %" STR(a) "\n"
template <int ORDER, int FILL, int DPPF>
__global__ __launch_bounds__(64) void dpp21(double* out, unsigned long long* cyc, int iters) {
  const int l = threadIdx.x;
  double a0 = 1.0 + 1e-9 * l, a1 = 1.1, a2 = 1.2, a3 = 1.3, a4 = 1.4, a5 = 1.5, a6 = 1.6, a7 = 1.7, a8 = 1.8, a9 = 1.9;
  const double x = 1e-13 * (l + 1), y = 1.0 + 1e-12 * l;
  const unsigned long long t0 = now();
  for (int it = 0; it < iters; ++it) {
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(a8), "+v"(a9) : "v"(x), "v"(y)
#define SEQ7(I, a) I(a, 0) I(a, 1) I(a, 2) I(a, 3) I(a, 4) I(a, 5) I(a, 6)
#define TRI0(I, n) I(0, n) I(1, n) I(2, n)
#define TRI1(I, n) I(0, n) F1(3) I(1, n) F1(4) I(2, n) F1(5)
#define TRI2(I, n) I(0, n) F1(3) F1(6) I(1, n) F1(4) F1(7) I(2, n) F1(5) F1(8)
#define ALL7(T, I) T(I, 0) T(I, 1) T(I, 2) T(I, 3) T(I, 4) T(I, 5) T(I, 6)
    if (ORDER == 0 && DPPF) asm volatile(".rept " STR(REPT) "\n" SEQ7(DPPI, 0) SEQ7(DPPI, 1) SEQ7(DPPI, 2) ".endr" OPS);
    if (ORDER == 0 && !DPPF) asm volatile(".rept " STR(REPT) "\n" SEQ7(PLAIN, 0) SEQ7(PLAIN, 1) SEQ7(PLAIN, 2) ".endr" OPS);
    if (ORDER == 1 && FILL == 0 && DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI0, DPPI) ".endr" OPS);
    if (ORDER == 1 && FILL == 0 && !DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI0, PLAIN) ".endr" OPS);
    if (ORDER == 1 && FILL == 1 && DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI1, DPPI) ".endr" OPS);
    if (ORDER == 1 && FILL == 1 && !DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI1, PLAIN) ".endr" OPS);
    if (ORDER == 1 && FILL == 2 && DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI2, DPPI) ".endr" OPS);
    if (ORDER == 1 && FILL == 2 && !DPPF) asm volatile(".rept " STR(REPT) "\n" ALL7(TRI2, PLAIN) ".endr" OPS);
#undef OPS
  }
  const unsigned long long t1 = now();
  if (l == 0) cyc[blockIdx.x] = t1 - t0;
  out[blockIdx.x * 64 + l] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + a8 + a9;
}

typedef void (*kern_t)(double*, unsigned long long*, int);
struct T { const char* name; kern_t k; };

int main() {
  double* d; unsigned long long* c;
  if (hipMalloc(&d, 2048 * 64 * 8) != hipSuccess || hipMalloc(&c, 2048 * 8) != hipSuccess) { printf("no device memory\n"); return 1; }
  std::vector<unsigned long long> hc(2048);
  const int iters = 200;
  auto run = [&](kern_t k, int blocks) {
    k<<<blocks, 64>>>(d, c, 4);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
    k<<<blocks, 64>>>(d, c, iters);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
    (void)hipMemcpy(hc.data(), c, blocks * 8, hipMemcpyDeviceToHost);
    double s = 0; for (int b = 0; b < blocks; ++b) s += (double)hc[b];
    return s / blocks / ((double)iters * REPT);      // cycles per group
  };
  for (int blocks : {1, 1024}) {
    printf("--- %d workgroups of one wavefront (%s)\n", blocks, blocks == 1 ? "alone on the chip" : "one per SIMD");
    const double f0 = run(lds_in_fma<0, 0>, blocks), f4 = run(lds_in_fma<4, 0>, blocks), f8 = run(lds_in_fma<8, 0>, blocks),
                 f12 = run(lds_in_fma<12, 0>, blocks), b1 = run(lds_in_fma<1, 0>, blocks), l1 = run(lds_in_fma<1, 1>, blocks);
    printf("(a) 100 chain-free v_fma_f64 + k broadcast ds_read_b128 in one batch: cycles per group\n");
    printf("    k = 0 %8.2f   (%.2f per FMA)\n", f0, f0 / 100);
    printf("    k = 4 %8.2f   %+6.2f per added read\n", f4, (f4 - f0) / 4);
    printf("    k = 8 %8.2f   %+6.2f per added read\n", f8, (f8 - f0) / 8);
    printf("    k =12 %8.2f   %+6.2f per added read\n", f12, (f12 - f0) / 12);
    printf("    k = 1 %8.2f   %+6.2f\n", b1, b1 - f0);
    printf("(b) the same with one lane-indexed ds_read_b128 (base + 16 (lane & 15))\n");
    printf("    k = 1 %8.2f   %+6.2f\n", l1, l1 - f0);
    printf("    eleven broadcast reads against one lane-indexed read, interpolated at k = 11: %+.2f cycles per knot\n",
           f8 + (f12 - f8) * 0.75 - l1);
    const double s_d = run(dpp21<0, 0, 1>, blocks), s_p = run(dpp21<0, 0, 0>, blocks), i0d = run(dpp21<1, 0, 1>, blocks), i0p = run(dpp21<1, 0, 0>, blocks),
                 i1d = run(dpp21<1, 1, 1>, blocks), i1p = run(dpp21<1, 1, 0>, blocks), i2d = run(dpp21<1, 2, 1>, blocks), i2p = run(dpp21<1, 2, 0>, blocks);
    printf("(c) 21 v_fmac_f64_dpp row_newbcast into three accumulators: cycles per group, DPP | plain v_fma_f64 in the same order | difference\n");
    printf("    accumulator after accumulator (7 + 7 + 7)        %8.2f | %8.2f | %+6.2f\n", s_d, s_p, s_d - s_p);
    printf("    the three interleaved                            %8.2f | %8.2f | %+6.2f\n", i0d, i0p, i0d - i0p);
    printf("    interleaved, 1 independent FMA after each (42)   %8.2f | %8.2f | %+6.2f\n", i1d, i1p, i1d - i1p);
    printf("    interleaved, 2 independent FMAs after each (63)  %8.2f | %8.2f | %+6.2f\n", i2d, i2p, i2d - i2p);
  }
  return 0;
}
