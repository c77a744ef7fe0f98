// ordered_sum.h -- the wave primitives and the fixed-order sums every module shares (internal).  "Fixed order" is the
// reproducibility promise of the library: the same input gives the same bits, run after run.  Each primitive states its
// order of addition once, here; the modules refer to it by name.  The sums hold additions only (the one product, the
// final kernel's optional scale, feeds no sum): this file is compiled into translation units with and without FMA
// contraction, and must leave nothing to contract.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

// a word range some kernel clears on the side (grid-stride), saving a fill launch
struct ZeroJob { uint32_t* ptr; int words; };
__device__ __forceinline__ void zero_job(const ZeroJob z) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < z.words; k += gridDim.x * blockDim.x) z.ptr[k] = 0u;
}

// Inclusive prefix sum over the 64 lanes of a wave by DPP row shifts and row broadcasts (six dependent VALU instructions;
// a __shfl_up ladder is six ds_bpermute round trips through the LDS unit, ~10 x the latency -- and the short binning
// kernels are nothing but latency).  Every lane must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    x += dpp_or_zero<0x111, 0xF>(x);  // row_shr:1
    x += dpp_or_zero<0x112, 0xF>(x);  // row_shr:2
    x += dpp_or_zero<0x114, 0xF>(x);  // row_shr:4
    x += dpp_or_zero<0x118, 0xF>(x);  // row_shr:8
    x += dpp_or_zero<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
    x += dpp_or_zero<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
    return x;
}
// the same inside every row of 16 lanes
__device__ __forceinline__ uint32_t row_scan_incl(uint32_t x) {
    x += dpp_or_zero<0x111, 0xF>(x);
    x += dpp_or_zero<0x112, 0xF>(x);
    x += dpp_or_zero<0x114, 0xF>(x);
    x += dpp_or_zero<0x118, 0xF>(x);
    return x;
}
__device__ __forceinline__ unsigned long long wave_scan_incl(unsigned long long x) {
    // (two 32-bit ladders would lose the carries: shift the halves, add as 64-bit)
#define GS_SCAN64_STEP(CTRL, MASK)                                                                           \
    x += (unsigned long long)dpp_or_zero<CTRL, MASK>((uint32_t)x) |                                          \
         ((unsigned long long)dpp_or_zero<CTRL, MASK>((uint32_t)(x >> 32)) << 32);
    GS_SCAN64_STEP(0x111, 0xF) GS_SCAN64_STEP(0x112, 0xF) GS_SCAN64_STEP(0x114, 0xF) GS_SCAN64_STEP(0x118, 0xF)
    GS_SCAN64_STEP(0x142, 0xA) GS_SCAN64_STEP(0x143, 0xC)
#undef GS_SCAN64_STEP
    return x;
}

// Wave-wide sum / max / min by the same ladder (the result is wave-uniform: lane 63 of the inclusive scan).
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(x), 63); }
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
    x = wave_scan_incl(x);
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63) |
           ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63) << 32);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
    x = max(x, dpp_or_zero<0x111, 0xF>(x));
    x = max(x, dpp_or_zero<0x112, 0xF>(x));
    x = max(x, dpp_or_zero<0x114, 0xF>(x));
    x = max(x, dpp_or_zero<0x118, 0xF>(x));
    x = max(x, dpp_or_zero<0x142, 0xA>(x));
    x = max(x, dpp_or_zero<0x143, 0xC>(x));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) { return ~wave_max(~x); }
// (float: the sum is taken in the ladder's fixed order -- the same bits on every run; lane 63 of the scan holds it)
__device__ __forceinline__ float wave_scan_incl(float x) {
#define GS_FSUM_STEP(CTRL, MASK) x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, MASK, 0xF, false));
    GS_FSUM_STEP(0x111, 0xF) GS_FSUM_STEP(0x112, 0xF) GS_FSUM_STEP(0x114, 0xF) GS_FSUM_STEP(0x118, 0xF)
    GS_FSUM_STEP(0x142, 0xA) GS_FSUM_STEP(0x143, 0xC)
#undef GS_FSUM_STEP
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_scan_incl(x)), 63));
}

// ---- block_sum: the sum of one float per thread over a workgroup of T threads.  Every wave adds its lanes by the DPP
// ladder (wave_sum), the wave sums w0, w1, .. go through `ws` (LDS, T / 64 floats, not in use by anyone else) and are
// added in the order the tag names:
//   WavesInOrder    ((w0 + w1) + w2) + w3 ...
//   WavesPairwise   (w0 + w1) + (w2 + w3)        (T = 256 only)
// The two differ in the last bit; a call site keeps the one it was written with.  Every thread must call it (it holds a
// barrier) and every thread gets the sum.
struct WavesInOrder {};
struct WavesPairwise {};
template <int T, class Order>
__device__ __forceinline__ float block_sum(float x, float* ws) {
    static_assert(T % 64 == 0 && (!std::is_same<Order, WavesPairwise>::value || T == 256), "whole waves; pairwise: four");
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    x = wave_sum(x);
    if (lane == 0) ws[wid] = x;
    __syncthreads();
    if constexpr (std::is_same<Order, WavesPairwise>::value) return (ws[0] + ws[1]) + (ws[2] + ws[3]);
    float s = ws[0];
#pragma unroll
    for (int w = 1; w < T / 64; w++) s += ws[w];
    return s;
}
// strided_sum: thread t of T adds p[t], p[t + T], .. below n, in index order, starting from 0
template <int T>
__device__ __forceinline__ float strided_sum(const float* __restrict__ p, int n) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += T) acc += p[i];
    return acc;
}
// ordered_final_kernel: out[q] = (partial[q nb + 0 .. nb - 1]: strided_sum, then block_sum in `Order`) [* scale], q =
// blockIdx.x -- the second pass of every two-pass sum.  SCALED = false: no multiply at all (a product by 1 is not free
// of consequences for a NaN's payload).
template <int T, class Order, bool SCALED>
__global__ __launch_bounds__(T) void ordered_final_kernel(const float* __restrict__ partial, int nb, float scale,
                                                          float* __restrict__ out) {
    __shared__ float ws[T / 64];
    const float s = block_sum<T, Order>(strided_sum<T>(partial + (size_t)blockIdx.x * nb, nb), ws);
    if (threadIdx.x == 0) out[blockIdx.x] = SCALED ? s * scale : s;
}

// runs64_sum: the sum of p[0 .. nb) in double by a workgroup of ONE wave.  Lane l adds its contiguous run of ceil(nb / 64)
// elements in index order, starting from 0; lane 0 adds the 64 runs in lane order, starting from 0.  `run`: LDS, 64
// doubles.  Valid in thread 0 (0 elsewhere); every thread must call it.
__device__ __forceinline__ double runs64_sum(const double* __restrict__ p, int nb, double* run) {
    const int l = threadIdx.x;
    const int per = (nb + 63) / 64, b0 = min(nb, l * per), b1 = min(nb, b0 + per);
    double a = 0.0;
    for (int b = b0; b < b1; b++) a += p[b];
    run[l] = a;
    __syncthreads();
    double s = 0.0;
    if (l == 0)
        for (int k = 0; k < 64; k++) s += run[k];
    return s;
}
