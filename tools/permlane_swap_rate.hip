// Microbenchmark: issue rate of the gfx950 lane-swap instructions (v_permlane16_swap_b32 / v_permlane32_swap_b32, wave64)
// next to v_add_f32 and to the ds_bpermute_b32 they replace in render_bwd's ring fold.  Eight registers per lane = four
// independent pairs, visited so that a swap never reads a register written less than three instructions earlier (the hardware
// wants two wait states between a VALU write and a swap's read of it).
// Build / run:  hipcc -O3 --offload-arch=gfx950 tools/permlane_swap_rate.hip -o permlane_swap_rate.bin && ./permlane_swap_rate.bin
#include <hip/hip_runtime.h>
#include <stdio.h>
template <int MODE>
__global__ __launch_bounds__(256) void k(float* out, int iters, float seed) {
    float a[8];
    for (int i = 0; i < 8; i++) a[i] = seed + i + threadIdx.x * 1e-3f;
    int idx = (int)((threadIdx.x ^ 16) << 2);
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                if (MODE == 0) asm volatile("v_add_f32 %0, %0, %0\n\tv_add_f32 %1, %1, %1" : "+v"(a[i]), "+v"(a[i + 1]));
                if (MODE == 1) asm volatile("v_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3" : "+v"(a[i]), "+v"(a[i + 1]), "+v"(a[(i + 4) & 7]), "+v"(a[(i + 5) & 7]));
                if (MODE == 2) asm volatile("v_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3" : "+v"(a[i]), "+v"(a[i + 1]), "+v"(a[(i + 4) & 7]), "+v"(a[(i + 5) & 7]));
                // the fold's pattern: a swap and the add of its two results (the add waits for the swap)
                if (MODE == 3) asm volatile("v_permlane16_swap_b32 %0, %1\n\tv_add_f32 %0, %0, %1" : "+v"(a[i]), "+v"(a[i + 1]));
                if (MODE == 4) asm volatile("v_permlane32_swap_b32 %0, %1\n\tv_add_f32 %0, %0, %1" : "+v"(a[i]), "+v"(a[i + 1]));
                // what the fold used until now: an LDS exchange and an add
                if (MODE == 5) asm volatile("ds_bpermute_b32 %1, %2, %0\n\ts_waitcnt lgkmcnt(0)\n\tv_add_f32 %0, %0, %1" : "+v"(a[i]), "+v"(a[i + 1]) : "v"(idx));
            }
        }
    }
    float s = 0;
    for (int i = 0; i < 8; i++) s += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
template <int MODE>
void run(const char* name, int blocks_per_cu) {
    int iters = 2048;
    int nb = 256 * blocks_per_cu;
    float* d; (void)hipMalloc(&d, (size_t)nb * 256 * 4);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(nb), dim3(256), 0, 0, d, 16, 1.0f);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(nb), dim3(256), 0, 0, d, iters, 1.0f);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    // instructions per SIMD: nb blocks of 4 waves over 256 CUs x 4 SIMDs, 32 instructions per wave and iteration
    double per_simd = (double)nb * 4 * iters * 32.0 / 1024.0;
    printf("%-34s blocks/CU=%d  %.3f ms  cycles/instr/SIMD @2.4GHz: %.2f\n", name, blocks_per_cu, ms, ms * 1e6 / per_simd * 2.4);
    (void)hipFree(d);
}
int main() {
    for (int b : {2, 8}) {
        run<0>("v_add_f32", b);
        run<1>("v_permlane16_swap_b32", b);
        run<2>("v_permlane32_swap_b32", b);
        run<3>("permlane16_swap + dependent add", b);
        run<4>("permlane32_swap + dependent add", b);
        run<5>("ds_bpermute_b32 + wait + add", b);
    }
    return 0;
}
