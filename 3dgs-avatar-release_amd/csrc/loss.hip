// loss.hip -- image-side L1 loss (replaces utils/loss_utils.py:21-22,
// torch.abs(network_output - gt).mean(), and its autograd chain of ~10 elementwise kernels).
// One streaming pass writes d(loss)/d(network_output) = sign(x - y) / n and one partial sum of
// |x - y| per block; a second, single-block pass adds the partials -- the schemes of block_sum (waves
// pairwise) and ordered_final_kernel in ordered_sum.h.  No atomics: the result is bitwise reproducible.
#include "common.h"
#include "ordered_sum.h"
#include "boundary.h"
#include <math.h>

#define L1_THREADS 256
#define L1_MAX_BLOCKS 1024

__device__ __forceinline__ float sgn_over_n(float d, float inv_n) { return d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f); }

__global__ __launch_bounds__(L1_THREADS) void l1_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                int64_t n, float inv_n, float* __restrict__ grad,
                                                                float* __restrict__ partial) {
    __shared__ float ws[L1_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float acc = 0.f;
    const int64_t n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* y4 = reinterpret_cast<const float4*>(y);
    float4* g4 = reinterpret_cast<float4*>(grad);
    const int64_t stride = (int64_t)gridDim.x * L1_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * L1_THREADS + tid; i < n4; i += stride) {
        const float4 a = x4[i], b = y4[i];
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
        acc += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
        g4[i] = make_float4(sgn_over_n(d0, inv_n), sgn_over_n(d1, inv_n), sgn_over_n(d2, inv_n), sgn_over_n(d3, inv_n));
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {  // the last n mod 4 elements
        const int64_t i = (n4 << 2) + tid;
        const float d = x[i] - y[i];
        acc += fabsf(d);
        grad[i] = sgn_over_n(d, inv_n);
    }
    acc = wave_sum(acc);  // (block_sum<L1_THREADS, WavesPairwise> in this kernel's own text: see l1_final_kernel)
    if (lane == 0) ws[wid] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// The second pass of the L1 / BCE / SSIM means, one workgroup: what ordered_final_kernel<L1_THREADS, WavesPairwise, true>
// computes for q = 0.  It and l1_partial_kernel run in every training step and keep their own text: written with
// block_sum they compile to one instruction less, and the step's kernels are held to the instructions they were measured with.
__global__ __launch_bounds__(L1_THREADS) void l1_final_kernel(const float* __restrict__ partial, int nparts, float inv_n,
                                                              float* __restrict__ loss) {
    __shared__ float ws[L1_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float acc = 0.f;
    for (int i = tid; i < nparts; i += L1_THREADS) acc += partial[i];
    acc = wave_sum(acc);
    if (lane == 0) ws[wid] = acc;
    __syncthreads();
    if (tid == 0) loss[0] = ((ws[0] + ws[1]) + (ws[2] + ws[3])) * inv_n;  // (WavesPairwise)
}

// Mask loss, BCE form (train.py:146-148): F.binary_cross_entropy(torch.clamp(x, 1e-3, 1 - 1e-3), y), mean over all
// elements, and its gradient w.r.t. x: (p - y) / (p (1 - p)) / n inside the clamp range, 0 outside.  Same
// two-stage ordered reduction as the L1 loss.
__global__ __launch_bounds__(L1_THREADS) void bce_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 int64_t n, float inv_n, float* __restrict__ grad,
                                                                 float* __restrict__ partial) {
    __shared__ float ws[L1_THREADS / 64];
    const int tid = threadIdx.x;
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * L1_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * L1_THREADS + tid; i < n; i += stride) {
        const float xv = x[i], t = y[i];
        const float p = fminf(fmaxf(xv, 1.0e-3f), 1.0f - 1.0e-3f);
        acc -= t * logf(p) + (1.0f - t) * logf(1.0f - p);
        const bool inside = xv >= 1.0e-3f && xv <= 1.0f - 1.0e-3f;  // clamp passes the gradient on its closed range
        grad[i] = inside ? (p - t) / (p * (1.0f - p)) * inv_n : 0.f;
    }
    const float s = block_sum<L1_THREADS, WavesPairwise>(acc, ws);
    if (tid == 0) partial[blockIdx.x] = s;
}

static int l1_blocks(int64_t n) {
    const int64_t want = ((n >> 2) + L1_THREADS - 1) / L1_THREADS;
    return (int)(want < 1 ? 1 : (want > L1_MAX_BLOCKS ? L1_MAX_BLOCKS : want));
}

static size_t l1_ws_bytes(int64_t n) { return (size_t)l1_blocks(n) * sizeof(float); }

static int launch_bce_loss(const float* x, const float* y, int64_t n, float* loss, float* grad, float* partial, hipStream_t s) {
    const int blocks = l1_blocks(n);
    const float inv_n = 1.0f / (float)n;
    StageScope st("bce_loss", s);
    hipLaunchKernelGGL(bce_partial_kernel, dim3(blocks), dim3(L1_THREADS), 0, s, x, y, n, inv_n, grad, partial);
    GS_LAUNCH_CHECK("bce_loss.partial", 0, s);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(L1_THREADS), 0, s, partial, blocks, inv_n, loss);
    GS_LAUNCH_CHECK("bce_loss.final", 0, s);
    return GS_OK;
}

// The same sum for MANY partials (the fused L1: one per quadrant, 16 384 at 1024 x 1024): one workgroup of 1024 threads, every
// thread's loads requested eight at a time before they are added (as a plain strided loop over 256 threads the launch took
// 16 us at config 3: 64 dependent round trips per thread).  Fixed order: thread t adds its partials t, t + 1024, ... in
// index order, the threads' sums go through the DPP ladder and the 16 wave sums are added in wave order STARTING FROM 0
// (0 + w0 + w1 ...: one addition more than block_sum<1024, WavesInOrder>, under which sixteen -0 would stay -0; the
// kernel runs in every training step and keeps its text).
__global__ __launch_bounds__(1024) void loss_final_wide_kernel(const float* __restrict__ partial, int nparts, float inv_n,
                                                               float* __restrict__ loss) {
    __shared__ float ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float acc = 0.f;
    for (int i0 = tid; i0 < nparts; i0 += 8 * 1024) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = (i0 + u * 1024 < nparts) ? partial[i0 + u * 1024] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u];
    }
    acc = wave_sum(acc);
    if (lane == 0) ws[wid] = acc;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; w++) t += ws[w];
        loss[0] = t * inv_n;
    }
}

int launch_loss_final(const float* partial, int nparts, float inv_n, float* loss, hipStream_t s) {
    // (no stage scope of its own: the fused L1 calls it from inside the render_fwd stage, and stage scopes do not nest)
    hipLaunchKernelGGL(loss_final_wide_kernel, dim3(1), dim3(1024), 0, s, partial, nparts, inv_n, loss);
    GS_LAUNCH_CHECK("loss_final", 0, s);
    return GS_OK;
}

static int launch_l1_loss(const float* x, const float* y, int64_t n, float* loss, float* grad, float* partial, hipStream_t s) {
    const int blocks = l1_blocks(n);
    const float inv_n = 1.0f / (float)n;
    StageScope st("l1_loss", s);
    hipLaunchKernelGGL(l1_partial_kernel, dim3(blocks), dim3(L1_THREADS), 0, s, x, y, n, inv_n, grad, partial);
    GS_LAUNCH_CHECK("l1_loss.partial", 0, s);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(L1_THREADS), 0, s, partial, blocks, inv_n, loss);
    GS_LAUNCH_CHECK("l1_loss.final", 0, s);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------
// SSIM (utils/loss_utils.py:27-67: 11x11 Gaussian window, sigma 1.5, zero
// padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements) with its gradient w.r.t. the first image.
// The reference runs five depthwise conv2d launches plus ~15 elementwise ones and lets autograd replay
// them backwards.  Here: one forward kernel (32x32 output tile per workgroup, 42x42 halo tiles of both
// images in LDS, the 121-tap window applied as two 11-tap passes, five moments at once) that also
// emits the three partial-derivative maps the backward needs, and one backward kernel that filters
// those three maps with the same window and combines them with the images.  Reductions are two-stage
// and ordered: bitwise reproducible.
// ---------------------------------------------------------------------------------------------
#define SS_T 32            // output tile edge (32 x 32 outputs per workgroup of 256 threads: four per thread)
#define SS_NT 256
#define SS_R 5             // window radius
#define SS_H (SS_T + 2 * SS_R)  // halo tile edge (42)
#define SS_C1 0.0001f
#define SS_C2 0.0009f

struct SsimWindow { float w[11]; };

__global__ __launch_bounds__(SS_NT) void ssim_fwd_kernel(int H, int W, const float* __restrict__ img1,
                                                         const float* __restrict__ img2, SsimWindow win,
                                                         float* __restrict__ dm_dmu1, float* __restrict__ dm_ds1,
                                                         float* __restrict__ dm_ds12, float* __restrict__ partial) {
    // the halo tiles live in the front of hx: every thread has its inputs in registers before the first hx word is
    // written (28 KB per workgroup instead of 42: one more workgroup per CU to hide the tile loads behind)
    __shared__ float hx[5][SS_H][SS_T + 1];
    float (*t1)[SS_H + 1] = reinterpret_cast<float (*)[SS_H + 1]>(&hx[0][0][0]);
    float (*t2)[SS_H + 1] = reinterpret_cast<float (*)[SS_H + 1]>(&hx[0][0][0] + SS_H * (SS_H + 1));
    static_assert(2 * SS_H * (SS_H + 1) <= 5 * SS_H * (SS_T + 1), "halo tiles fit in hx");
    __shared__ float ws[SS_NT / 64];
    const int tid = threadIdx.x, tx = tid % SS_T, ty = tid / SS_T;  // ty in 0..7: rows 4 ty .. 4 ty + 3
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const size_t plane = (size_t)blockIdx.z * H * W;
    // halo tiles: 42 rows of 42, a row per trip of 64 threads (no integer division).  All of a thread's 22 loads are
    // requested before the first is stored to LDS (as a plain loop the compiler waits for every load in turn: 22 dependent
    // round trips in front of the arithmetic of every workgroup)
    {
        constexpr int TRIPS = (SS_H + SS_NT / 64 - 1) / (SS_NT / 64);
        const int c = tid & 63;
        float v1[TRIPS], v2[TRIPS];
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const int r = (tid >> 6) + u * (SS_NT / 64);
            const int y = y0 + r - SS_R, x = x0 + c - SS_R;
            const bool in = r < SS_H && c < SS_H && y >= 0 && y < H && x >= 0 && x < W;  // zero padding (conv2d padding = 5)
            v1[u] = in ? img1[plane + (size_t)y * W + x] : 0.f;
            v2[u] = in ? img2[plane + (size_t)y * W + x] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const int r = (tid >> 6) + u * (SS_NT / 64);
            if (r < SS_H && c < SS_H) { t1[r][c] = v1[u]; t2[r][c] = v2[u]; }
        }
    }
    __syncthreads();
    // horizontal pass, 42 rows x 32 columns, five moments: a thread takes 8 adjacent columns of one row and slides the
    // window over the 18 inputs it holds in registers (one LDS read per input instead of one per tap)
    {
        const int r = tid >> 2, c0 = (tid & 3) * 8;
        float a[18], b[18], aa[18], bb[18], ab[18];
        if (r < SS_H) {
#pragma unroll
            for (int j = 0; j < 18; j++) {
                a[j] = t1[r][c0 + j];
                b[j] = t2[r][c0 + j];
                aa[j] = a[j] * a[j];
                bb[j] = b[j] * b[j];
                ab[j] = a[j] * b[j];
            }
        }
        __syncthreads();  // the tiles are in registers: hx may overwrite them
        if (r < SS_H) {
#pragma unroll
            for (int o = 0; o < 8; o++) {
                float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const float w = win.w[k];
                    m1 += w * a[o + k];
                    m2 += w * b[o + k];
                    e11 += w * aa[o + k];
                    e22 += w * bb[o + k];
                    e12 += w * ab[o + k];
                }
                hx[0][r][c0 + o] = m1; hx[1][r][c0 + o] = m2; hx[2][r][c0 + o] = e11; hx[3][r][c0 + o] = e22;
                hx[4][r][c0 + o] = e12;
            }
        }
    }
    __syncthreads();
    // vertical pass: a thread takes 4 adjacent rows of one column (14 inputs per moment in registers)
    float val = 0.f;
    {
        const int oy0 = ty * 4;  // ty = tid / 32 in 0..7
        float acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; m++) {
            float v[14];
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = hx[m][oy0 + j][tx];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) sum += win.w[k] * v[o + k];
                acc[m][o] = sum;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const float mu1 = acc[0][o], mu2 = acc[1][o], e11 = acc[2][o], e22 = acc[3][o], e12 = acc[4][o];
            const int x = x0 + tx, y = y0 + oy0 + o;
            if (x < W && y < H) {
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
                const float A = 2.f * mu12 + SS_C1, B = 2.f * s12 + SS_C2;
                const float C = mu1_sq + mu2_sq + SS_C1, D = s1 + s2 + SS_C2;
                const float inv_cd = 1.0f / (C * D);
                const float v = A * B * inv_cd;
                val += v;
                if (dm_dmu1) {
                    // ssim as a function of (mu1, E[x^2], E[xy]) of this window; s1 and s12 depend on mu1 too
                    const float d_s1 = -v / D;              // d ssim / d s1   = -A B / (C D^2)
                    const float d_s12 = 2.f * A * inv_cd;   // d ssim / d s12  =  2 A / (C D)
                    const float d_mu1 = 2.f * mu2 * B * inv_cd - 2.f * mu1 * v / C - 2.f * mu1 * d_s1 - mu2 * d_s12;
                    const size_t oo = plane + (size_t)y * W + x;
                    dm_dmu1[oo] = d_mu1;
                    dm_ds1[oo] = d_s1;
                    dm_ds12[oo] = d_s12;
                }
            }
        }
    }
    val = block_sum<SS_NT, WavesPairwise>(val, ws);
    if (tid == 0) partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = val;
}

// dL/dimg1(p) = g/n * sum_q w(q - p) [ dm_dmu1(q) + 2 img1(p) dm_ds1(q) + img2(p) dm_ds12(q) ]
__global__ __launch_bounds__(SS_NT) void ssim_bwd_kernel(int H, int W, const float* __restrict__ img1,
                                                         const float* __restrict__ img2, SsimWindow win,
                                                         const float* __restrict__ dm_dmu1,
                                                         const float* __restrict__ dm_ds1,
                                                         const float* __restrict__ dm_ds12,
                                                         const float* __restrict__ dL_dssim, float inv_n,
                                                         float* __restrict__ dL_dimg1) {
    // (hx overwrites the front of t once every thread holds its inputs in registers: 22 KB per workgroup, not 38)
    __shared__ float t[3][SS_H][SS_H + 1];
    float (*hx)[SS_H][SS_T + 1] = reinterpret_cast<float (*)[SS_H][SS_T + 1]>(&t[0][0][0]);
    static_assert(SS_T + 1 <= SS_H + 1, "hx fits in t");
    const int tid = threadIdx.x, tx = tid % SS_T, ty = tid / SS_T;
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const size_t plane = (size_t)blockIdx.z * H * W;
    {  // (all 33 loads of a thread requested before the first LDS store: see ssim_fwd_kernel)
        constexpr int TRIPS = (SS_H + SS_NT / 64 - 1) / (SS_NT / 64);
        const int c = tid & 63;
        float v0[TRIPS], v1[TRIPS], v2[TRIPS];
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const int r = (tid >> 6) + u * (SS_NT / 64);
            const int y = y0 + r - SS_R, x = x0 + c - SS_R;
            const bool in = r < SS_H && c < SS_H && y >= 0 && y < H && x >= 0 && x < W;  // windows centred outside the image do not exist
            const size_t o = plane + (size_t)y * W + x;
            v0[u] = in ? dm_dmu1[o] : 0.f;
            v1[u] = in ? dm_ds1[o] : 0.f;
            v2[u] = in ? dm_ds12[o] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const int r = (tid >> 6) + u * (SS_NT / 64);
            if (r < SS_H && c < SS_H) { t[0][r][c] = v0[u]; t[1][r][c] = v1[u]; t[2][r][c] = v2[u]; }
        }
    }
    __syncthreads();
    {
        // horizontal pass: 8 adjacent columns of one row per thread, the 18 inputs of each map in registers
        const int r = tid >> 2, c0 = (tid & 3) * 8;
        float v[3][18];
        if (r < SS_H) {
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int j = 0; j < 18; j++) v[m][j] = t[m][r][c0 + j];
        }
        __syncthreads();  // the maps are in registers: hx may overwrite them
        if (r < SS_H) {
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int o = 0; o < 8; o++) {
                    float sum = 0.f;
#pragma unroll
                    for (int k = 0; k < 11; k++) sum += win.w[k] * v[m][o + k];
                    hx[m][r][c0 + o] = sum;
                }
        }
    }
    __syncthreads();
    const float g = dL_dssim[0] * inv_n;
    {
        // vertical pass: 4 adjacent rows of one column per thread
        const int oy0 = ty * 4;
        float f[3][4];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float v[14];
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = hx[m][oy0 + j][tx];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) sum += win.w[k] * v[o + k];
                f[m][o] = sum;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = x0 + tx, y = y0 + oy0 + o;
            if (x < W && y < H) {
                const size_t oo = plane + (size_t)y * W + x;
                dL_dimg1[oo] = g * (f[0][o] + 2.f * img1[oo] * f[1][o] + img2[oo] * f[2][o]);
            }
        }
    }
}

static SsimWindow ssim_window() {
    // utils/loss_utils.py:27-29: exp(-(x - 5)^2 / (2 * 1.5^2)) evaluated in double, stored as fp32, normalised in fp32.
    // The divisor is torch's `gauss.sum()`, which for these eleven values is the correctly rounded sum (3.7592328;
    // adding them one by one in fp32 gives 3.7592325): pinned by the reference's own window in tests/golden/losses.npz.
    SsimWindow w;
    double sd = 0.0;
    for (int k = 0; k < 11; k++) {
        w.w[k] = (float)exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        sd += (double)w.w[k];
    }
    const float s = (float)sd;
    for (int k = 0; k < 11; k++) w.w[k] /= s;
    return w;
}

static inline int ssim_tiles(int v) { return (v + SS_T - 1) / SS_T; }
static size_t ssim_ws_bytes(int C, int H, int W) { return (size_t)C * ssim_tiles(H) * ssim_tiles(W) * sizeof(float); }

static int launch_ssim_forward(int C, int H, int W, const float* img1, const float* img2, float* ssim_out, float* dm_dmu1,
                               float* dm_ds1, float* dm_ds12, float* partial, hipStream_t s) {
    const dim3 grid(ssim_tiles(W), ssim_tiles(H), C);
    StageScope st("ssim_fwd", s);
    hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(SS_NT), 0, s, H, W, img1, img2, ssim_window(), dm_dmu1, dm_ds1,
                       dm_ds12, partial);
    GS_LAUNCH_CHECK("ssim.forward", 0, s);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(L1_THREADS), 0, s, partial, (int)(grid.x * grid.y * grid.z),
                       1.0f / ((float)C * (float)H * (float)W), ssim_out);
    GS_LAUNCH_CHECK("ssim.final", 0, s);
    return GS_OK;
}

static int launch_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* dm_dmu1,
                                const float* dm_ds1, const float* dm_ds12, const float* dL_dssim, float* dL_dimg1,
                                hipStream_t s) {
    const dim3 grid(ssim_tiles(W), ssim_tiles(H), C);
    StageScope st("ssim_bwd", s);
    hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(SS_NT), 0, s, H, W, img1, img2, ssim_window(), dm_dmu1, dm_ds1,
                       dm_ds12, dL_dssim, 1.0f / ((float)C * (float)H * (float)W), dL_dimg1);
    GS_LAUNCH_CHECK("ssim.backward", 0, s);
    return GS_OK;
}

extern "C" {

int gs_l1_loss_workspace_bytes(int64_t n, size_t* out) {
    if (!out || n < 0) return GS_E_BAD_ARG;
    *out = l1_ws_bytes(n);
    return GS_OK;
}
int gs_l1_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace, size_t workspace_bytes,
               void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n <= 0 || !x || !y || !loss || !dL_dx || !workspace) return GS_E_BAD_ARG;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(dL_dx, 16)) return GS_E_BAD_ARG;  // float4 accesses
    if (workspace_bytes < l1_ws_bytes(n)) return GS_E_WORKSPACE;
    return launch_l1_loss(x, y, n, loss, dL_dx, (float*)workspace, (hipStream_t)stream);
}

int gs_bce_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace, size_t workspace_bytes,
                void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n <= 0 || !x || !y || !loss || !dL_dx || !workspace) return GS_E_BAD_ARG;
    if (workspace_bytes < l1_ws_bytes(n)) return GS_E_WORKSPACE;
    return launch_bce_loss(x, y, n, loss, dL_dx, (float*)workspace, (hipStream_t)stream);
}

int gs_ssim_workspace_bytes(int32_t C, int32_t H, int32_t W, size_t* out) {
    if (!out || C <= 0 || H <= 0 || W <= 0) return GS_E_BAD_ARG;
    *out = ssim_ws_bytes(C, H, W);
    return GS_OK;
}
int gs_ssim_forward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_out, float* dm_dmu1,
                    float* dm_dsigma1_sq, float* dm_dsigma12, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !ssim_out || !workspace) return GS_E_BAD_ARG;
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr)) return GS_E_BAD_ARG;
    if (workspace_bytes < ssim_ws_bytes(C, H, W)) return GS_E_WORKSPACE;
    return launch_ssim_forward(C, H, W, img1, img2, ssim_out, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, (float*)workspace,
                               (hipStream_t)stream);
}
int gs_ssim_backward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* dm_dmu1,
                     const float* dm_dsigma1_sq, const float* dm_dsigma12, const float* dL_dssim, float* dL_dimg1,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dssim || !dL_dimg1)
        return GS_E_BAD_ARG;
    return launch_ssim_backward(C, H, W, img1, img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dssim, dL_dimg1,
                                (hipStream_t)stream);
}

}  // extern "C"
