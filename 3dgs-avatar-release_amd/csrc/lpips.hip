// lpips.hip -- the perceptual loss of the avatar model (train.py:28,62-64,127-138 `lpips.LPIPS(net='vgg')`, and the test
// metric of utils/general_utils.py:279-291) as one fused op on the exact-fp32 MFMA: thirteen implicit-GEMM convolutions
// whose kernel takes the crop's H and W as run-time arguments (the foreground crop changes with every frame), both images
// of a call through every layer in one launch, and a backward to the image without atomics or memsets.
//
// NOTHING of the `lpips` package or of torchvision was available when this was written: the structure below is RECALLED
// from the public packages (lpips 0.1.x, torchvision's vgg16) and could not be checked against them.
//
// Spec (fp32 throughout).  Images are (3, H, W) with a channel stride and a row stride (a crop of a larger image is read in
// place), 16 <= H, W <= 2048.
//   input    x <- 2 x - 1 with `normalize`; then (x - shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448,
//            .450) unless the state dict carries its own.  Folded into the first layer's operand load; the zero padding of
//            the first convolution pads the TRANSFORMED image.
//   trunk    VGG16 features[0:30]: thirteen 3x3 convolutions (stride 1, zero padding 1), each followed by bias and ReLU,
//            channels 3>64>64 | 64>128>128 | 128>256>256>256 | 256>512>512>512 | 512>512>512>512, `|` a 2x2 stride-2
//            max-pool with floor.  The five taps are the ReLU outputs in front of each pool and the last one
//            (relu1_2, 2_2, 3_3, 4_3, 5_3): layers 1, 3, 6, 9, 12 of the thirteen.
//   head     per tap k: n(x) = x / (sqrt(sum_c x^2) + 1e-10), d = (n(f0) - n(f1))^2, s_k = the mean over the pixels of
//            sum_c lin_k[c] d[c] (lin_k a C>1 1x1 convolution without bias; the dropout in front of it is the identity: the
//            network is always in eval mode).  loss = sum_k s_k.
// Backward, to the images only (every weight is frozen): the head's gradient into each tap through n(.), the 1e-10
//   included (a pixel whose features are ALL zero takes no gradient through the norm, where torch's sqrt gives NaN); ReLU as
//   a > 0 on the saved post-activation (zero takes zero, as torch does); the pool to the FIRST maximum in row-major window
//   order, as torch does; backward-data convolution as a gather with the flipped, transposed weights; the input
//   transform's factor.  No atomics, no memsets; every sum -- the spatial means included -- in an order fixed by the shapes
//   alone: the same inputs give the same bits on every run, stream and device.
// What the forward saves, per image that needs a gradient: its thirteen post-activations (ReLU masks, pool arguments) and
//   the head's gradient into its five taps for a unit dL/dloss (the other image's taps are gone by the time of the
//   backward; the backward multiplies dL/dloss in at the very end).  An image that needs no gradient saves nothing: its maps
//   live in two transient buffers that alternate.
// Kernels.  Feature maps are channels-last ((H, W, C): K is contiguous for the implicit GEMM).
//   lp_conv_kernel   ONE kernel for both directions: out[p][n] = sum_tap sum_k in[p + tap][k] w[tap][k][n] over a tile of 8 x 8
//                    pixels and 16 nt (nt = 1, 2, 4) output channels; 4 waves, each 16 pixels (two tile rows) x 16 nt channels
//                    on __builtin_amdgcn_mfma_f32_16x16x4f32.  Per chunk of LP_KC input channels the 10 x 10 halo and the nine
//                    taps' weights are staged in LDS (zero fill at the image's edges and past K and N: H and W never select
//                    another kernel).  Forward: bias and ReLU in the epilogue; the first layer reads the image through its
//                    strides and transforms it on the way.  Backward: w = the flipped, transposed weights, the a > 0 mask
//                    multiplied in at the operand load; the first layer writes the image gradient, times the transform's
//                    factor and dL/dloss.  An output's sum: a chunk's 9 x LP_KC products in one MFMA chain (tap by tap, k by k),
//                    the chunks' sums added in order -- whatever nt is.
//                    nt is the largest of 4, 2, 1 that still gives 256 workgroups (a function of the shapes alone): conv4_x
//                    and conv5_x have few pixels and tile over the output channels instead (DESIGN.md has the counts).
//   lp_pool_kernel, lp_unpool_kernel   the 2x2 max-pool, and its backward as a gather that also adds the head's gradient
//                    into the tap it comes from (every element written once).
//   lp_head_kernel   a wave per pixel, 16 pixels per wave in order, 64 per workgroup: the pixel's term, the head's
//                    gradients, one partial per workgroup (waves in index order).
//   lp_sum_kernel    one workgroup: per tap the partials in a fixed strided order, then the five terms in order.  The
//                    pixel sums of both kernels are compensated (Kahan): fp32 operations in a fixed order.
//   lp_pack_kernel   the weights for both directions, once, when they are loaded.
#include "common.h"
#include "boundary.h"

#define LP_THREADS 256
#define LP_TS 8     // tile edge: 64 pixels, 16 per wave
#define LP_HALO 10
#define LP_KC 8     // input channels per staged chunk
#define LP_SA 12    // floats per staged pixel: 4 x odd
#define LP_SB 80    // floats per staged weight row: 16 mod 32
#define LP_HEAD_PIX 64
#define LP_LAYERS GS_LPIPS_LAYERS
#define LP_TAPS GS_LPIPS_TAPS

typedef float lp_f4 __attribute__((ext_vector_type(4)));

// ---- shapes
static const int LP_C[LP_LAYERS + 1] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int LP_TAP_LAYER[LP_TAPS] = {1, 3, 6, 9, 12};
static inline int lp_level(int l) { return l < 2 ? 0 : l < 4 ? 1 : l < 7 ? 2 : l < 10 ? 3 : 4; }
static inline size_t lp_npix(int H, int W, int v) { return (size_t)(H >> v) * (size_t)(W >> v); }
struct LpOff { size_t wf[LP_LAYERS], b[LP_LAYERS], wb[LP_LAYERS], lin[LP_TAPS], total; int cin[LP_LAYERS], cout[LP_LAYERS], linc[LP_TAPS]; };
// the packed weights, in floats: [0, 3) shift, [3, 6) scale, then per layer the forward weights [9][Cin][Cout], the bias and
// the backward weights [9][Cout][Cin], then the five lin vectors (every block starts 16-byte aligned)
static inline LpOff lp_offsets() {
    LpOff o;
    size_t at = 16;
    for (int l = 0; l < LP_LAYERS; l++) {
        const size_t n = (size_t)9 * LP_C[l] * LP_C[l + 1];
        o.cin[l] = LP_C[l]; o.cout[l] = LP_C[l + 1];
        o.wf[l] = at; at += n;
        o.b[l] = at; at += LP_C[l + 1];
        o.wb[l] = at; at += n;
    }
    for (int k = 0; k < LP_TAPS; k++) { o.linc[k] = LP_C[LP_TAP_LAYER[k] + 1]; o.lin[k] = at; at += o.linc[k]; }
    o.total = at;
    return o;
}
static size_t lpips_packed_bytes() { return lp_offsets().total * sizeof(float); }
static inline size_t lp_head_blocks(int H, int W, int k) { return (lp_npix(H, W, k) + LP_HEAD_PIX - 1) / LP_HEAD_PIX; }
// floats an image that needs a gradient saves: thirteen post-activations, then five head gradients
static inline size_t lp_saved_floats(int H, int W) {
    size_t n = 0;
    for (int l = 0; l < LP_LAYERS; l++) n += (size_t)LP_C[l + 1] * lp_npix(H, W, lp_level(l));
    for (int k = 0; k < LP_TAPS; k++) n += (size_t)LP_C[LP_TAP_LAYER[k] + 1] * lp_npix(H, W, k);
    return n;
}
// which: 0 the forward's transient workspace, 1 what the forward saves, 2 the backward's transient workspace
static size_t lpips_workspace_bytes(int H, int W, int grad0, int grad1, int which) {
    const size_t full = (size_t)64 * lp_npix(H, W, 0), half = (size_t)64 * lp_npix(H, W, 1);
    const int ng = (grad0 ? 1 : 0) + (grad1 ? 1 : 0);
    size_t n = 0;
    if (which == 0) {
        n = (size_t)ng * half + (size_t)(2 - ng) * 2 * full;
        for (int k = 0; k < LP_TAPS; k++) n += lp_head_blocks(H, W, k);
    } else if (which == 1) {
        n = (size_t)ng * lp_saved_floats(H, W);
    } else {
        n = (size_t)ng * 2 * full;
    }
    return n * sizeof(float);
}

// ---- the convolution
struct LpConv {
    const float* in[2];
    const float* mask[2];  // backward: the saved post-activation of the layer (in's shape, channels-last); NULL forward
    float* out[2];
    const float* w;     // [9][K][N]
    const float* bias;  // [N], NULL backward
    const float* tf;    // shift[3], scale[3] (the head of the packed weights)
    const float* gain;  // out_tf: a device scalar multiplied into the output, NULL = 1
    int H, W, K, N, nt, tiles_x, tiles_y, relu;
    int in_tf, out_tf;  // 0 none, 1 the input transform / its factor, 2 the same with `normalize`
    long long in_sx, in_sy, in_sc, out_sx, out_sy, out_sc;  // strides in floats: next pixel, next row, next channel
};

template <int NT>
__device__ __forceinline__ void lp_mm(const float* s_in, const float* s_w, int abase, int bbase, int ksteps, lp_f4* acc) {
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const float* ap = s_in + abase + ((tap / 3) * LP_HALO + tap % 3) * LP_SA;
        const float* wp = s_w + tap * LP_KC * LP_SB + bbase;
        for (int ks = 0; ks < ksteps; ks++) {
            const float av = ap[4 * ks];
#pragma unroll
            for (int jt = 0; jt < NT; jt++)
                acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[4 * ks * LP_SB + 16 * jt], acc[jt], 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(LP_THREADS) void lp_conv_kernel(LpConv c) {
    __shared__ float4 s_in4[LP_HALO * LP_HALO * LP_SA / 4];
    __shared__ float4 s_w4[9 * LP_KC * LP_SB / 4];
    float* s_in = reinterpret_cast<float*>(s_in4);
    float* s_w = reinterpret_cast<float*>(s_w4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int tpi = c.tiles_x * c.tiles_y;
    int b = blockIdx.x;
    const int img = b / tpi;
    b -= img * tpi;
    const int ty = b / c.tiles_x, tx = b - ty * c.tiles_x;
    const int y0 = ty * LP_TS, x0 = tx * LP_TS, n0 = blockIdx.y * 16 * c.nt, ncols = 16 * c.nt;
    const float* __restrict__ in = c.in[img];
    const float* __restrict__ mask = c.mask[img];
    const bool in4 = c.in_sc == 1 && (c.K & 3) == 0 && (c.in_sx & 3) == 0 && (c.in_sy & 3) == 0;
    const bool w4 = (c.N & 3) == 0;
    // an output's sum: the 9 kc products of a chunk in one MFMA chain, the chunks' sums added in order -- the rounding error
    // of a blocked sum grows with sqrt(72) + sqrt(K / 8), not with sqrt(9 K)
    lp_f4 acc[4], part[4];
#pragma unroll
    for (int jt = 0; jt < 4; jt++) acc[jt] = lp_f4{0.0f, 0.0f, 0.0f, 0.0f};
    const int abase = ((2 * wave + (i >> 3)) * LP_HALO + (i & 7)) * LP_SA + kq, bbase = kq * LP_SB + i;
    for (int k0 = 0; k0 < c.K; k0 += LP_KC) {
        const int kc = min(LP_KC, c.K - k0), ksteps = (kc + 3) >> 2, kpad = 4 * ksteps;
        __syncthreads();
        if (in4) {  // (kc is a multiple of 4)
            for (int idx = t; idx < LP_HALO * LP_HALO * ksteps; idx += LP_THREADS) {
                const int pix = idx / ksteps, q = idx - pix * ksteps;
                const int py = pix / LP_HALO, px = pix - py * LP_HALO, gy = y0 - 1 + py, gx = x0 - 1 + px;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gy >= 0 && gy < c.H && gx >= 0 && gx < c.W) {
                    v = *reinterpret_cast<const float4*>(in + (long long)gy * c.in_sy + (long long)gx * c.in_sx + k0 + 4 * q);
                    if (mask) {
                        const float4 m = *reinterpret_cast<const float4*>(mask + ((size_t)gy * c.W + gx) * c.K + k0 + 4 * q);
                        v.x = m.x > 0.0f ? v.x : 0.0f;
                        v.y = m.y > 0.0f ? v.y : 0.0f;
                        v.z = m.z > 0.0f ? v.z : 0.0f;
                        v.w = m.w > 0.0f ? v.w : 0.0f;
                    }
                }
                *reinterpret_cast<float4*>(s_in + pix * LP_SA + 4 * q) = v;
            }
        } else {
            for (int idx = t; idx < LP_HALO * LP_HALO * kpad; idx += LP_THREADS) {
                const int pix = idx / kpad, kk = idx - pix * kpad;
                const int py = pix / LP_HALO, px = pix - py * LP_HALO, gy = y0 - 1 + py, gx = x0 - 1 + px;
                float v = 0.0f;
                if (kk < kc && gy >= 0 && gy < c.H && gx >= 0 && gx < c.W) {
                    v = in[(long long)gy * c.in_sy + (long long)gx * c.in_sx + (long long)(k0 + kk) * c.in_sc];
                    if (c.in_tf) {  // (K = 3: one chunk)
                        if (c.in_tf == 2) v = 2.0f * v - 1.0f;
                        v = (v - c.tf[kk]) / c.tf[3 + kk];
                    }
                    if (mask) v = mask[((size_t)gy * c.W + gx) * c.K + k0 + kk] > 0.0f ? v : 0.0f;
                }
                s_in[pix * LP_SA + kk] = v;
            }
        }
        if (w4) {
            const int c4 = ncols >> 2;
            for (int idx = t; idx < 9 * kpad * c4; idx += LP_THREADS) {
                const int row = idx / c4, n = 4 * (idx - row * c4);
                const int tap = row / kpad, kk = row - tap * kpad;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (kk < kc && n0 + n < c.N) v = *reinterpret_cast<const float4*>(c.w + ((size_t)tap * c.K + k0 + kk) * c.N + n0 + n);
                *reinterpret_cast<float4*>(s_w + (tap * LP_KC + kk) * LP_SB + n) = v;
            }
        } else {
            for (int idx = t; idx < 9 * kpad * ncols; idx += LP_THREADS) {
                const int row = idx / ncols, n = idx - row * ncols;
                const int tap = row / kpad, kk = row - tap * kpad;
                s_w[(tap * LP_KC + kk) * LP_SB + n] = (kk < kc && n0 + n < c.N) ? c.w[((size_t)tap * c.K + k0 + kk) * c.N + n0 + n] : 0.0f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int jt = 0; jt < 4; jt++) part[jt] = lp_f4{0.0f, 0.0f, 0.0f, 0.0f};
        switch (c.nt) {  // (uniform)
            case 1: lp_mm<1>(s_in, s_w, abase, bbase, ksteps, part); break;
            case 2: lp_mm<2>(s_in, s_w, abase, bbase, ksteps, part); break;
            default: lp_mm<4>(s_in, s_w, abase, bbase, ksteps, part); break;
        }
#pragma unroll
        for (int jt = 0; jt < 4; jt++) acc[jt] += part[jt];
    }
    float* __restrict__ out = c.out[img];
    const float gain = (c.out_tf && c.gain) ? c.gain[0] : 1.0f;
#pragma unroll
    for (int jt = 0; jt < 4; jt++) {
        const int ch = n0 + jt * 16 + i;
        if (jt >= c.nt || ch >= c.N) continue;
        const float bv = c.bias ? c.bias[ch] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int pi = 4 * kq + r, gy = y0 + 2 * wave + (pi >> 3), gx = x0 + (pi & 7);
            if (gy >= c.H || gx >= c.W) continue;
            float v = acc[jt][r] + bv;
            if (c.relu) v = v > 0.0f ? v : 0.0f;
            if (c.out_tf) {
                if (c.out_tf == 2) v = 2.0f * v;
                v = v / c.tf[3 + ch] * gain;
            }
            out[(long long)gy * c.out_sy + (long long)gx * c.out_sx + (long long)ch * c.out_sc] = v;
        }
    }
}

// ---- the pools.  in (H, W, C) -> out (H / 2, W / 2, C), four channels a thread
struct LpPool {
    const float* in[2];
    const float* g[2];    // unpool: the head's gradient into the tap, (H, W, C)
    const float* dp[2];   // unpool: the gradient of the pooled map, (H / 2, W / 2, C)
    float* out[2];
    int H, W, C;
};
__global__ __launch_bounds__(LP_THREADS) void lp_pool_kernel(LpPool p) {
    const int Ho = p.H >> 1, Wo = p.W >> 1, c4 = p.C >> 2, img = blockIdx.y;
    const size_t idx = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (idx >= (size_t)Ho * Wo * c4) return;
    const int cc = 4 * (int)(idx % c4);
    const size_t pix = idx / c4;
    const int yo = (int)(pix / Wo), xo = (int)(pix - (size_t)yo * Wo);
    const float* src = p.in[img] + ((size_t)(2 * yo) * p.W + 2 * xo) * p.C + cc;
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + p.C);
    const float4 d = *reinterpret_cast<const float4*>(src + (size_t)p.W * p.C);
    const float4 e = *reinterpret_cast<const float4*>(src + (size_t)p.W * p.C + p.C);
    float4 m;
    m.x = fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x));
    m.y = fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y));
    m.z = fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z));
    m.w = fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w));
    *reinterpret_cast<float4*>(p.out[img] + pix * p.C + cc) = m;
}
// 1 where window element `me` (0..3, row-major) is the first maximum
__device__ __forceinline__ bool lp_first_max(float v0, float v1, float v2, float v3, int me) {
    int arg = 0;
    float best = v0;
    if (v1 > best) { best = v1; arg = 1; }
    if (v2 > best) { best = v2; arg = 2; }
    if (v3 > best) { best = v3; arg = 3; }
    return arg == me;
}
// out (H, W, C) = g + (the pooled map's gradient where this element was its window's first maximum)
__global__ __launch_bounds__(LP_THREADS) void lp_unpool_kernel(LpPool p) {
    const int Ho = p.H >> 1, Wo = p.W >> 1, c4 = p.C >> 2, img = blockIdx.y;
    const size_t idx = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (idx >= (size_t)p.H * p.W * c4) return;
    const int cc = 4 * (int)(idx % c4);
    const size_t pix = idx / c4;
    const int y = (int)(pix / p.W), x = (int)(pix - (size_t)y * p.W), yo = y >> 1, xo = x >> 1;
    float4 r = *reinterpret_cast<const float4*>(p.g[img] + pix * p.C + cc);
    if (yo < Ho && xo < Wo) {
        const float* src = p.in[img] + ((size_t)(2 * yo) * p.W + 2 * xo) * p.C + cc;
        const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + p.C);
        const float4 d = *reinterpret_cast<const float4*>(src + (size_t)p.W * p.C);
        const float4 e = *reinterpret_cast<const float4*>(src + (size_t)p.W * p.C + p.C);
        const float4 u = *reinterpret_cast<const float4*>(p.dp[img] + ((size_t)yo * Wo + xo) * p.C + cc);
        const int me = 2 * (y & 1) + (x & 1);
        if (lp_first_max(a.x, b.x, d.x, e.x, me)) r.x += u.x;
        if (lp_first_max(a.y, b.y, d.y, e.y, me)) r.y += u.y;
        if (lp_first_max(a.z, b.z, d.z, e.z, me)) r.z += u.z;
        if (lp_first_max(a.w, b.w, d.w, e.w, me)) r.w += u.w;
    }
    *reinterpret_cast<float4*>(p.out[img] + pix * p.C + cc) = r;
}

// s + c += x, compensated (Kahan): the spatial means add up to 4 M non-negative terms, whose plain sequential sum would
// lose several units in the last place -- more than everything in front of it
__device__ __forceinline__ void lp_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}
// ---- the head of one tap: f0, f1 (npix, C) -> one partial per workgroup; g0, g1 (NULL = not wanted): d s_k / d f
__global__ __launch_bounds__(LP_THREADS) void lp_head_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                             const float* __restrict__ lin, int C, unsigned npix, float hw,
                                                             float* __restrict__ partial, float* __restrict__ g0,
                                                             float* __restrict__ g1) {
    __shared__ float s_part[LP_THREADS / 64], s_comp[LP_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nj = C >> 6;  // C is 64 .. 512: up to 8 channels a lane
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = j < nj ? lin[lane + 64 * j] : 0.0f;
    float total = 0.0f, comp = 0.0f;
    const unsigned p0 = blockIdx.x * LP_HEAD_PIX + wave * (LP_HEAD_PIX / 4);
    for (unsigned p = p0; p < p0 + LP_HEAD_PIX / 4 && p < npix; p++) {
        float a[8], b[8], sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            a[j] = j < nj ? f0[(size_t)p * C + lane + 64 * j] : 0.0f;
            b[j] = j < nj ? f1[(size_t)p * C + lane + 64 * j] : 0.0f;
            sa += a[j] * a[j];
            sb += b[j] * b[j];
        }
        const float ra = sqrtf(wave_sum(sa)), rb = sqrtf(wave_sum(sb)), na = ra + 1e-10f, nb = rb + 1e-10f;
        float d[8], val = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            d[j] = a[j] / na - b[j] / nb;
            val += w[j] * (d[j] * d[j]);
        }
        lp_add(total, comp, wave_sum(val));
        if (g0 || g1) {
            float u[8], da = 0.0f, db = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                u[j] = 2.0f * w[j] * d[j] / hw;
                da += u[j] * a[j];
                db += u[j] * b[j];
            }
            da = wave_sum(da);
            db = wave_sum(db);
            const float ka = ra > 0.0f ? da / (na * na * ra) : 0.0f, kb = rb > 0.0f ? db / (nb * nb * rb) : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (j < nj && g0) g0[(size_t)p * C + lane + 64 * j] = u[j] / na - a[j] * ka;
                if (j < nj && g1) g1[(size_t)p * C + lane + 64 * j] = b[j] * kb - u[j] / nb;
            }
        }
    }
    if (lane == 0) { s_part[wave] = total; s_comp[wave] = comp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f, c = 0.0f;
        for (int k = 0; k < LP_THREADS / 64; k++) {
            lp_add(s, c, s_part[k]);
            lp_add(s, c, -s_comp[k]);
        }
        partial[blockIdx.x] = s;
    }
}
struct LpSum { const float* partial[LP_TAPS]; unsigned n[LP_TAPS]; float hw[LP_TAPS]; };
__global__ __launch_bounds__(LP_THREADS) void lp_sum_kernel(LpSum s, float* __restrict__ loss, float* __restrict__ per_tap) {
    __shared__ float s_acc[LP_THREADS], s_cmp[LP_THREADS];
    float result = 0.0f, result_c = 0.0f;
    for (int k = 0; k < LP_TAPS; k++) {
        float acc = 0.0f, cmp = 0.0f;
        for (unsigned e = threadIdx.x; e < s.n[k]; e += LP_THREADS) lp_add(acc, cmp, s.partial[k][e]);
        __syncthreads();
        s_acc[threadIdx.x] = acc;
        s_cmp[threadIdx.x] = cmp;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.0f, c = 0.0f;
            for (int e = 0; e < LP_THREADS; e++) {
                lp_add(tot, c, s_acc[e]);
                lp_add(tot, c, -s_cmp[e]);
            }
            tot = tot / s.hw[k];
            if (per_tap) per_tap[k] = tot;
            lp_add(result, result_c, tot);
        }
    }
    if (threadIdx.x == 0) loss[0] = result;
}

// ---- the weights, repacked for both directions (blockIdx.y: the layer; LP_LAYERS: the lin vectors, shift and scale)
__global__ __launch_bounds__(LP_THREADS) void lp_pack_kernel(GsLpipsArgs a, float* __restrict__ packed, LpOff o) {
    const int l = blockIdx.y;
    const size_t e0 = (size_t)blockIdx.x * LP_THREADS + threadIdx.x, stride = (size_t)gridDim.x * LP_THREADS;
    if (l == LP_LAYERS) {
        const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
        for (size_t e = e0; e < 16; e += stride)
            packed[e] = e < 3 ? (a.shift ? a.shift[e] : shift[e]) : e < 6 ? (a.scale ? a.scale[e - 3] : scale[e - 3]) : 0.0f;
        for (int k = 0; k < LP_TAPS; k++)
            for (size_t e = e0; e < (size_t)o.linc[k]; e += stride) packed[o.lin[k] + e] = a.lin[k][e];
        return;
    }
    const size_t cin = o.cin[l], cout = o.cout[l];
    const float* __restrict__ W = a.weight[l];  // (Cout, Cin, 3, 3)
    for (size_t e = e0; e < 9 * cin * cout; e += stride) {
        const size_t tap = e / (cin * cout), rem = e - tap * cin * cout;
        {  // forward: [tap][ci][co]
            const size_t ci = rem / cout, co = rem - ci * cout;
            packed[o.wf[l] + e] = W[(co * cin + ci) * 9 + tap];
        }
        {  // backward: [tap][co][ci], the window flipped
            const size_t co = rem / cin, ci = rem - co * cin;
            packed[o.wb[l] + e] = W[(co * cin + ci) * 9 + (8 - tap)];
        }
    }
    for (size_t e = e0; e < cout; e += stride) packed[o.b[l] + e] = a.bias[l][e];
}

// ---- launchers (the C ABI has checked every argument)
static int launch_lpips_pack(const GsLpipsArgs* a, float* packed, hipStream_t s) {
    StageScope st("lpips_pack", s);
    hipLaunchKernelGGL(lp_pack_kernel, dim3(256, LP_LAYERS + 1), dim3(LP_THREADS), 0, s, *a, packed, lp_offsets());
    GS_LAUNCH_CHECK("lpips_pack", 0, s);
    return GS_OK;
}
// workgroups of a convolution launch on n images of H x W with N output channels: {nt, grid.x, grid.y}
static inline void lp_conv_grid(int H, int W, int N, int nimg, int* nt, int* gx, int* gy) {
    const int tiles = ((W + LP_TS - 1) / LP_TS) * ((H + LP_TS - 1) / LP_TS) * nimg, n16 = (N + 15) / 16;
    int pick = 1;
    for (int cand = 4; cand > 1; cand >>= 1)
        if (cand <= n16 && (long long)tiles * ((n16 + cand - 1) / cand) >= 256) { pick = cand; break; }
    *nt = pick;
    *gx = tiles;
    *gy = (n16 + pick - 1) / pick;
}
static int lpips_conv_workgroups(int H, int W, int N, int nimg) {
    int nt, gx, gy;
    lp_conv_grid(H, W, N, nimg, &nt, &gx, &gy);
    return gx * gy;
}
static int lp_launch_conv(LpConv c, int nimg, hipStream_t s) {
    int gx, gy;
    lp_conv_grid(c.H, c.W, c.N, nimg, &c.nt, &gx, &gy);
    c.tiles_x = (c.W + LP_TS - 1) / LP_TS;
    c.tiles_y = (c.H + LP_TS - 1) / LP_TS;
    hipLaunchKernelGGL(lp_conv_kernel, dim3(gx, gy), dim3(LP_THREADS), 0, s, c);
    GS_LAUNCH_CHECK("lpips_conv", 0, s);
    return GS_OK;
}
// layer l of the packed weights, forward (backward = 0) or backward-data, as a launch description without its maps
static LpConv lp_layer(const float* packed, int l, int backward, int H, int W) {
    const LpOff o = lp_offsets();
    LpConv c = {};
    c.H = H;
    c.W = W;
    c.tf = packed;
    if (!backward) {
        c.K = LP_C[l]; c.N = LP_C[l + 1];
        c.w = packed + o.wf[l];
        c.bias = packed + o.b[l];
        c.relu = 1;
    } else {
        c.K = LP_C[l + 1]; c.N = LP_C[l];
        c.w = packed + o.wb[l];
    }
    c.in_sc = 1; c.in_sx = c.K; c.in_sy = (long long)W * c.K;
    c.out_sc = 1; c.out_sx = c.N; c.out_sy = (long long)W * c.N;
    return c;
}
static int launch_lpips_conv(const float* packed, int layer, int backward, int normalize, int H, int W, const float* in, long long in_cs,
                             long long in_rs, const float* mask, float* out, hipStream_t s) {
    StageScope st("lpips_conv", s);
    LpConv c = lp_layer(packed, layer, backward, H, W);
    c.in[0] = in; c.mask[0] = backward ? mask : nullptr; c.out[0] = out;
    if (layer == 0 && !backward) {
        c.in_tf = normalize ? 2 : 1;
        c.in_sc = in_cs; c.in_sy = in_rs; c.in_sx = 1;
    }
    if (layer == 0 && backward) {  // the image gradient, (3, H, W) contiguous
        c.out_tf = normalize ? 2 : 1;
        c.out_sc = (long long)H * W; c.out_sy = W; c.out_sx = 1;
    }
    return lp_launch_conv(c, 1, s);
}

static int launch_lpips_forward(const GsLpipsArgs* a, float* loss, float* per_tap, float* saved, float* ws, hipStream_t s) {
    StageScope st("lpips", s);
    const int H = a->H, W = a->W;
    const LpOff o = lp_offsets();
    const bool grad[2] = {a->need_grad0 != 0, a->need_grad1 != 0};
    const size_t full = (size_t)64 * lp_npix(H, W, 0), half = (size_t)64 * lp_npix(H, W, 1), per_saved = lp_saved_floats(H, W);
    // carve: per image either its saved block and one transient map (the pools' outputs), or two transient maps
    float *act[2][LP_LAYERS] = {}, *hg[2][LP_TAPS] = {}, *tmp[2][2] = {};
    for (int j = 0; j < 2; j++) {
        if (grad[j]) {
            float* p = saved;
            saved += per_saved;
            for (int l = 0; l < LP_LAYERS; l++) { act[j][l] = p; p += (size_t)LP_C[l + 1] * lp_npix(H, W, lp_level(l)); }
            for (int k = 0; k < LP_TAPS; k++) { hg[j][k] = p; p += (size_t)LP_C[LP_TAP_LAYER[k] + 1] * lp_npix(H, W, k); }
            tmp[j][0] = tmp[j][1] = ws;
            ws += half;
        } else {
            tmp[j][0] = ws;
            tmp[j][1] = ws + full;
            ws += 2 * full;
        }
    }
    float* partial[LP_TAPS];
    for (int k = 0; k < LP_TAPS; k++) { partial[k] = ws; ws += lp_head_blocks(H, W, k); }
    const float* cur[2] = {a->in0, a->in1};
    int flip[2] = {0, 0};  // which transient map an image without a gradient writes next
    for (int l = 0, k = 0; l < LP_LAYERS; l++) {
        const int v = lp_level(l), Hv = H >> v, Wv = W >> v;
        if (l > 0 && lp_level(l - 1) != v) {  // the pool in front of this layer
            LpPool p = {};
            p.H = H >> (v - 1); p.W = W >> (v - 1); p.C = LP_C[l];
            for (int j = 0; j < 2; j++) {
                p.in[j] = cur[j];
                p.out[j] = tmp[j][flip[j]];
                cur[j] = p.out[j];
                flip[j] ^= 1;
            }
            const size_t n = (size_t)Hv * Wv * (p.C >> 2);
            hipLaunchKernelGGL(lp_pool_kernel, dim3((unsigned)((n + LP_THREADS - 1) / LP_THREADS), 2), dim3(LP_THREADS), 0, s, p);
            GS_LAUNCH_CHECK("lpips_pool", 0, s);
        }
        LpConv c = lp_layer(a->packed, l, 0, Hv, Wv);
        for (int j = 0; j < 2; j++) {
            c.in[j] = cur[j];
            if (grad[j]) {
                c.out[j] = act[j][l];
            } else {
                c.out[j] = tmp[j][flip[j]];
                flip[j] ^= 1;
            }
            cur[j] = c.out[j];
        }
        if (l == 0) {
            // (both images through one launch: one set of strides, so the second image is addressed from the first's base
            // only when the strides agree -- otherwise two launches)
            c.in_tf = a->normalize ? 2 : 1;
            c.in_sx = 1;
            if (a->cs0 == a->cs1 && a->rs0 == a->rs1) {
                c.in_sc = a->cs0; c.in_sy = a->rs0;
                if (const int rc = lp_launch_conv(c, 2, s)) return rc;
            } else {
                LpConv c1 = c;
                c.in_sc = a->cs0; c.in_sy = a->rs0;
                if (const int rc = lp_launch_conv(c, 1, s)) return rc;
                c1.in[0] = c1.in[1]; c1.out[0] = c1.out[1];
                c1.in_sc = a->cs1; c1.in_sy = a->rs1;
                if (const int rc = lp_launch_conv(c1, 1, s)) return rc;
            }
        } else if (const int rc = lp_launch_conv(c, 2, s)) {
            return rc;
        }
        if (l == LP_TAP_LAYER[k]) {
            const size_t npix = lp_npix(H, W, k);
            hipLaunchKernelGGL(lp_head_kernel, dim3((unsigned)lp_head_blocks(H, W, k)), dim3(LP_THREADS), 0, s, cur[0], cur[1],
                               a->packed + o.lin[k], LP_C[l + 1], (unsigned)npix, (float)npix, partial[k], hg[0][k], hg[1][k]);
            GS_LAUNCH_CHECK("lpips_head", 0, s);
            k++;
        }
    }
    LpSum sum;
    for (int k = 0; k < LP_TAPS; k++) {
        sum.partial[k] = partial[k];
        sum.n[k] = (unsigned)lp_head_blocks(H, W, k);
        sum.hw[k] = (float)lp_npix(H, W, k);
    }
    hipLaunchKernelGGL(lp_sum_kernel, dim3(1), dim3(LP_THREADS), 0, s, sum, loss, per_tap);
    GS_LAUNCH_CHECK("lpips_sum", 0, s);
    return GS_OK;
}

static int launch_lpips_backward(const GsLpipsArgs* a, const float* dL_dloss, float* d_in0, float* d_in1, const float* saved, float* ws,
                                 hipStream_t s) {
    StageScope st("lpips_bwd", s);
    const int H = a->H, W = a->W;
    const size_t full = (size_t)64 * lp_npix(H, W, 0), per_saved = lp_saved_floats(H, W);
    // the images that saved something, in the forward's order, and which of them the caller wants a gradient for
    const float *act[2][LP_LAYERS] = {}, *hg[2][LP_TAPS] = {};
    float *d[2][2] = {}, *d_img[2] = {};
    int n = 0;
    for (int j = 0; j < 2; j++) {
        if (!(j == 0 ? a->need_grad0 : a->need_grad1)) continue;
        const float* p = saved;
        saved += per_saved;
        float* out = j == 0 ? d_in0 : d_in1;
        if (!out) continue;
        for (int l = 0; l < LP_LAYERS; l++) { act[n][l] = p; p += (size_t)LP_C[l + 1] * lp_npix(H, W, lp_level(l)); }
        for (int k = 0; k < LP_TAPS; k++) { hg[n][k] = p; p += (size_t)LP_C[LP_TAP_LAYER[k] + 1] * lp_npix(H, W, k); }
        d[n][0] = ws;
        d[n][1] = ws + full;
        ws += 2 * full;
        d_img[n] = out;
        n++;
    }
    if (n == 0) return GS_OK;
    const float* cur[2] = {hg[0][LP_TAPS - 1], hg[1][LP_TAPS - 1]};
    for (int l = LP_LAYERS - 1; l >= 0; l--) {
        const int v = lp_level(l), Hv = H >> v, Wv = W >> v;
        LpConv c = lp_layer(a->packed, l, 1, Hv, Wv);
        float* dst[2] = {};
        for (int j = 0; j < n; j++) {
            c.in[j] = cur[j];
            c.mask[j] = act[j][l];
            dst[j] = l == 0 ? d_img[j] : (cur[j] == d[j][0] ? d[j][1] : d[j][0]);
            c.out[j] = dst[j];
        }
        if (l == 0) {
            c.out_tf = a->normalize ? 2 : 1;
            c.gain = dL_dloss;
            c.out_sc = (long long)H * W; c.out_sy = W; c.out_sx = 1;
        }
        if (const int rc = lp_launch_conv(c, n, s)) return rc;
        for (int j = 0; j < n; j++) cur[j] = dst[j];
        if (l > 0 && lp_level(l - 1) != v) {  // back through the pool, into the tap in front of it
            LpPool p = {};
            p.H = H >> (v - 1); p.W = W >> (v - 1); p.C = LP_C[l];
            for (int j = 0; j < n; j++) {
                p.in[j] = act[j][l - 1];
                p.g[j] = hg[j][v - 1];
                p.dp[j] = cur[j];
                p.out[j] = cur[j] == d[j][0] ? d[j][1] : d[j][0];
                cur[j] = p.out[j];
            }
            const size_t e = (size_t)p.H * p.W * (p.C >> 2);
            hipLaunchKernelGGL(lp_unpool_kernel, dim3((unsigned)((e + LP_THREADS - 1) / LP_THREADS), n), dim3(LP_THREADS), 0, s, p);
            GS_LAUNCH_CHECK("lpips_unpool", 0, s);
        }
    }
    return GS_OK;
}
// the pools on caller-given maps (tests): backward = 0: out (H / 2, W / 2, C) = pool(in); 1: out (H, W, C) = g + unpool(dp)
static int launch_lpips_pool(int backward, int H, int W, int C, const float* in, const float* g, const float* dp, float* out, hipStream_t s) {
    LpPool p = {};
    p.H = H; p.W = W; p.C = C;
    p.in[0] = in; p.g[0] = g; p.dp[0] = dp; p.out[0] = out;
    const size_t e = (backward ? (size_t)H * W : (size_t)(H >> 1) * (W >> 1)) * (C >> 2);
    if (e == 0) return GS_OK;
    if (backward)
        hipLaunchKernelGGL(lp_unpool_kernel, dim3((unsigned)((e + LP_THREADS - 1) / LP_THREADS), 1), dim3(LP_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(lp_pool_kernel, dim3((unsigned)((e + LP_THREADS - 1) / LP_THREADS), 1), dim3(LP_THREADS), 0, s, p);
    GS_LAUNCH_CHECK("lpips_pool", 0, s);
    return GS_OK;
}

extern "C" {

static int lpips_validate(const GsLpipsArgs* a) {
    if (!a || a->H < GS_LPIPS_MIN_SIZE || a->H > GS_LPIPS_MAX_SIZE || a->W < GS_LPIPS_MIN_SIZE || a->W > GS_LPIPS_MAX_SIZE)
        return GS_E_BAD_ARG;
    if (!required(a->in0, 4) || !required(a->in1, 4) || !required(a->packed, 16)) return GS_E_BAD_ARG;
    if (a->cs0 < 1 || a->cs1 < 1 || a->rs0 < a->W || a->rs1 < a->W) return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_lpips_packed_bytes(size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    *out = lpips_packed_bytes();
    return GS_OK;
}
int gs_lpips_pack_weights(const GsLpipsArgs* a, void* packed, size_t packed_bytes, void* stream) {
    if (!a || !required(packed, 16) || !aligned(a->shift, 4) || !aligned(a->scale, 4)) return GS_E_BAD_ARG;
    for (int l = 0; l < GS_LPIPS_LAYERS; l++)
        if (!required(a->weight[l], 4) || !required(a->bias[l], 4)) return GS_E_BAD_ARG;
    for (int k = 0; k < GS_LPIPS_TAPS; k++)
        if (!required(a->lin[k], 4)) return GS_E_BAD_ARG;
    if (packed_bytes < lpips_packed_bytes()) return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_pack(a, (float*)packed, (hipStream_t)stream);
}
int gs_lpips_workspace_bytes(int32_t H, int32_t W, int32_t need_grad0, int32_t need_grad1, int32_t which, size_t* out) {
    if (!out || H < GS_LPIPS_MIN_SIZE || H > GS_LPIPS_MAX_SIZE || W < GS_LPIPS_MIN_SIZE || W > GS_LPIPS_MAX_SIZE || which < 0 ||
        which > GS_LPIPS_WS_BACKWARD)
        return GS_E_BAD_ARG;
    *out = lpips_workspace_bytes(H, W, need_grad0, need_grad1, which);
    return GS_OK;
}
int gs_lpips_forward(const GsLpipsArgs* a, float* loss, float* per_tap, void* saved, size_t saved_bytes, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (const int rc = lpips_validate(a)) return rc;
    if (!required(loss, 4) || !aligned(per_tap, 4) || !required(workspace, 16)) return GS_E_BAD_ARG;
    const size_t need_saved = lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_SAVED);
    if (need_saved && !required(saved, 16)) return GS_E_BAD_ARG;
    if (saved_bytes < need_saved ||
        workspace_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_FORWARD))
        return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_forward(a, loss, per_tap, (float*)saved, (float*)workspace, (hipStream_t)stream);
}
int gs_lpips_backward(const GsLpipsArgs* a, const float* dL_dloss, float* d_in0, float* d_in1, const void* saved,
                      size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = lpips_validate(a)) return rc;
    if (!aligned(dL_dloss, 4) || !aligned(d_in0, 4) || !aligned(d_in1, 4)) return GS_E_BAD_ARG;
    if ((d_in0 && !a->need_grad0) || (d_in1 && !a->need_grad1)) return GS_E_BAD_ARG;
    if (!d_in0 && !d_in1) return GS_OK;
    if (!required(saved, 16) || !required(workspace, 16)) return GS_E_BAD_ARG;
    if (saved_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_SAVED) ||
        workspace_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_BACKWARD))
        return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_backward(a, dL_dloss, d_in0, d_in1, (const float*)saved, (float*)workspace, (hipStream_t)stream);
}
int gs_lpips_conv(const float* packed, int32_t layer, int32_t backward, int32_t normalize, int32_t H, int32_t W, const float* in,
                  int64_t in_cs, int64_t in_rs, const float* mask, float* out, void* stream) {
    if (!required(packed, 16) || layer < 0 || layer >= GS_LPIPS_LAYERS || H < 1 || W < 1 || H > GS_LPIPS_MAX_SIZE ||
        W > GS_LPIPS_MAX_SIZE)
        return GS_E_BAD_ARG;
    const bool image_in = layer == 0 && !backward, image_out = layer == 0 && backward;
    if (image_in ? (!required(in, 4) || in_cs < 1 || in_rs < W) : !required(in, 16)) return GS_E_BAD_ARG;
    if (image_out ? !required(out, 4) : !required(out, 16)) return GS_E_BAD_ARG;
    if (backward && !required(mask, 16)) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_conv(packed, layer, backward, normalize, H, W, in, in_cs, in_rs, mask, out, (hipStream_t)stream);
}
int gs_lpips_pool(int32_t backward, int32_t H, int32_t W, int32_t C, const float* in, const float* g, const float* dp, float* out,
                  void* stream) {
    if (H < 1 || W < 1 || H > GS_LPIPS_MAX_SIZE || W > GS_LPIPS_MAX_SIZE || C < 4 || C > 512 || (C & 3) || !required(in, 16) ||
        !required(out, 16))
        return GS_E_BAD_ARG;
    if (backward && (!required(g, 16) || ((H >> 1) && (W >> 1) && !required(dp, 16)))) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_pool(backward, H, W, C, in, g, dp, out, (hipStream_t)stream);
}

}  // extern "C"
