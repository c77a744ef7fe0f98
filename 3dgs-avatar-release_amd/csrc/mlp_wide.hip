// mlp_wide.hip -- the coordinate networks mlp.hip turns down (models/network_utils.py VanillaCondMLP with a frequency
// encoding, skip connections or width 256; HannwCondMLP) as one fused op on the exact-fp32 MFMA, by mlp.hip's rules: one
// forward launch that keeps a row tile on chip from the input to the output, a backward that is a tile walk back, a split-K
// parameter-gradient launch and a final sum in index order.  New code beside the narrow kernels, which it does not touch.
//
// Spec (fp32 throughout; every array row-major and contiguous).  x (N, d); one optional condition row cond (C,) that joins
// the first layer only; nl = n_hidden + 1 nn.Linear layers of hidden width W.
//   Encoding e = enc(x), E columns.  multires == 0: e = x, E = d.  multires = m > 0: the block x (with include_input), then
//     for k = 0 .. m - 1 the blocks w_k sin(2^k x), w_k cos(2^k x), d columns each: E = d (include_input + 2 m).  The band
//     weights w_k are host floats by value (all 1 for VanillaCondMLP, the Hann window for HannwCondMLP); 2^k x is exact; sin
//     and cos are sinf / cosf (the fast intrinsics' error grows with the argument, and arguments reach 2^(m-1)).
//   Layers.  h_0 = e.  Layer l reads v_l: v_0 = [h_0 | cond]; v_l = [h_l | e] / sqrt(2) for l in the skip set (bit l of
//     skip_mask, 1 <= l <= n_hidden); v_l = h_l otherwise.  z_l = v_l W_l^T + b_l; h_{l+1} = leaky(z_l) for l < nl - 1;
//     y = z_{nl-1}.  A layer that feeds a skip layer has W - E outputs (as the reference constructs it), so E < W wherever
//     a skip exists:  W_0 (out_0, E + C);  W_l (out_l, W);  out_l = dout for the last layer, W - E before a skip, else W.
//     leaky(z) = z > 0 ? z : slope z, slope >= 0 (0: ReLU); a unit with a == 0 takes the slope in the backward.
//   Backward from g = dL/dy: dz_{nl-1} = g;  dv_l = dz_l W_l (/ sqrt(2) at a skip layer);  dz_{l-1} = dv_l[:, :out_{l-1}] *
//     (v_l > 0 ? 1 : slope);  at a skip layer dv_l[:, W - E:] is added to de, the encoding's gradient, in the row's own
//     tile (no cross-row sum);  dW_l = dz_l^T v_l, db_l = the column sums of dz_l;  de += dz_0 W_0[:, :E];
//     dW_0[:, E:] = db_0 (x) cond;  dcond = W_0[:, E:]^T db_0 (no (N, E + C) matrix exists in either direction);
//     dx = (x block of de) + sum_k 2^k w_k (cos(2^k x) de_sin,k - sin(2^k x) de_cos,k), the encoding recomputed from x.
//     A gradient nobody asked for (NULL) is neither computed nor written; the walk stops at the lowest layer somebody asked
//     for, and de exists only when dx is wanted.
//   Supported: W a multiple of 32 in 32..GS_WMLP_MAX_WIDTH, 1..GS_WMLP_MAX_HIDDEN hidden layers, multires 0..GS_WMLP_MAX_FREQS,
//     E in 1..GS_WMLP_MAX_ENC, C in 0..GS_WMLP_MAX_COND, dout in 1..GS_WMLP_MAX_OUT.
// What the forward saves: for every hidden layer the W-column input of the NEXT layer, v_1 .. v_{n_hidden}, (n_hidden, N, W).
//   Before a skip layer that is [h / sqrt(2) | e / sqrt(2)]: the W - E = 217 activation columns of the reference's networks
//   are no multiple of 4, and saving the layer's whole input instead keeps every saved row W floats long and 16-byte
//   aligned, gives the backward's mask (v and h have the same sign) and is dW's right-hand side as it stands.
// What is different from mlp.hip at width 256 (WM_THREADS = 512 threads, 8 waves, a wave owns 16 rows of WM_T = 128):
//   LDS      a 128 x 256 tile (row stride WM_AS = 260 = 4 x 65: 133 120 B) leaves 30 KB of the 160 KiB, so the weights are
//            staged in K-chunks of WM_KC = 28 columns (forward: 256 rows of stride 28 = 4 x 7, 28 672 B; backward: 28 rows
//            of stride 272 = 16 mod 32, 30 464 B), a barrier pair per chunk because all waves share them.  The wave's
//            accumulators, 16 rows x 256 columns = 16 column tiles x 4 = 64 VGPRs, stay in registers across the chunks.
//            Static LDS: forward 161 856 B, backward 163 648 B, of the 163 840 B a workgroup may declare; the compiler's
//            report: 256 VGPRs and 136 / 232 B of scratch per lane (forward / backward), 2 waves per SIMD.
//   in place a wave reads its own 16 rows only and overwrites them after its last K-chunk of the layer.
//   skip     the encoding has no tile of its own: before a skip layer the wave writes e / sqrt(2), recomputed from x, into
//            the W - out columns its W - E activations leave free, and the layer is a plain K = W product.  In the
//            backward de lives in global memory ((N, E): the workspace, or dx itself at multires 0); every element is
//            written and re-read by its row's own wave, the highest skip first and the first layer last.
//   layer 0  the encoding is computed into the tile in passes of WM_EC = 256 columns (E up to 512: two passes), each
//            streamed through the K-chunks, the accumulators staying in registers.
//   dW       split-K as mlp.hip's, an item being a 128 x 128 block of one layer's dW; layer 0 recomputes its encoding
//            columns.  R = max(GS_WMLP_PARTIAL_MIN_ROWS, ceil(N / GS_WMLP_MAX_PARTIALS) rounded up to 32) rows per
//            partial: a function of N alone.
// No atomics, no memsets, no host synchronisation, no host memory traffic: every output is bitwise reproducible and the
// calls are capture-safe.
#include "common.h"
#include "boundary.h"
#include "../../include/gsplat_mi355_wmlp.h"

#define WM_THREADS 512
#define WM_WAVES 8
#define WM_T GS_WMLP_TILE_ROWS
#define WM_AS 260                          // row stride of the tile: 4 x 65
#define WM_KC 28                           // K columns (forward) / rows (backward) of the weights per chunk
#define WM_WS_F 28                         // forward weight stride: 4 x 7
#define WM_WS_B 272                        // backward weight stride: 16 mod 32
#define WM_EC 256                          // encoding columns per pass of the first layer
#define WM_DC 128                          // rows and columns of one dW item
#define WM_DS 144                          // widest stride of the dW kernel's two tiles
#define WM_RK 32                           // rows staged per step of the dW kernel
#define WM_FINAL_THREADS 256
#define WM_SQRT2 1.41421356237309515f
static_assert(WM_T == 16 * WM_WAVES, "a wave owns 16 rows of the tile");
static_assert(GS_WMLP_MAX_WIDTH == 256 && WM_AS >= GS_WMLP_MAX_WIDTH && WM_EC <= GS_WMLP_MAX_WIDTH, "16 column tiles a wave");
static_assert(GS_WMLP_MAX_OUT <= 64 && GS_WMLP_MAX_LAYERS == GS_WMLP_MAX_HIDDEN + 1, "the output layer is at most four tiles");
static_assert(GS_WMLP_PARTIAL_MIN_ROWS % WM_RK == 0 && WM_RK % 4 == 0 && WM_KC % 4 == 0, "row chunks start 16-byte aligned");
static_assert(WM_T * WM_AS * 4 + GS_WMLP_MAX_WIDTH * WM_WS_F * 4 + 64 <= 163840, "forward LDS");
static_assert(WM_T * WM_AS * 4 + WM_KC * WM_WS_B * 4 + 64 <= 163840, "backward LDS");
static_assert(WM_FINAL_THREADS >= GS_WMLP_MAX_WIDTH, "the final kernel sums db_0 one thread a unit");

typedef float wm_f4 __attribute__((ext_vector_type(4)));

// ---- shapes (host and device)
__host__ __device__ static inline int wm_enc_dim(const GsWideMlpArgs& a) {
    return a.multires > 0 ? a.dim_x * ((a.include_input ? 1 : 0) + 2 * a.multires) : a.dim_x;
}
__host__ __device__ static inline bool wm_skip(const GsWideMlpArgs& a, int l) { return (a.skip_mask >> l) & 1u; }
__host__ __device__ static inline int wm_in(const GsWideMlpArgs& a, int l) { return l == 0 ? wm_enc_dim(a) : a.width; }
__host__ __device__ static inline int wm_ld(const GsWideMlpArgs& a, int l) { return l == 0 ? wm_enc_dim(a) + a.dim_cond : a.width; }
__host__ __device__ static inline int wm_out(const GsWideMlpArgs& a, int l) {
    if (l == a.n_hidden) return a.dim_out;
    return wm_skip(a, l + 1) ? a.width - wm_enc_dim(a) : a.width;
}
__host__ __device__ static inline int wm_pad(int v, int m) { return (v + m - 1) / m * m; }
__host__ __device__ static inline int wm_stride_b(int w) { return (w + 15) / 32 * 32 + 16; }
__host__ __device__ static inline int wm_blocks(int v) { return (v + WM_DC - 1) / WM_DC; }
// floats of one partial: per layer dW_l without the condition's columns, then db_l; the offset of layer l in it
__host__ __device__ static inline int wm_part_off(const GsWideMlpArgs& a, int l) {
    int off = 0;
    for (int k = 0; k < l; k++) off += wm_out(a, k) * (wm_in(a, k) + 1);
    return off;
}
static inline int wm_rows_per_partial(int N) {
    const int r = wm_pad((N + GS_WMLP_MAX_PARTIALS - 1) / GS_WMLP_MAX_PARTIALS, WM_RK);
    return r > GS_WMLP_PARTIAL_MIN_ROWS ? r : GS_WMLP_PARTIAL_MIN_ROWS;
}
static inline int wm_partials(int N) {
    const int R = wm_rows_per_partial(N);
    return (N + R - 1) / R;
}
static inline int wm_items(const GsWideMlpArgs& a) {
    int n = 0;
    for (int l = 0; l <= a.n_hidden; l++) n += wm_blocks(wm_in(a, l)) * wm_blocks(wm_out(a, l));
    return n;
}
static inline bool wm_wanted(const GsWideMlpArgs& a, int l) { return a.dW[l] || a.db[l] || (l == 0 && a.dim_cond > 0 && a.dcond); }
// the lowest layer whose dz somebody needs (n_hidden + 1: nobody)
static inline int wm_lowest(const GsWideMlpArgs& a) {
    if (a.dx) return 0;
    for (int l = 0; l <= a.n_hidden; l++)
        if (wm_wanted(a, l)) return l;
    return a.n_hidden + 1;
}
static size_t wmlp_saved_bytes(const GsWideMlpArgs* a) { return (size_t)a->n_hidden * a->N * a->width * sizeof(float); }
static size_t wmlp_workspace_bytes(const GsWideMlpArgs* a, int backward) {
    if (a->N == 0) return 0;
    if (!backward) return a->dim_cond > 0 ? (size_t)a->width * sizeof(float) : 0;
    // dz_0 .. dz_{n_hidden-1}, de (with an encoding), then the partials
    const size_t de = a->multires > 0 ? (size_t)a->N * wm_enc_dim(*a) : 0;
    return ((size_t)a->n_hidden * a->N * a->width + de + (size_t)wm_partials(a->N) * wm_part_off(*a, a->n_hidden + 1)) * sizeof(float);
}

// ---- the encoding: column c of enc(x) for the row at xr; bw = the band weights (LDS)
__device__ __forceinline__ float wm_enc(const GsWideMlpArgs& a, const float* bw, const float* __restrict__ xr, int c) {
    if (a.multires == 0) return xr[c];
    const int d = a.dim_x;
    int b = c / d;
    const int j = c - b * d;
    if (a.include_input) {
        if (b == 0) return xr[j];
        b--;
    }
    const int k = b >> 1;
    const float arg = xr[j] * (float)(1 << k);
    return bw[k] * ((b & 1) ? cosf(arg) : sinf(arg));
}
__device__ __forceinline__ void wm_band_weights(const GsWideMlpArgs& a, float* bw) {
#pragma unroll
    for (int k = 0; k < GS_WMLP_MAX_FREQS; k++)
        if (threadIdx.x == k) bw[k] = a.band_w[k];
}

// ---- staging (as mlp.hip's)
// Columns [c0, c0 + cw) of n rows of a contiguous (., ld) slab at src (16-byte aligned) -> dst[r * S + c], read in aligned
// 16-byte units; columns cw .. cpad - 1 and rows n .. rows - 1 are zeroed.
__device__ __forceinline__ void wm_load_rows(float* dst, int S, const float* __restrict__ src, int n, int rows, int ld, int c0,
                                             int cw, int cpad) {
    const int t = threadIdx.x, U = (cw + 3) / 4 + 1, total = n * ld;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int idx = t; idx < n * U; idx += WM_THREADS) {
        const int r = idx / U, u = idx - r * U;
        const int s = r * ld + c0, e = s + cw, q = (s >> 2) + u;
        if (4 * q >= e) continue;
        float v[4];
        if (4 * q + 3 < total) {
            const float4 v4 = s4[q];
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = 4 * q + j < total ? src[4 * q + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int f = 4 * q + j;
            if (f >= s && f < e) dst[r * S + (f - s)] = v[j];
        }
    }
    for (int idx = t; idx < rows * cpad; idx += WM_THREADS) {
        const int r = idx / cpad, c = idx - r * cpad;
        if (r >= n || c >= cw) dst[r * S + c] = 0.0f;
    }
}
// rows x cols of a weight matrix at src (row stride ld) -> dst[r * S + c]; rows .. rpad - 1 and columns cols .. cpad - 1 are
// zeroed.  16-byte loads where the layout allows them (the hidden layers always do).
__device__ __forceinline__ void wm_load_weights(float* dst, int S, const float* __restrict__ src, int ld, int rows, int rpad,
                                                int cols, int cpad) {
    const int t = threadIdx.x;
    if (((ld | cols | cpad) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int c4 = cpad >> 2;
        for (int idx = t; idx < rpad * c4; idx += WM_THREADS) {
            const int r = idx / c4, c = 4 * (idx - r * c4);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < rows && c < cols) v = *reinterpret_cast<const float4*>(src + (size_t)r * ld + c);
            *reinterpret_cast<float4*>(dst + r * S + c) = v;
        }
    } else {
        for (int idx = t; idx < rpad * cpad; idx += WM_THREADS) {
            const int r = idx / cpad, c = idx - r * cpad;
            dst[r * S + c] = (r < rows && c < cols) ? src[(size_t)r * ld + c] : 0.0f;
        }
    }
}

// ---- products: the wave's 16 rows at `arow` (row stride WM_AS, already offset to the chunk's first column) times 4 NQ
// column tiles of 16, over `ksteps` steps of 4.  BWD = false: w[j * ws + k] (out = a W^T);  BWD = true: w[k * ws + j]
// (out = a W).  Tiles past the layer's own are computed from whatever the weight buffer holds there and never read.
template <int NQ, bool BWD>
__device__ __forceinline__ void wm_mm_n(const float* arow, const float* w, int ws, int ksteps, wm_f4* acc) {
    const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
    const float* ap = arow + i * WM_AS + kq;
    const float* wp = BWD ? w + kq * ws + i : w + i * ws + kq;
    const int wk = BWD ? 4 * ws : 4, wj = BWD ? 16 : 16 * ws;
    for (int ks = 0; ks < ksteps; ks++) {
        const float av = ap[4 * ks];
#pragma unroll
        for (int jt = 0; jt < 4 * NQ; jt++) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[ks * wk + jt * wj], acc[jt], 0, 0, 0);
    }
}
template <bool BWD>
__device__ __forceinline__ void wm_mm(int nt, const float* arow, const float* w, int ws, int ksteps, wm_f4* acc) {
    switch ((nt + 3) >> 2) {  // (wave-uniform)
        case 1: wm_mm_n<1, BWD>(arow, w, ws, ksteps, acc); break;
        case 2: wm_mm_n<2, BWD>(arow, w, ws, ksteps, acc); break;
        case 3: wm_mm_n<3, BWD>(arow, w, ws, ksteps, acc); break;
        default: wm_mm_n<4, BWD>(arow, w, ws, ksteps, acc); break;
    }
}
__device__ __forceinline__ void wm_zero(wm_f4* acc) {
#pragma unroll
    for (int jt = 0; jt < 16; jt++) acc[jt] = wm_f4{0.0f, 0.0f, 0.0f, 0.0f};
}
// the wave's 16 rows of the tile (W floats each, n_valid of them real) -> one contiguous block at dst, 16 bytes a lane
__device__ __forceinline__ void wm_store_rows(const float* arow, float* __restrict__ dst, int W, int n_valid) {
    const int lane = threadIdx.x & 63, w4 = W >> 2;
    for (int f = lane; f < 16 * w4; f += 64) {
        const int r = f / w4, c = 4 * (f - r * w4);
        if (r < n_valid) *reinterpret_cast<float4*>(dst + (size_t)r * W + c) = *reinterpret_cast<const float4*>(arow + r * WM_AS + c);
    }
}

// b0'[o] = b_0[o] + sum_c W_0[o][E + c] cond[c], o = blockIdx.x
__global__ __launch_bounds__(64) void wm_cond_kernel(GsWideMlpArgs a, float* __restrict__ b0) {
    const int o = blockIdx.x, lane = threadIdx.x, E = wm_enc_dim(a);
    const float* w = a.W[0] + (size_t)o * (E + a.dim_cond) + E;
    float acc = 0.0f;
    for (int c = lane; c < a.dim_cond; c += 64) acc += w[c] * a.cond[c];
    acc = wave_sum(acc);
    if (lane == 0) b0[o] = a.b[0][o] + acc;
}

__global__ __launch_bounds__(WM_THREADS) void wm_fwd_kernel(GsWideMlpArgs a, const float* __restrict__ b0, float* __restrict__ y,
                                                            float* __restrict__ acts) {
    __shared__ float4 s_act4[WM_T * WM_AS / 4];
    __shared__ float4 s_w4[GS_WMLP_MAX_WIDTH * WM_WS_F / 4];
    __shared__ float s_bw[16];
    float* s_act = reinterpret_cast<float*>(s_act4);
    float* s_w = reinterpret_cast<float*>(s_w4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, nl = a.n_hidden + 1, d = a.dim_x, dout = a.dim_out, E = wm_enc_dim(a);
    const size_t row0 = (size_t)blockIdx.x * WM_T;
    const int n = (int)min((size_t)WM_T, (size_t)a.N - row0);
    float* arow = s_act + wave * 16 * WM_AS;
    const int n_wave = n - wave * 16;  // (may be <= 0)
    const int col = lane & 15, rq = (lane >> 4) * 4;
    wm_band_weights(a, s_bw);
    wm_f4 acc[16];
    for (int l = 0; l < nl; l++) {
        const int out = wm_out(a, l), nt = (out + 15) >> 4, rpad = min(((nt + 3) >> 2) * 64, GS_WMLP_MAX_WIDTH);
        wm_zero(acc);
        if (l == 0) {
            for (int e0 = 0; e0 < E; e0 += WM_EC) {
                const int ew = min(WM_EC, E - e0), e4 = wm_pad(ew, 4);
                __syncthreads();  // (the band weights; the previous pass's reads)
                for (int idx = t; idx < WM_T * e4; idx += WM_THREADS) {
                    const int r = idx / e4, c = idx - r * e4;
                    s_act[r * WM_AS + c] = (r < n && c < ew) ? wm_enc(a, s_bw, a.x + (row0 + r) * d, e0 + c) : 0.0f;
                }
                for (int k0 = 0; k0 < ew; k0 += WM_KC) {
                    const int kw = min(WM_KC, ew - k0), k4 = wm_pad(kw, 4);
                    __syncthreads();
                    wm_load_weights(s_w, WM_WS_F, a.W[0] + e0 + k0, E + a.dim_cond, out, rpad, kw, k4);
                    __syncthreads();
                    wm_mm<false>(nt, arow + k0, s_w, WM_WS_F, k4 >> 2, acc);
                }
            }
        } else {
            for (int k0 = 0; k0 < W; k0 += WM_KC) {
                const int kw = min(WM_KC, W - k0);
                __syncthreads();
                wm_load_weights(s_w, WM_WS_F, a.W[l] + k0, W, out, rpad, kw, kw);
                __syncthreads();
                wm_mm<false>(nt, arow + k0, s_w, WM_WS_F, kw >> 2, acc);
            }
        }
        const float* bias = (l == 0 && b0) ? b0 : a.b[l];
        const bool hidden = l < nl - 1, feeds_skip = hidden && wm_skip(a, l + 1);
#pragma unroll
        for (int jt = 0; jt < 16; jt++) {
            if (jt < nt) {
                const int c = jt * 16 + col;
                if (c < out) {
                    const float bv = bias[c];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float v = acc[jt][r] + bv;
                        if (hidden) v = v > 0.0f ? v : v * a.slope;
                        if (feeds_skip) v = v / WM_SQRT2;
                        arow[(rq + r) * WM_AS + c] = v;
                    }
                }
            }
        }
        if (feeds_skip) {  // the next layer's input is [h | e] / sqrt(2): the encoding takes the W - out = E free columns
            for (int f = lane; f < 16 * E; f += 64) {
                const int r = f / E, c = f - r * E;
                arow[r * WM_AS + out + c] = r < n_wave ? wm_enc(a, s_bw, a.x + (row0 + wave * 16 + r) * d, c) / WM_SQRT2 : 0.0f;
            }
        }
        if (hidden && acts && n_wave > 0)
            wm_store_rows(arow, acts + ((size_t)l * a.N + row0 + wave * 16) * W, W, n_wave);
    }
    __syncthreads();
    for (int f = t; f < n * dout; f += WM_THREADS) {
        const int r = f / dout;
        y[row0 * dout + f] = s_act[r * WM_AS + (f - r * dout)];
    }
}

// `de`: the encoding's gradient, (N, E) -- dx itself at multires 0; NULL when dx is not wanted
__global__ __launch_bounds__(WM_THREADS) void wm_bwd_kernel(GsWideMlpArgs a, const float* __restrict__ acts, const float* __restrict__ g,
                                                            float* __restrict__ dz, float* de, int lowest) {
    __shared__ float4 s_dz4[WM_T * WM_AS / 4];
    __shared__ float4 s_w4[WM_KC * WM_WS_B / 4];
    __shared__ float s_bw[16];
    float* s_dz = reinterpret_cast<float*>(s_dz4);
    float* s_w = reinterpret_cast<float*>(s_w4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, wt = W >> 4, nl = a.n_hidden + 1, d = a.dim_x, dout = a.dim_out, E = wm_enc_dim(a);
    const size_t row0 = (size_t)blockIdx.x * WM_T;
    const int n = (int)min((size_t)WM_T, (size_t)a.N - row0);
    float* arow = s_dz + wave * 16 * WM_AS;
    const int n_wave = n - wave * 16;
    const size_t wrow0 = row0 + wave * 16;
    const int col = lane & 15, rq = (lane >> 4) * 4;
    wm_band_weights(a, s_bw);
    wm_f4 acc[16];
    bool de_written = false;
    wm_load_rows(s_dz, WM_AS, g + row0 * dout, n, WM_T, dout, 0, dout, wm_pad(dout, 4));
    for (int l = nl - 1; l > lowest; l--) {  // dz_{l-1} from dz_l
        const int out = wm_out(a, l), k4 = wm_pad(out, 4), outp = wm_out(a, l - 1);
        const bool skip = wm_skip(a, l);
        wm_zero(acc);
        for (int k0 = 0; k0 < k4; k0 += WM_KC) {
            const int kw = min(WM_KC, k4 - k0);
            __syncthreads();
            wm_load_weights(s_w, WM_WS_B, a.W[l] + (size_t)k0 * W, W, min(kw, out - k0), kw, W, W);
            __syncthreads();
            wm_mm<true>(wt, arow + k0, s_w, WM_WS_B, kw >> 2, acc);
        }
        const float* al = acts + ((size_t)(l - 1) * a.N + wrow0) * W;
#pragma unroll
        for (int jt = 0; jt < 16; jt++) {
            if (jt < wt) {
                const int c = jt * 16 + col;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool valid = rq + r < n_wave;
                    float dv = acc[jt][r];
                    if (skip) dv = dv / WM_SQRT2;
                    float keep = 0.0f;
                    if (c < outp) {
                        const float av = valid ? al[(size_t)(rq + r) * W + c] : 0.0f;
                        keep = av > 0.0f ? dv : dv * a.slope;
                    } else if (de && valid) {  // (a skip layer: c - outp < E)
                        float* p = de + (wrow0 + rq + r) * E + (c - outp);
                        *p = de_written ? *p + dv : dv;
                    }
                    arow[(rq + r) * WM_AS + c] = keep;
                }
            }
        }
        de_written = de_written || skip;
        if (n_wave > 0) wm_store_rows(arow, dz + ((size_t)(l - 1) * a.N + wrow0) * W, W, n_wave);
    }
    if (!de) return;  // (uniform)
    const int out0 = wm_out(a, 0), k4 = wm_pad(out0, 4), ld0 = E + a.dim_cond;
    for (int e0 = 0; e0 < E; e0 += WM_EC) {
        const int ew = min(WM_EC, E - e0), cpad = wm_pad(ew, 16);
        wm_zero(acc);
        for (int k0 = 0; k0 < k4; k0 += WM_KC) {
            const int kw = min(WM_KC, k4 - k0);
            __syncthreads();
            wm_load_weights(s_w, WM_WS_B, a.W[0] + (size_t)k0 * ld0 + e0, ld0, min(kw, out0 - k0), kw, ew, cpad);
            __syncthreads();
            wm_mm<true>(cpad >> 4, arow + k0, s_w, WM_WS_B, kw >> 2, acc);
        }
#pragma unroll
        for (int jt = 0; jt < 16; jt++) {
            const int c = jt * 16 + col;
            if (c < ew) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (rq + r < n_wave) {
                        float* p = de + (wrow0 + rq + r) * E + e0 + c;
                        *p = de_written ? *p + acc[jt][r] : acc[jt][r];
                    }
            }
        }
    }
    if (a.multires == 0) return;  // (de is dx)
    __syncthreads();              // the row's de is complete, and visible to the workgroup
    const int inc = a.include_input ? 1 : 0;
    for (int idx = t; idx < n * d; idx += WM_THREADS) {
        const int r = idx / d, j = idx - r * d;
        const float xv = a.x[(row0 + r) * d + j];
        const float* der = de + (row0 + r) * E + j;
        float s = inc ? der[0] : 0.0f;
        for (int k = 0; k < a.multires; k++) {
            const float f = (float)(1 << k), arg = xv * f;
            const float sn = sinf(arg), cs = cosf(arg);
            s = s + (f * s_bw[k]) * (cs * der[(inc + 2 * k) * d] - sn * der[(inc + 2 * k + 1) * d]);
        }
        a.dx[(row0 + r) * d + j] = s;
    }
}

// partial p = blockIdx.x of item blockIdx.y -- the block [o0, o0 + ow) x [c0, c0 + cw) of one layer's dW, and (with c0 == 0)
// db over the same outputs -- over the rows [p R, min(N, (p + 1) R))
__global__ __launch_bounds__(WM_THREADS) void wm_dw_kernel(GsWideMlpArgs a, const float* __restrict__ acts, const float* __restrict__ g,
                                                           const float* __restrict__ dz, int R, float* __restrict__ partial,
                                                           int part_floats) {
    __shared__ float4 s_d4[WM_RK * WM_DS / 4];
    __shared__ float4 s_a4[WM_RK * WM_DS / 4];
    __shared__ float s_bw[16];
    float* s_d = reinterpret_cast<float*>(s_d4);
    float* s_a = reinterpret_cast<float*>(s_a4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, nl = a.n_hidden + 1, d = a.dim_x;
    int item = blockIdx.y, l = 0, ni = 1;
    for (; l < nl; l++) {
        ni = wm_blocks(wm_in(a, l));
        const int cnt = ni * wm_blocks(wm_out(a, l));
        if (item < cnt) break;
        item -= cnt;
    }
    if (l >= nl) return;
    if (!(a.dW[l] || a.db[l] || (l == 0 && a.dim_cond > 0 && a.dcond))) return;
    const int o0 = (item / ni) * WM_DC, c0 = (item % ni) * WM_DC;
    const int out = wm_out(a, l), in = wm_in(a, l), ow = min(WM_DC, out - o0), cw = min(WM_DC, in - c0);
    const int opad = wm_pad(ow, 16), ipad = wm_pad(cw, 16), sd = wm_stride_b(opad), sa = wm_stride_b(ipad);
    const int ldz = l == nl - 1 ? out : W;
    const float* dzl = l == nl - 1 ? g : dz + (size_t)l * a.N * W;       // (N, ldz)
    const float* al = l == 0 ? a.x : acts + (size_t)(l - 1) * a.N * W;    // x (N, d), or v_l (N, W)
    wm_band_weights(a, s_bw);
    // the wave's job: output tile row ot, `gn` column tiles from it0
    const int ot_n = opad >> 4, it_n = ipad >> 4, q = WM_WAVES / ot_n, gsz = (it_n + q - 1) / q, jn = (it_n + gsz - 1) / gsz;
    const int ot = wave / jn, it0 = (wave - ot * jn) * gsz;
    const int gn = ot < ot_n ? min(gsz, it_n - it0) : 0;
    const size_t r_begin = (size_t)blockIdx.x * R, r_end = min((size_t)a.N, r_begin + R);
    wm_f4 acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = wm_f4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;
    for (size_t r0 = r_begin; r0 < r_end; r0 += WM_RK) {
        const int n = (int)min((size_t)WM_RK, r_end - r0);
        __syncthreads();
        wm_load_rows(s_d, sd, dzl + r0 * ldz, n, WM_RK, ldz, o0, ow, opad);
        if (l == 0) {
            for (int idx = t; idx < WM_RK * ipad; idx += WM_THREADS) {
                const int r = idx / ipad, c = idx - r * ipad;
                s_a[r * sa + c] = (r < n && c < cw) ? wm_enc(a, s_bw, al + (r0 + r) * d, c0 + c) : 0.0f;
            }
        } else {
            wm_load_rows(s_a, sa, al + r0 * W, n, WM_RK, W, c0, cw, ipad);
        }
        __syncthreads();
        if (gn > 0) {
            const float* dp = s_d + (lane >> 4) * sd + ot * 16 + (lane & 15);
            const float* ap = s_a + (lane >> 4) * sa + it0 * 16 + (lane & 15);
            for (int ks = 0; ks < WM_RK / 4; ks++) {
                const float dv = dp[4 * ks * sd];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k < gn) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, ap[4 * ks * sa + 16 * k], acc[k], 0, 0, 0);
            }
        }
        if (c0 == 0 && t < ow)
            for (int r = 0; r < n; r++) bsum += s_d[r * sd + t];
    }
    float* part = partial + (size_t)blockIdx.x * part_floats + wm_part_off(a, l);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (k < gn) {
            const int i = (it0 + k) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = ot * 16 + (lane >> 4) * 4 + r;
                if (o < ow && i < cw) part[(o0 + o) * in + c0 + i] = acc[k][r];
            }
        }
    }
    if (c0 == 0 && t < ow) part[out * in + o0 + t] = bsum;
}

// element e of [ W_0 | b_0 | W_1 | b_1 | .. | dcond ]: the partials in index order
__global__ __launch_bounds__(WM_FINAL_THREADS) void wm_final_kernel(GsWideMlpArgs a, const float* __restrict__ partial, int P,
                                                                    int part_floats, int total) {
    __shared__ float s_db0[GS_WMLP_MAX_WIDTH];
    const int t = threadIdx.x, nl = a.n_hidden + 1, E = wm_enc_dim(a), C = a.dim_cond, out0 = wm_out(a, 0);
    if (C > 0 && (a.dW[0] || a.dcond)) {  // (uniform)
        if (t < out0) {
            float s = 0.0f;
            for (int p = 0; p < P; p++) s += partial[(size_t)p * part_floats + out0 * E + t];
            s_db0[t] = s;
        }
        __syncthreads();
    }
    int e = blockIdx.x * WM_FINAL_THREADS + t;
    if (e >= total) return;
    for (int l = 0; l < nl; l++) {
        const int out = wm_out(a, l), in = wm_in(a, l), ld = wm_ld(a, l);
        if (e < out * ld) {
            if (!a.dW[l]) return;
            const int o = e / ld, i = e - o * ld;
            float s;
            if (i < in) {
                const float* p0 = partial + wm_part_off(a, l) + o * in + i;
                s = 0.0f;
                for (int p = 0; p < P; p++) s += p0[(size_t)p * part_floats];
            } else {
                s = s_db0[o] * a.cond[i - in];
            }
            a.dW[l][e] = s;
            return;
        }
        e -= out * ld;
        if (e < out) {
            if (!a.db[l]) return;
            const float* p0 = partial + wm_part_off(a, l) + out * in + e;
            float s = 0.0f;
            for (int p = 0; p < P; p++) s += p0[(size_t)p * part_floats];
            a.db[l][e] = s;
            return;
        }
        e -= out;
    }
    if (a.dcond) {  // e < C
        const float* w = a.W[0] + E + e;
        float s = 0.0f;
        for (int o = 0; o < out0; o++) s += w[(size_t)o * (E + C)] * s_db0[o];
        a.dcond[e] = s;
    }
}

// ---- launchers (the C ABI has checked every argument)
static int launch_wmlp_forward(const GsWideMlpArgs* a, float* y, float* acts, void* workspace, hipStream_t s) {
    StageScope st("wmlp", s);
    float* b0 = nullptr;
    if (a->dim_cond > 0) {
        b0 = reinterpret_cast<float*>(workspace);
        hipLaunchKernelGGL(wm_cond_kernel, dim3(wm_out(*a, 0)), dim3(64), 0, s, *a, b0);
        GS_LAUNCH_CHECK("wmlp_cond", 0, s);
    }
    hipLaunchKernelGGL(wm_fwd_kernel, dim3((a->N + WM_T - 1) / WM_T), dim3(WM_THREADS), 0, s, *a, b0, y, acts);
    GS_LAUNCH_CHECK("wmlp", 0, s);
    return GS_OK;
}
static int launch_wmlp_backward(const GsWideMlpArgs* a, const float* acts, const float* g, void* workspace, hipStream_t s) {
    StageScope st("wmlp_bwd", s);
    const int nl = a->n_hidden + 1, lowest = wm_lowest(*a);
    if (lowest > a->n_hidden) return GS_OK;
    float* dz = reinterpret_cast<float*>(workspace);
    float* de_ws = dz + (size_t)a->n_hidden * a->N * a->width;
    float* partial = de_ws + (a->multires > 0 ? (size_t)a->N * wm_enc_dim(*a) : 0);
    float* de = !a->dx ? nullptr : (a->multires > 0 ? de_ws : a->dx);
    const int R = wm_rows_per_partial(a->N), P = wm_partials(a->N), part_floats = wm_part_off(*a, nl);
    if (lowest < a->n_hidden || a->dx) {
        hipLaunchKernelGGL(wm_bwd_kernel, dim3((a->N + WM_T - 1) / WM_T), dim3(WM_THREADS), 0, s, *a, acts, g, dz, de, lowest);
        GS_LAUNCH_CHECK("wmlp_bwd", 0, s);
    }
    bool any = false;
    for (int l = 0; l < nl; l++) any = any || wm_wanted(*a, l);
    if (!any) return GS_OK;
    hipLaunchKernelGGL(wm_dw_kernel, dim3(P, wm_items(*a)), dim3(WM_THREADS), 0, s, *a, acts, g, dz, R, partial, part_floats);
    GS_LAUNCH_CHECK("wmlp_dw", 0, s);
    int total = a->dim_cond;
    for (int l = 0; l < nl; l++) total += wm_out(*a, l) * (wm_ld(*a, l) + 1);
    hipLaunchKernelGGL(wm_final_kernel, dim3((total + WM_FINAL_THREADS - 1) / WM_FINAL_THREADS), dim3(WM_FINAL_THREADS), 0, s, *a,
                       partial, P, part_floats, total);
    GS_LAUNCH_CHECK("wmlp_final", 0, s);
    return GS_OK;
}

extern "C" {

static int wmlp_validate(const GsWideMlpArgs* a) {
    if (!a || a->N < 0 || a->width < 32 || a->width > GS_WMLP_MAX_WIDTH || a->width % 32 != 0 || a->n_hidden < 1 ||
        a->n_hidden > GS_WMLP_MAX_HIDDEN || a->dim_x < 1 || a->dim_x > GS_WMLP_MAX_ENC || a->multires < 0 ||
        a->multires > GS_WMLP_MAX_FREQS || (a->include_input != 0 && a->include_input != 1) || a->dim_cond < 0 ||
        a->dim_cond > GS_WMLP_MAX_COND || a->dim_out < 1 || a->dim_out > GS_WMLP_MAX_OUT || !(a->slope >= 0.0f) ||
        !(a->slope < INFINITY))
        return GS_E_BAD_ARG;
    const int E = wm_enc_dim(*a);
    if (E < 1 || E > GS_WMLP_MAX_ENC) return GS_E_BAD_ARG;
    // a skip at layer 0 or past the last linear; a skip whose encoding leaves the layer before it no outputs
    if ((a->skip_mask & 1u) || (a->skip_mask >> (a->n_hidden + 1)) != 0 || (a->skip_mask != 0 && E >= a->width)) return GS_E_BAD_ARG;
    for (int k = 0; k < a->multires; k++)
        if (!(a->band_w[k] == a->band_w[k])) return GS_E_BAD_ARG;
    return GS_OK;
}
// x, the condition and every layer's parameters
static bool wmlp_inputs_ok(const GsWideMlpArgs* a) {
    if (!required(a->x, 4) || (a->dim_cond > 0 && !required(a->cond, 4))) return false;
    for (int l = 0; l <= a->n_hidden; l++)
        if (!required(a->W[l], 4) || !required(a->b[l], 4)) return false;
    return true;
}
int gs_wmlp_workspace_bytes(const GsWideMlpArgs* a, int32_t backward, size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    if (const int rc = wmlp_validate(a)) return rc;
    *out = wmlp_workspace_bytes(a, backward != 0);
    return GS_OK;
}
int gs_wmlp_saved_bytes(const GsWideMlpArgs* a, size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    if (const int rc = wmlp_validate(a)) return rc;
    *out = wmlp_saved_bytes(a);
    return GS_OK;
}
int gs_wmlp_forward(const GsWideMlpArgs* a, float* y, float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = wmlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!wmlp_inputs_ok(a) || !required(y, 4) || !aligned(saved, 16)) return GS_E_BAD_ARG;
    if (a->dim_cond > 0) {
        if (!required(workspace, 4)) return GS_E_BAD_ARG;
        if (workspace_bytes < wmlp_workspace_bytes(a, 0)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    return launch_wmlp_forward(a, y, saved, workspace, (hipStream_t)stream);
}
int gs_wmlp_backward(const GsWideMlpArgs* a, const float* saved, const float* dL_dy, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (const int rc = wmlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!wmlp_inputs_ok(a) || !required(saved, 16) || !required(dL_dy, 16) || !aligned(a->dx, 4) || !aligned(a->dcond, 4))
        return GS_E_BAD_ARG;
    if (a->dcond && a->dim_cond == 0) return GS_E_BAD_ARG;
    bool any = a->dx || a->dcond;
    for (int l = 0; l <= a->n_hidden; l++) {
        if (!aligned(a->dW[l], 4) || !aligned(a->db[l], 4)) return GS_E_BAD_ARG;
        any = any || a->dW[l] || a->db[l];
    }
    if (any) {
        if (!required(workspace, 16)) return GS_E_BAD_ARG;
        if (workspace_bytes < wmlp_workspace_bytes(a, 1)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    if (!any) return GS_OK;
    return launch_wmlp_backward(a, saved, dL_dy, workspace, (hipStream_t)stream);
}

}  // extern "C"
