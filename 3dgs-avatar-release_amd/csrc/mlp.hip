// mlp.hip -- the dense networks of the avatar model (models/network_utils.py VanillaCondMLP :182-249: the skinning
// field, the non-rigid deformer's MLP, the colour MLP) as one fused op on the exact-fp32 MFMA: one forward launch that keeps
// a row tile's activations on chip from the input to the output, and a three-launch backward without atomics, instead of
// an addmm and a leaky_relu per layer (and a cat and an expand for the condition) that each write and re-read an (N, W)
// matrix, and about twice that in the autograd replay.
//
// Spec (fp32 throughout; every array row-major and contiguous).  n_hidden hidden layers of one width W, nl = n_hidden + 1
// linear layers, nn.Linear layouts:
//   W_0 (W, din + C), b_0 (W);  W_l (W, W), b_l (W) for 0 < l < nl - 1;  W_{nl-1} (dout, W), b_{nl-1} (dout)
//   y = L_{nl-1}( leaky( .. leaky( L_0([x | cond]) ) .. ) ),  L_l(v) = v W_l^T + b_l,  leaky(z) = z > 0 ? z : slope z
//   (no activation after the last layer).  x (N, din); cond (C,) is ONE row that every row of x shares (C may be 0).
//   Supported: W a multiple of 32 in 32..GS_MLP_MAX_WIDTH, 1..GS_MLP_MAX_HIDDEN hidden layers, din in 1..GS_MLP_MAX_IN, C in
//   0..GS_MLP_MAX_COND, dout in 1..GS_MLP_MAX_OUT.  Everything else is the caller's business (gsplat_mi355/mlp.py falls back).
// The condition is never expanded: z_0 = x W_0[:, :din]^T + b0',  b0' = b_0 + W_0[:, din:] cond, formed once per launch.
// Backward from g = dL/dy (N, dout), with a_l the post-activation of hidden layer l (a_{-1} = x) and dz_l = dL/dz_l:
//   dz_{nl-1} = g;  dz_{l-1} = (dz_l W_l) * (a_{l-1} > 0 ? 1 : slope)     (a > 0 <=> z > 0; a == 0 takes the slope, as torch
//                                                                          does at z == 0)
//   dW_l = dz_l^T a_{l-1},  db_l = the column sums of dz_l;  dx = dz_0 W_0[:, :din];
//   dW_0[:, din:] = db_0 (x) cond;  dcond = W_0[:, din:]^T db_0.          No (N, din + C) matrix exists in either direction.
//   A gradient nobody asked for (NULL) is neither computed nor written; the walk stops at the lowest layer somebody asked for.
// What the forward saves: the hidden post-activations a_0 .. a_{n_hidden-1}, (n_hidden, N, W), when the caller hands a
//   buffer.  Recomputing them in the backward would need every layer of a tile on chip at once (6 x 128 x 128 floats =
//   384 KiB against 160 KiB of LDS) or one more forward GEMM chain at the fp32 matrix rate, which costs more than
//   writing and reading N W floats per layer at memory speed.
// Kernels (ML_THREADS = 512 threads, 8 waves; every product on __builtin_amdgcn_mfma_f32_16x16x4f32, whose result is a
// k-ordered fmaf chain):
//   ml_cond_kernel   b0' (W blocks of one wave: lane c, c + 64, .. in order, then the DPP ladder).  Only with C > 0.
//   ml_fwd_kernel    a workgroup owns ML_T = 128 consecutive rows, 16 per wave.  Its rows of x are one contiguous slab
//                    that starts 16-byte aligned for every din and is read with 16-byte loads into LDS (zero-padded to the
//                    MFMA's k step; din > ML_KC is streamed in chunks of ML_KC columns, the accumulators staying in
//                    registers).  Per layer the weights are staged in LDS, each wave multiplies its 16 rows by all of them,
//                    adds the bias, applies the LeakyReLU and writes the result over its own rows in LDS (and to the saved
//                    activations, its 16 rows being one contiguous block); the last layer's rows go out through LDS.
//   ml_bwd_kernel    the same tile walks back: g comes into LDS, per layer dz_l W_l against the staged weights, the mask from
//                    the saved a_{l-1}, the result over the wave's own rows and out to dz_{l-1} in the workspace; at the
//                    bottom dx in chunks of ML_KC columns, straight from the accumulators.
//   ml_dw_kernel     split-K: workgroup (p, item) sums dz_l^T a_{l-1} and the columns of dz_l over the rows [p R, (p + 1) R)
//                    in row order (ML_RK rows staged per step) into partial p.  An item is a layer, layer 0 once per chunk of
//                    ML_KC input columns.  R = max(GS_MLP_PARTIAL_MIN_ROWS, ceil(N / GS_MLP_MAX_PARTIALS) rounded up to
//                    ML_RK): at most GS_MLP_MAX_PARTIALS partials, a function of N alone -- never of the device.
//   ml_final_kernel  one thread per parameter element: the partials in index order; the condition's columns of dW_0 and
//                    dcond from db_0, which every workgroup that needs it sums first (the same order, the same bits).
// No atomics, no memsets, no host synchronisation, no host memory traffic: every output is bitwise reproducible and the
// calls are capture-safe.  LDS strides are chosen so that the MFMA operand reads (16 lanes along one index, 4 along the
// other) touch 64 distinct banks: 4 x odd where the 16 lanes walk rows, 16 mod 32 where they walk columns.
#include "common.h"
#include "boundary.h"

#define ML_THREADS 512
#define ML_WAVES 8
#define ML_T GS_MLP_TILE_ROWS
#define ML_KC 128                          // input columns per chunk of the first layer
#define ML_AS 132                          // row stride of the activation tile: 4 x 33
#define ML_WS_F 132                        // widest forward weight stride
#define ML_WS_B 144                        // widest backward weight stride
#define ML_RK 32                           // rows staged per step of the dW kernel
#define ML_FINAL_THREADS 256
static_assert(ML_T == 16 * ML_WAVES, "a wave owns 16 rows of the tile");
static_assert(GS_MLP_MAX_WIDTH == ML_KC && GS_MLP_MAX_WIDTH % 32 == 0, "one weight tile holds the widest layer");
static_assert(GS_MLP_MAX_OUT <= 64 && GS_MLP_MAX_OUT % 16 == 0, "the output layer is at most four column tiles");
static_assert(GS_MLP_PARTIAL_MIN_ROWS % ML_RK == 0 && ML_RK % 4 == 0, "row chunks start 16-byte aligned");

typedef float ml_f4 __attribute__((ext_vector_type(4)));

// ---- shapes (host and device)
__host__ __device__ static inline int ml_in(const GsMlpArgs& a, int l) { return l == 0 ? a.dim_in : a.width; }
__host__ __device__ static inline int ml_ld(const GsMlpArgs& a, int l) { return l == 0 ? a.dim_in + a.dim_cond : a.width; }
__host__ __device__ static inline int ml_out(const GsMlpArgs& a, int l) { return l == a.n_hidden ? a.dim_out : a.width; }
__host__ __device__ static inline int ml_pad(int v, int m) { return (v + m - 1) / m * m; }
// row strides: the 16 lanes walk rows, the 4 lane groups columns (k4 a multiple of 4) / the other way round
__host__ __device__ static inline int ml_stride_f(int k4) { return 4 * ((k4 >> 2) | 1); }
__host__ __device__ static inline int ml_stride_b(int w) { return (w + 15) / 32 * 32 + 16; }
// floats of one partial: per layer the x part of dW_l, then db_l; the offset of layer l in it
__host__ __device__ static inline int ml_part_off(const GsMlpArgs& a, int l) {
    int off = 0;
    for (int k = 0; k < l; k++) off += ml_out(a, k) * (ml_in(a, k) + 1);
    return off;
}
static inline int ml_rows_per_partial(int N) {
    const int r = ml_pad((N + GS_MLP_MAX_PARTIALS - 1) / GS_MLP_MAX_PARTIALS, ML_RK);
    return r > GS_MLP_PARTIAL_MIN_ROWS ? r : GS_MLP_PARTIAL_MIN_ROWS;
}
static inline int ml_partials(int N) {
    const int R = ml_rows_per_partial(N);
    return (N + R - 1) / R;
}
static inline bool ml_wanted(const GsMlpArgs& a, int l) { return a.dW[l] || a.db[l] || (l == 0 && a.dim_cond > 0 && a.dcond); }
// the lowest layer whose dz somebody needs (n_hidden + 1: nobody)
static inline int ml_lowest(const GsMlpArgs& a) {
    if (a.dx) return 0;
    for (int l = 0; l <= a.n_hidden; l++)
        if (ml_wanted(a, l)) return l;
    return a.n_hidden + 1;
}
static size_t mlp_workspace_bytes(const GsMlpArgs* a, int backward) {
    if (a->N == 0) return 0;
    if (!backward) return a->dim_cond > 0 ? (size_t)a->width * sizeof(float) : 0;
    // dz_0 .. dz_{n_hidden-1}, then the partials
    return ((size_t)a->n_hidden * a->N * a->width + (size_t)ml_partials(a->N) * ml_part_off(*a, a->n_hidden + 1)) * sizeof(float);
}

// ---- staging
// Columns [c0, c0 + cw) of n rows of a contiguous (., ld) slab at src (16-byte aligned) -> dst[r * S + c], read in aligned
// 16-byte units (a row's segment takes (cw + 3) / 4 + 1 of them at most); columns cw .. cpad - 1 and rows n .. rows - 1 are
// zeroed.
__device__ __forceinline__ void ml_load_rows(float* dst, int S, const float* __restrict__ src, int n, int rows, int ld, int c0,
                                             int cw, int cpad) {
    const int t = threadIdx.x, U = (cw + 3) / 4 + 1, total = n * ld;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int idx = t; idx < n * U; idx += ML_THREADS) {
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
    for (int idx = t; idx < rows * cpad; idx += ML_THREADS) {
        const int r = idx / cpad, c = idx - r * cpad;
        if (r >= n || c >= cw) dst[r * S + c] = 0.0f;
    }
}
// rows x cols of a weight matrix at src (row stride ld) -> dst[r * S + c]; rows .. rpad - 1 and columns cols .. cpad - 1 are
// zeroed.  16-byte loads where the layout allows them (the hidden layers always do).
__device__ __forceinline__ void ml_load_weights(float* dst, int S, const float* __restrict__ src, int ld, int rows, int rpad,
                                                int cols, int cpad) {
    const int t = threadIdx.x;
    if (((ld | cols | cpad) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int c4 = cpad >> 2;
        for (int idx = t; idx < rpad * c4; idx += ML_THREADS) {
            const int r = idx / c4, c = 4 * (idx - r * c4);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < rows && c < cols) v = *reinterpret_cast<const float4*>(src + (size_t)r * ld + c);
            *reinterpret_cast<float4*>(dst + r * S + c) = v;
        }
    } else {
        for (int idx = t; idx < rpad * cpad; idx += ML_THREADS) {
            const int r = idx / cpad, c = idx - r * cpad;
            dst[r * S + c] = (r < rows && c < cols) ? src[(size_t)r * ld + c] : 0.0f;
        }
    }
}

// ---- products: the wave's 16 rows `arow` (row stride ML_AS) times NT column tiles of 16, over `ksteps` steps of 4.
// BWD = false: w[j * ws + k] (a Linear's weight as stored: out = a W^T);  BWD = true: w[k * ws + j] (out = a W).
template <int NT, bool BWD>
__device__ __forceinline__ void ml_mm_n(const float* arow, const float* w, int ws, int ksteps, ml_f4* acc) {
    const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
    const float* ap = arow + i * ML_AS + kq;
    const float* wp = BWD ? w + kq * ws + i : w + i * ws + kq;
    const int wk = BWD ? 4 * ws : 4, wj = BWD ? 16 : 16 * ws;
    for (int ks = 0; ks < ksteps; ks++) {
        const float av = ap[4 * ks];
#pragma unroll
        for (int jt = 0; jt < NT; jt++) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wp[ks * wk + jt * wj], acc[jt], 0, 0, 0);
    }
}
template <bool BWD>
__device__ __forceinline__ void ml_mm(int nt, const float* arow, const float* w, int ws, int ksteps, ml_f4* acc) {
    switch (nt) {  // (wave-uniform)
        case 1: ml_mm_n<1, BWD>(arow, w, ws, ksteps, acc); break;
        case 2: ml_mm_n<2, BWD>(arow, w, ws, ksteps, acc); break;
        case 3: ml_mm_n<3, BWD>(arow, w, ws, ksteps, acc); break;
        case 4: ml_mm_n<4, BWD>(arow, w, ws, ksteps, acc); break;
        case 5: ml_mm_n<5, BWD>(arow, w, ws, ksteps, acc); break;
        case 6: ml_mm_n<6, BWD>(arow, w, ws, ksteps, acc); break;
        case 7: ml_mm_n<7, BWD>(arow, w, ws, ksteps, acc); break;
        default: ml_mm_n<8, BWD>(arow, w, ws, ksteps, acc); break;
    }
}
__device__ __forceinline__ void ml_zero(ml_f4* acc) {
#pragma unroll
    for (int jt = 0; jt < 8; jt++) acc[jt] = ml_f4{0.0f, 0.0f, 0.0f, 0.0f};
}
// the wave's 16 rows of the tile (W floats each, n_valid of them real) -> one contiguous block at dst, 16 bytes a lane
__device__ __forceinline__ void ml_store_rows(const float* arow, float* __restrict__ dst, int W, int n_valid) {
    const int lane = threadIdx.x & 63, w4 = W >> 2;
    for (int f = lane; f < 16 * w4; f += 64) {
        const int r = f / w4, c = 4 * (f - r * w4);
        if (r < n_valid) *reinterpret_cast<float4*>(dst + (size_t)r * W + c) = *reinterpret_cast<const float4*>(arow + r * ML_AS + c);
    }
}

// b0'[o] = b_0[o] + sum_c W_0[o][din + c] cond[c], o = blockIdx.x
__global__ __launch_bounds__(64) void ml_cond_kernel(GsMlpArgs a, float* __restrict__ b0) {
    const int o = blockIdx.x, lane = threadIdx.x;
    const float* w = a.W[0] + (size_t)o * (a.dim_in + a.dim_cond) + a.dim_in;
    float acc = 0.0f;
    for (int c = lane; c < a.dim_cond; c += 64) acc += w[c] * a.cond[c];
    acc = wave_sum(acc);
    if (lane == 0) b0[o] = a.b[0][o] + acc;
}

__global__ __launch_bounds__(ML_THREADS) void ml_fwd_kernel(GsMlpArgs a, const float* __restrict__ b0, float* __restrict__ y,
                                                            float* __restrict__ acts) {
    __shared__ float4 s_act4[ML_T * ML_AS / 4];
    __shared__ float4 s_w4[GS_MLP_MAX_WIDTH * ML_WS_F / 4];
    float* s_act = reinterpret_cast<float*>(s_act4);
    float* s_w = reinterpret_cast<float*>(s_w4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, wt = W >> 4, nl = a.n_hidden + 1, din = a.dim_in, dout = a.dim_out;
    const size_t row0 = (size_t)blockIdx.x * ML_T;
    const int n = (int)min((size_t)ML_T, (size_t)a.N - row0);
    float* arow = s_act + wave * 16 * ML_AS;
    const int n_wave = n - wave * 16;  // (may be <= 0)
    const int col = lane & 15, rq = (lane >> 4) * 4;
    ml_f4 acc[8];
    for (int l = 0; l < nl; l++) {
        const int out = ml_out(a, l), nt = l == nl - 1 ? (out + 15) >> 4 : wt;
        ml_zero(acc);
        if (l == 0) {
            for (int c0 = 0; c0 < din; c0 += ML_KC) {
                const int cw = min(ML_KC, din - c0), k4 = ml_pad(cw, 4), ws = ml_stride_f(k4);
                __syncthreads();
                ml_load_rows(s_act, ML_AS, a.x + row0 * din, n, ML_T, din, c0, cw, k4);
                ml_load_weights(s_w, ws, a.W[0] + c0, din + a.dim_cond, W, W, cw, k4);
                __syncthreads();
                ml_mm<false>(nt, arow, s_w, ws, k4 >> 2, acc);
            }
        } else {
            __syncthreads();
            ml_load_weights(s_w, ML_WS_F, a.W[l], W, out, nt * 16, W, W);
            __syncthreads();
            ml_mm<false>(nt, arow, s_w, ML_WS_F, W >> 2, acc);
        }
        const float* bias = (l == 0 && b0) ? b0 : a.b[l];
        const bool hidden = l < nl - 1;
#pragma unroll
        for (int jt = 0; jt < 8; jt++) {
            if (jt < nt) {
                const int c = jt * 16 + col;
                const float bv = c < out ? bias[c] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[jt][r] + bv;
                    if (hidden) v = v > 0.0f ? v : v * a.slope;
                    arow[(rq + r) * ML_AS + c] = v;
                }
            }
        }
        if (hidden && acts && n_wave > 0)
            ml_store_rows(arow, acts + ((size_t)l * a.N + row0 + wave * 16) * W, W, n_wave);
    }
    __syncthreads();
    for (int f = t; f < n * dout; f += ML_THREADS) {
        const int r = f / dout;
        y[row0 * dout + f] = s_act[r * ML_AS + (f - r * dout)];
    }
}

__global__ __launch_bounds__(ML_THREADS) void ml_bwd_kernel(GsMlpArgs a, const float* __restrict__ acts, const float* __restrict__ g,
                                                            float* __restrict__ dz, int lowest) {
    __shared__ float4 s_dz4[ML_T * ML_AS / 4];
    __shared__ float4 s_w4[GS_MLP_MAX_WIDTH * ML_WS_B / 4];
    float* s_dz = reinterpret_cast<float*>(s_dz4);
    float* s_w = reinterpret_cast<float*>(s_w4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, wt = W >> 4, nl = a.n_hidden + 1, din = a.dim_in, dout = a.dim_out;
    const size_t row0 = (size_t)blockIdx.x * ML_T;
    const int n = (int)min((size_t)ML_T, (size_t)a.N - row0);
    float* arow = s_dz + wave * 16 * ML_AS;
    const int n_wave = n - wave * 16;
    const int col = lane & 15, rq = (lane >> 4) * 4;
    ml_f4 acc[8];
    ml_load_rows(s_dz, ML_AS, g + row0 * dout, n, ML_T, dout, 0, dout, ml_pad(dout, 4));
    for (int l = nl - 1; l > lowest; l--) {  // dz_{l-1} from dz_l
        const int out = ml_out(a, l), k4 = ml_pad(out, 4), ws = ml_stride_b(W);
        __syncthreads();
        ml_load_weights(s_w, ws, a.W[l], W, out, k4, W, W);
        __syncthreads();
        ml_zero(acc);
        ml_mm<true>(wt, arow, s_w, ws, k4 >> 2, acc);
        const float* al = acts + ((size_t)(l - 1) * a.N + row0 + wave * 16) * W;
#pragma unroll
        for (int jt = 0; jt < 8; jt++) {
            if (jt < wt) {
                const int c = jt * 16 + col;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float av = rq + r < n_wave ? al[(size_t)(rq + r) * W + c] : 0.0f;
                    arow[(rq + r) * ML_AS + c] = av > 0.0f ? acc[jt][r] : acc[jt][r] * a.slope;
                }
            }
        }
        if (n_wave > 0) ml_store_rows(arow, dz + ((size_t)(l - 1) * a.N + row0 + wave * 16) * W, W, n_wave);
    }
    if (a.dx) {
        for (int c0 = 0; c0 < din; c0 += ML_KC) {
            const int cw = min(ML_KC, din - c0), cpad = ml_pad(cw, 16), ws = ml_stride_b(cpad);
            __syncthreads();
            ml_load_weights(s_w, ws, a.W[0] + c0, din + a.dim_cond, W, W, cw, cpad);
            __syncthreads();
            ml_zero(acc);
            ml_mm<true>(cpad >> 4, arow, s_w, ws, W >> 2, acc);
#pragma unroll
            for (int jt = 0; jt < 8; jt++) {
                const int c = jt * 16 + col;
                if (c < cw) {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (rq + r < n_wave) a.dx[(row0 + wave * 16 + rq + r) * din + c0 + c] = acc[jt][r];
                }
            }
        }
    }
}

// partial p of item blockIdx.y: dW_l[:, c0 : c0 + cw] and (with c0 == 0) db_l over the rows [p R, min(N, (p + 1) R))
__global__ __launch_bounds__(ML_THREADS) void ml_dw_kernel(GsMlpArgs a, const float* __restrict__ acts, const float* __restrict__ g,
                                                           const float* __restrict__ dz, int R, float* __restrict__ partial,
                                                           int part_floats) {
    __shared__ float4 s_d4[ML_RK * ML_WS_B / 4];
    __shared__ float4 s_a4[ML_RK * ML_WS_B / 4];
    float* s_d = reinterpret_cast<float*>(s_d4);
    float* s_a = reinterpret_cast<float*>(s_a4);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int W = a.width, nl = a.n_hidden + 1, din = a.dim_in;
    const int chunks0 = (din + ML_KC - 1) / ML_KC;
    const int l = (int)blockIdx.y < chunks0 ? 0 : (int)blockIdx.y - chunks0 + 1;
    const int c0 = l == 0 ? (int)blockIdx.y * ML_KC : 0;
    if (!(a.dW[l] || a.db[l] || (l == 0 && a.dim_cond > 0 && a.dcond))) return;
    const int out = ml_out(a, l), in = ml_in(a, l), cw = min(ML_KC, in - c0);
    const int opad = ml_pad(out, 16), ipad = ml_pad(cw, 16), sd = ml_stride_b(opad), sa = ml_stride_b(ipad);
    const float* dzl = l == nl - 1 ? g : dz + (size_t)l * a.N * W;  // (N, out)
    const float* al = l == 0 ? a.x : acts + (size_t)(l - 1) * a.N * W;  // (N, in)
    // the wave's job: output tile row ot, `gn` column tiles from it0 (ot_n jobs-per-row groups of gsz)
    const int ot_n = opad >> 4, it_n = ipad >> 4, q = ML_WAVES / ot_n, gsz = (it_n + q - 1) / q, jn = (it_n + gsz - 1) / gsz;
    const int ot = wave / jn, it0 = (wave - ot * jn) * gsz;
    const int gn = ot < ot_n ? min(gsz, it_n - it0) : 0;
    const size_t r_begin = (size_t)blockIdx.x * R, r_end = min((size_t)a.N, r_begin + R);
    ml_f4 acc[8];
    ml_zero(acc);
    float bsum = 0.0f;
    for (size_t r0 = r_begin; r0 < r_end; r0 += ML_RK) {
        const int n = (int)min((size_t)ML_RK, r_end - r0);
        __syncthreads();
        ml_load_rows(s_d, sd, dzl + r0 * out, n, ML_RK, out, 0, out, opad);
        ml_load_rows(s_a, sa, al + r0 * in, n, ML_RK, in, c0, cw, ipad);
        __syncthreads();
        if (gn > 0) {
            const float* dp = s_d + (lane >> 4) * sd + ot * 16 + (lane & 15);
            const float* ap = s_a + (lane >> 4) * sa + it0 * 16 + (lane & 15);
            for (int ks = 0; ks < ML_RK / 4; ks++) {
                const float dv = dp[4 * ks * sd];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k < gn) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, ap[4 * ks * sa + 16 * k], acc[k], 0, 0, 0);
            }
        }
        if (c0 == 0 && t < out)
            for (int r = 0; r < n; r++) bsum += s_d[r * sd + t];
    }
    float* part = partial + (size_t)blockIdx.x * part_floats + ml_part_off(a, l);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (k < gn) {
            const int i = (it0 + k) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = ot * 16 + (lane >> 4) * 4 + r;
                if (o < out && i < cw) part[o * in + c0 + i] = acc[k][r];
            }
        }
    }
    if (c0 == 0 && t < out) part[out * in + t] = bsum;
}

// element e of [ W_0 | b_0 | W_1 | b_1 | .. | dcond ]: the partials in index order
__global__ __launch_bounds__(ML_FINAL_THREADS) void ml_final_kernel(GsMlpArgs a, const float* __restrict__ partial, int P,
                                                                    int part_floats, int total) {
    __shared__ float s_db0[GS_MLP_MAX_WIDTH];
    const int t = threadIdx.x, nl = a.n_hidden + 1, din = a.dim_in, C = a.dim_cond, W = a.width;
    if (C > 0 && (a.dW[0] || a.dcond)) {  // (uniform)
        if (t < W) {
            float s = 0.0f;
            for (int p = 0; p < P; p++) s += partial[(size_t)p * part_floats + W * din + t];
            s_db0[t] = s;
        }
        __syncthreads();
    }
    int e = blockIdx.x * ML_FINAL_THREADS + t;
    if (e >= total) return;
    for (int l = 0; l < nl; l++) {
        const int out = ml_out(a, l), in = ml_in(a, l), ld = ml_ld(a, l);
        if (e < out * ld) {
            if (!a.dW[l]) return;
            const int o = e / ld, i = e - o * ld;
            float s;
            if (i < in) {
                const float* p0 = partial + ml_part_off(a, l) + o * in + i;
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
            const float* p0 = partial + ml_part_off(a, l) + out * in + e;
            float s = 0.0f;
            for (int p = 0; p < P; p++) s += p0[(size_t)p * part_floats];
            a.db[l][e] = s;
            return;
        }
        e -= out;
    }
    if (a.dcond) {  // e < C
        const float* w = a.W[0] + din + e;
        float s = 0.0f;
        for (int o = 0; o < W; o++) s += w[(size_t)o * (din + C)] * s_db0[o];
        a.dcond[e] = s;
    }
}

// ---- launchers (the C ABI has checked every argument)
static int launch_mlp_forward(const GsMlpArgs* a, float* y, float* acts, void* workspace, hipStream_t s) {
    StageScope st("mlp", s);
    float* b0 = nullptr;
    if (a->dim_cond > 0) {
        b0 = reinterpret_cast<float*>(workspace);
        hipLaunchKernelGGL(ml_cond_kernel, dim3(a->width), dim3(64), 0, s, *a, b0);
        GS_LAUNCH_CHECK("mlp_cond", 0, s);
    }
    hipLaunchKernelGGL(ml_fwd_kernel, dim3((a->N + ML_T - 1) / ML_T), dim3(ML_THREADS), 0, s, *a, b0, y, acts);
    GS_LAUNCH_CHECK("mlp", 0, s);
    return GS_OK;
}
static int launch_mlp_backward(const GsMlpArgs* a, const float* acts, const float* g, void* workspace, hipStream_t s) {
    StageScope st("mlp_bwd", s);
    const int nl = a->n_hidden + 1, lowest = ml_lowest(*a);
    if (lowest > a->n_hidden) return GS_OK;
    float* dz = reinterpret_cast<float*>(workspace);
    float* partial = dz + (size_t)a->n_hidden * a->N * a->width;
    const int R = ml_rows_per_partial(a->N), P = ml_partials(a->N), part_floats = ml_part_off(*a, nl);
    if (lowest < a->n_hidden || a->dx) {
        hipLaunchKernelGGL(ml_bwd_kernel, dim3((a->N + ML_T - 1) / ML_T), dim3(ML_THREADS), 0, s, *a, acts, g, dz, lowest);
        GS_LAUNCH_CHECK("mlp_bwd", 0, s);
    }
    bool any = false;
    for (int l = 0; l < nl; l++) any = any || ml_wanted(*a, l);
    if (!any) return GS_OK;
    const int items = (a->dim_in + ML_KC - 1) / ML_KC + a->n_hidden;
    hipLaunchKernelGGL(ml_dw_kernel, dim3(P, items), dim3(ML_THREADS), 0, s, *a, acts, g, dz, R, partial, part_floats);
    GS_LAUNCH_CHECK("mlp_dw", 0, s);
    int total = a->dim_cond;
    for (int l = 0; l < nl; l++) total += ml_out(*a, l) * (ml_ld(*a, l) + 1);
    hipLaunchKernelGGL(ml_final_kernel, dim3((total + ML_FINAL_THREADS - 1) / ML_FINAL_THREADS), dim3(ML_FINAL_THREADS), 0, s, *a,
                       partial, P, part_floats, total);
    GS_LAUNCH_CHECK("mlp_final", 0, s);
    return GS_OK;
}

extern "C" {

static int mlp_validate(const GsMlpArgs* a) {
    if (!a || a->N < 0 || a->width < 32 || a->width > GS_MLP_MAX_WIDTH || a->width % 32 != 0 || a->n_hidden < 1 ||
        a->n_hidden > GS_MLP_MAX_HIDDEN || a->dim_in < 1 || a->dim_in > GS_MLP_MAX_IN || a->dim_cond < 0 ||
        a->dim_cond > GS_MLP_MAX_COND || a->dim_out < 1 || a->dim_out > GS_MLP_MAX_OUT || !(a->slope == a->slope))
        return GS_E_BAD_ARG;
    return GS_OK;
}
// x, the condition and every layer's parameters
static bool mlp_inputs_ok(const GsMlpArgs* a) {
    if (!required(a->x, 16) || (a->dim_cond > 0 && !required(a->cond, 4))) return false;
    for (int l = 0; l <= a->n_hidden; l++)
        if (!required(a->W[l], 4) || !required(a->b[l], 4)) return false;
    return true;
}
int gs_mlp_workspace_bytes(const GsMlpArgs* a, int32_t backward, size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    if (const int rc = mlp_validate(a)) return rc;
    *out = mlp_workspace_bytes(a, backward != 0);
    return GS_OK;
}
int gs_mlp_forward(const GsMlpArgs* a, float* y, float* acts, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!mlp_inputs_ok(a) || !required(y, 4) || !aligned(acts, 16)) return GS_E_BAD_ARG;
    if (a->dim_cond > 0) {
        if (!required(workspace, 4)) return GS_E_BAD_ARG;
        if (workspace_bytes < mlp_workspace_bytes(a, 0)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    return launch_mlp_forward(a, y, acts, workspace, (hipStream_t)stream);
}
int gs_mlp_backward(const GsMlpArgs* a, const float* acts, const float* dL_dy, void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (const int rc = mlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!mlp_inputs_ok(a) || !required(acts, 16) || !required(dL_dy, 16) || !aligned(a->dx, 4) || !aligned(a->dcond, 4))
        return GS_E_BAD_ARG;
    if (a->dcond && a->dim_cond == 0) return GS_E_BAD_ARG;
    bool any = a->dx || a->dcond;
    for (int l = 0; l <= a->n_hidden; l++) {
        if (!aligned(a->dW[l], 4) || !aligned(a->db[l], 4)) return GS_E_BAD_ARG;
        any = any || a->dW[l] || a->db[l];
    }
    if (any) {
        if (!required(workspace, 16)) return GS_E_BAD_ARG;
        if (workspace_bytes < mlp_workspace_bytes(a, 1)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    if (!any) return GS_OK;
    return launch_mlp_backward(a, acts, dL_dy, workspace, (hipStream_t)stream);
}

}  // extern "C"
