// hashgrid.hip -- the multiresolution hash-grid encoding of the reference's non-rigid deformer (models/network_utils.py:329-
// 343, tcnn.Encoding(3, config) under HashGridwithMLP.forward, models/deformer/non_rigid.py:226-300; every training step
// after iteration 3000 with the default configs/non_rigid/hashgrid.yaml): a forward launch, a gather-only input gradient
// and a parameter gradient that sums every table entry's contributions in a fixed order (no float atomics).
//
// Spec.  There is no tiny-cuda-nn source to check against: the rules below restate upstream GridEncoding from memory.
// This restatement and the tests pin them, not tcnn.
//   Configuration: n_levels L (16), n_features_per_level F (2), log2_hashmap_size T (19), base_resolution N0 (16),
//   per_level_scale b (2.0), interpolation "Linear", hash "CoherentPrime"; 3-D input; F in {1, 2, 4, 8}.
//   Level table, computed once on the host in float32 as tcnn's host code does:
//   * log2b = (float)log2((double)b)
//   * scale_l = exp2f(l * log2b) * N0 - 1
//   * res_l = (uint32)ceilf(scale_l) + 1
//   * dense_l = res_l^3 rounded up to a multiple of 8 (capped at 2^31-1 before the rounding, if the float cube exceeds it)
//   * size_l = min(dense_l, 2^T)
//   * offset_0 = 0, offset_{l+1} = offset_l + size_l, n_params = offset_L * F
//   The device never recomputes scale_l: the host passes the float32 values to the kernels, so the kernels and the
//   restatement make the same integer decisions.
//   Forward, per point i and level l.  Inputs are not clamped:
//   * For each dim d: pos_d = fmaf(scale_l, x_d, 0.5f), c_d = (uint32)(int32)floorf(pos_d), t_d = pos_d - floorf(pos_d).
//   * Corner k = 0..7: v_d = c_d + bit_d(k) (uint32, wrapping).  The weight is w_k = prod_d (bit_d(k) ? t_d : 1 - t_d).
//   * Corner index, in uint32 arithmetic throughout:
//     * Start with stride = 1, idx = 0.
//     * For d = 0, 1, 2, and only while stride <= size_l: idx += v_d * stride, then stride *= res_l.
//     * If size_l < stride at the end, replace idx with the hash idx = (v_0 * 1) ^ (v_1 * 2654435761) ^ (v_2 * 805459861).
//     * entry = idx % size_l.
//   * So x = 1.0 on a dense level wraps through the modulo, and a negative x wraps through the int -> uint32 cast.  Any
//     finite input reads inside the table.
//   * out[i, l*F + f] = sum_k w_k theta[(offset_l + entry_k)*F + f].  The output is (N, L*F), row-major.
//   Backward, given G = dL/dout:
//   * dL/dtheta[(offset_l + e)*F + f] = sum over (i, k) with entry_k(i, l) = e of w_k G[i, l*F + f].
//   * dL/dx_d[i] = sum_l scale_l sum_f G[i, l*F+f] d(trilinear form)/dt_d.  This is the one-sided derivative of the
//     cell that floorf picked.
//   * No second derivatives.
// Arithmetic: fp32 throughout, compiled with -ffp-contract=off (build.py STRICT); the one fused multiply-add is the
// explicit fmaf of pos_d.  Sums run in k order (forward), level order (input gradient) and list order (parameters).
//
// Passes.  Forward: hg_fwd, one thread per (point, level), t = i L + l: the thread's F outputs are one store.
// Backward:
//   hg_points       one thread per point: for every level its cell; the input gradient row (re-reading the 8 corners of
//                   every level, written once), and the (key = offset_l + entry_k, value = 8 i + k) pair of every corner at
//                   position (l N + i) 8 + k.  It also clears the sort's digit totals (no memset node).
//   radix sort      radix_sort.hip, stable LSD on the key bits: the pairs of one entry stay in (l, i, k) order.
//   hg_starts       start[e], e = 0 .. n_entries, the first sorted pair whose key is >= e (list_starts: sorted_lists.h).
//   hg_chunks       a wave per chunk of HG_CHUNK sorted pairs: for the (at most two) lists longer than HG_CHUNK that
//                   reach into the chunk, the sum of their pairs inside it (lane-strided, then the DPP ladder).
//   hg_entries      one thread per entry writes its F gradient words once (an empty list writes 0): up to HG_HEAVY
//                   pairs the thread adds them in list order; up to HG_CHUNK the wave takes the list over (lane l: pairs
//                   l, l + 64, ..., then the ladder); longer lists add their chunk partials in chunk order, the same way.
// Every order is fixed: the same input gives the same bits, run after run and under graph replay.
#include "common.h"
#include "boundary.h"
#include "ordered_sum.h"
#include "sorted_lists.h"

#define HG_THREADS 256
#ifndef HG_HEAVY
#define HG_HEAVY 32    // pairs of a list above which its wave takes it over
#endif
#ifndef HG_CHUNK
#define HG_CHUNK 1024  // pairs per chunk: lists longer than this are summed from chunk partials
#endif

// ---- the level table (host), passed to the kernels by value; hashgrid_table is the one source of the integer decisions
struct HgTable {
    int L, F;
    float scale[GS_HASHGRID_MAX_LEVELS];
    uint32_t res[GS_HASHGRID_MAX_LEVELS], size[GS_HASHGRID_MAX_LEVELS], off[GS_HASHGRID_MAX_LEVELS + 1];
};
static int hashgrid_table(const GsHashGrid* g, HgTable* t) {
    const int L = g->n_levels, F = g->n_features_per_level, T = g->log2_hashmap_size, N0 = g->base_resolution;
    const float b = g->per_level_scale;
    if (L < 1 || L > GS_HASHGRID_MAX_LEVELS || !(F == 1 || F == 2 || F == 4 || F == 8) || T < 1 || T > 30 || N0 < 1 ||
        !(b >= 1.0f) || !(b <= 1.0e4f))
        return GS_E_BAD_ARG;
    const float log2b = (float)log2((double)b);
    uint64_t off = 0;
    t->L = L;
    t->F = F;
    for (int l = 0; l < L; l++) {
        const float scale = exp2f((float)l * log2b) * (float)N0 - 1.0f;
        if (!(scale < 2147483520.0f)) return GS_E_TOO_LARGE;  // res_l must fit 32 bits
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        const float cube_f = powf((float)res, 3.0f);
        uint32_t dense = cube_f > (float)0x7FFFFFFF ? 0x7FFFFFFFu : res * res * res;
        dense = (dense + 7u) & ~7u;
        const uint32_t hashed = 1u << T;
        const uint32_t size = dense < hashed ? dense : hashed;
        t->scale[l] = scale;
        t->res[l] = res;
        t->size[l] = size;
        t->off[l] = (uint32_t)off;
        off += size;
        if (off * (uint64_t)F >= ((uint64_t)1 << 31)) return GS_E_TOO_LARGE;  // n_params indexes 32-bit words
    }
    t->off[L] = (uint32_t)off;
    return GS_OK;
}

static inline int hg_bits(uint32_t n) {  // bits of a key in [0, n)
    int b = 1;
    while (b < 32 && (n - 1u) >> b != 0u) b++;
    return b;
}

// workspace: the pair sort's buffers and tables for M = 8 L N pairs (PairSort) | start u32[n_entries + 1]
// | chunk partials f32[chunks][2][F]
struct HgWs {
    PairSort sort;
    uint32_t* start;
    float* part;
    size_t total;
};
static inline HgWs hg_carve(const HgTable& t, int N, void* base) {
    const size_t M = (size_t)8 * t.L * (size_t)N, nch = (M + HG_CHUNK - 1) / HG_CHUNK;
    Carver c(base);
    HgWs w;
    w.sort = PairSort::carve(c, M);
    w.start = c.take<uint32_t>((size_t)t.off[t.L] + 1);
    w.part = c.take<float>(nch * 2 * t.F);
    w.total = c.o;
    return w;
}
static size_t hashgrid_workspace_bytes(const HgTable& t, int N) { return hg_carve(t, N, nullptr).total; }

// ---- device helpers
template <int F>
__device__ __forceinline__ void hg_load(const float* __restrict__ p, float* v) {
    if (F == 1) {
        v[0] = p[0];
    } else if (F == 2) {
        const float2 a = *(const float2*)p;
        v[0] = a.x; v[1] = a.y;
    } else {
#pragma unroll
        for (int q = 0; q < F; q += 4) {
            const float4 a = *(const float4*)(p + q);
            v[q] = a.x; v[q + 1] = a.y; v[q + 2] = a.z; v[q + 3] = a.w;
        }
    }
}
template <int F>
__device__ __forceinline__ void hg_store(float* __restrict__ p, const float* v) {
    if (F == 1) {
        p[0] = v[0];
    } else if (F == 2) {
        *(float2*)p = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int q = 0; q < F; q += 4) *(float4*)(p + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
    }
}

struct HgCell {
    uint32_t c[3];
    float t[3];
};
__device__ __forceinline__ HgCell hg_cell(float scale, const float* x) {
    HgCell c;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float pos = fmaf(scale, x[d], 0.5f);
        const float fl = floorf(pos);
        c.c[d] = (uint32_t)(int32_t)fl;
        c.t[d] = pos - fl;
    }
    return c;
}
__device__ __forceinline__ float hg_weight(const HgCell& c, int k) {
    const float w0 = (k & 1) ? c.t[0] : 1.0f - c.t[0];
    const float w1 = (k & 2) ? c.t[1] : 1.0f - c.t[1];
    const float w2 = (k & 4) ? c.t[2] : 1.0f - c.t[2];
    return (w0 * w1) * w2;
}
__device__ __forceinline__ uint32_t hg_entry(const HgCell& c, int k, uint32_t res, uint32_t size) {
    const uint32_t v[3] = {c.c[0] + (uint32_t)(k & 1), c.c[1] + (uint32_t)((k >> 1) & 1), c.c[2] + (uint32_t)((k >> 2) & 1)};
    uint32_t stride = 1u, idx = 0u;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (stride > size) break;
        idx += v[d] * stride;
        stride *= res;
    }
    if (size < stride) idx = (v[0] * 1u) ^ (v[1] * 2654435761u) ^ (v[2] * 805459861u);
    return (size & (size - 1u)) == 0u ? (idx & (size - 1u)) : idx % size;
}
__device__ __forceinline__ void hg_x(const float* __restrict__ x, uint32_t i, float* v) {
    v[0] = x[(size_t)i * 3];
    v[1] = x[(size_t)i * 3 + 1];
    v[2] = x[(size_t)i * 3 + 2];
}
__device__ __forceinline__ int hg_level_of(const HgTable& t, uint32_t e) {
    int l = 0;
    for (int j = 1; j < t.L; j++) l += e >= t.off[j] ? 1 : 0;
    return l;
}

// ---- forward
template <int F>
__global__ __launch_bounds__(HG_THREADS) void hg_fwd_kernel(HgTable tab, int N, const float* __restrict__ x,
                                                            const float* __restrict__ theta, float* __restrict__ out) {
    const uint32_t t = blockIdx.x * HG_THREADS + threadIdx.x;  // (N L < 2^31: gs_hashgrid_forward)
    if (t >= (uint32_t)N * (uint32_t)tab.L) return;
    const uint32_t i = t / (uint32_t)tab.L;
    const int l = (int)(t - i * (uint32_t)tab.L);
    float xi[3];
    hg_x(x, i, xi);
    const HgCell c = hg_cell(tab.scale[l], xi);
    const uint32_t res = tab.res[l], size = tab.size[l], off = tab.off[l];
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float th[F];
        hg_load<F>(theta + (size_t)(off + hg_entry(c, k, res, size)) * F, th);
        const float w = hg_weight(c, k);
#pragma unroll
        for (int f = 0; f < F; f++) acc[f] += w * th[f];
    }
    hg_store<F>(out + (size_t)t * F, acc);
}

static int launch_hashgrid_forward(const HgTable& tab, int N, const float* x, const float* params, float* out, hipStream_t s) {
    const long long n = (long long)N * tab.L;
    const int nb = (int)((n + HG_THREADS - 1) / HG_THREADS);
    StageScope st("hashgrid_fwd", s);
#define HG_FWD(FF) hipLaunchKernelGGL(hg_fwd_kernel<FF>, dim3(nb), dim3(HG_THREADS), 0, s, tab, N, x, params, out)
    switch (tab.F) {
        case 1: HG_FWD(1); break;
        case 2: HG_FWD(2); break;
        case 4: HG_FWD(4); break;
        default: HG_FWD(8); break;
    }
#undef HG_FWD
    GS_LAUNCH_CHECK("hashgrid_fwd", 0, s);
    return GS_OK;
}

// ---- backward
// one thread per point: input gradient row (dx != NULL) and the sort pairs of every level (keys != NULL)
template <int F>
__global__ __launch_bounds__(HG_THREADS) void hg_points_kernel(HgTable tab, int N, const float* __restrict__ x,
                                                               const float* __restrict__ theta, const float* __restrict__ G,
                                                               float* __restrict__ dx, uint32_t* __restrict__ keys,
                                                               uint32_t* __restrict__ vals, ZeroJob zj) {
    zero_job(zj);
    const uint32_t i = blockIdx.x * HG_THREADS + threadIdx.x;
    if (i >= (uint32_t)N) return;
    float xi[3];
    hg_x(x, i, xi);
    float gx[3] = {0.0f, 0.0f, 0.0f};
    const int LF = tab.L * F;
    for (int l = 0; l < tab.L; l++) {
        const HgCell c = hg_cell(tab.scale[l], xi);
        const uint32_t res = tab.res[l], size = tab.size[l], off = tab.off[l];
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) e[k] = hg_entry(c, k, res, size);
        if (keys) {
            const size_t p = ((size_t)l * N + i) * 8;
            uint4* kp = (uint4*)(keys + p);
            uint4* vp = (uint4*)(vals + p);
            kp[0] = make_uint4(off + e[0], off + e[1], off + e[2], off + e[3]);
            kp[1] = make_uint4(off + e[4], off + e[5], off + e[6], off + e[7]);
            vp[0] = make_uint4(8 * i, 8 * i + 1, 8 * i + 2, 8 * i + 3);
            vp[1] = make_uint4(8 * i + 4, 8 * i + 5, 8 * i + 6, 8 * i + 7);
        }
        if (dx) {
            float g[F];
            hg_load<F>(G + (size_t)i * LF + l * F, g);
            // d(trilinear form)/dt_d = sum_k (bit_d(k) ? 1 : -1) (product of the other two factors) sum_f g_f theta_k,f
            float dt[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                float th[F];
                hg_load<F>(theta + (size_t)(off + e[k]) * F, th);
                float sk = 0.0f;
#pragma unroll
                for (int f = 0; f < F; f++) sk += g[f] * th[f];
                const float w0 = (k & 1) ? c.t[0] : 1.0f - c.t[0];
                const float w1 = (k & 2) ? c.t[1] : 1.0f - c.t[1];
                const float w2 = (k & 4) ? c.t[2] : 1.0f - c.t[2];
                const float s0 = (k & 1) ? sk : -sk, s1 = (k & 2) ? sk : -sk, s2 = (k & 4) ? sk : -sk;
                dt[0] += (w1 * w2) * s0;
                dt[1] += (w0 * w2) * s1;
                dt[2] += (w0 * w1) * s2;
            }
            const float sc = tab.scale[l];
#pragma unroll
            for (int d = 0; d < 3; d++) gx[d] += sc * dt[d];
        }
    }
    if (dx) {
        dx[(size_t)i * 3] = gx[0];
        dx[(size_t)i * 3 + 1] = gx[1];
        dx[(size_t)i * 3 + 2] = gx[2];
    }
}

// start[e], e = 0 .. n_entries, from the sorted keys: list_starts (sorted_lists.h), one thread per pair
__global__ __launch_bounds__(HG_THREADS) void hg_starts_kernel(uint32_t n_entries, long long M, const uint32_t* __restrict__ ks,
                                                               uint32_t* __restrict__ start) {
    list_starts(ks, M, n_entries, (long long)blockIdx.x * HG_THREADS + threadIdx.x, start);
}

// lane-strided sum of the contributions of sorted pairs [a, b) to an entry of level l, then the DPP ladder (wave-uniform
// arguments; every lane gets the total)
template <int F>
__device__ __forceinline__ void hg_wave_list(const HgTable& tab, int N, int l, uint32_t a, uint32_t b,
                                             const uint32_t* __restrict__ src, const float* __restrict__ x,
                                             const float* __restrict__ G, float* acc) {
    const int lane = threadIdx.x & (WAVE - 1);
    const float sc = tab.scale[l];
    const int LF = tab.L * F;
    float s[F];
#pragma unroll
    for (int f = 0; f < F; f++) s[f] = 0.0f;
    for (uint32_t p = a + lane; p < b; p += WAVE) {
        const uint32_t v = src[p], i = v >> 3;
        float xi[3], g[F];
        hg_x(x, i, xi);
        hg_load<F>(G + (size_t)i * LF + l * F, g);
        const float w = hg_weight(hg_cell(sc, xi), (int)(v & 7u));
#pragma unroll
        for (int f = 0; f < F; f++) s[f] += w * g[f];
    }
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = wave_sum(s[f]);
}

// a wave per chunk of HG_CHUNK sorted pairs: partial sums of the long lists reaching into it (slot 0: the list at the
// chunk's first pair, slot 1: the list at its last pair, when that is another one)
template <int F>
__global__ __launch_bounds__(HG_THREADS) void hg_chunks_kernel(HgTable tab, int N, long long M, const uint32_t* __restrict__ ks,
                                                               const uint32_t* __restrict__ src,
                                                               const uint32_t* __restrict__ start, const float* __restrict__ x,
                                                               const float* __restrict__ G, float* __restrict__ part) {
    const long long c = ((long long)blockIdx.x * HG_THREADS + threadIdx.x) / WAVE;
    const long long p0 = c * HG_CHUNK;
    if (p0 >= M) return;  // (wave-uniform)
    const uint32_t p1 = (uint32_t)(p0 + HG_CHUNK < M ? p0 + HG_CHUNK : M);
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t e0 = ks[p0], e1 = ks[p1 - 1];
    const uint32_t s0 = start[e0], t0 = start[e0 + 1];
    float acc[F];
    if (t0 - s0 > HG_CHUNK) {
        hg_wave_list<F>(tab, N, hg_level_of(tab, e0), (uint32_t)p0, t0 < p1 ? t0 : p1, src, x, G, acc);
        if (lane == 0) hg_store<F>(part + (size_t)c * 2 * F, acc);
    }
    if (e1 != e0) {
        const uint32_t s1 = start[e1], t1 = start[e1 + 1];
        if (t1 - s1 > HG_CHUNK) {
            hg_wave_list<F>(tab, N, hg_level_of(tab, e1), s1, p1, src, x, G, acc);
            if (lane == 0) hg_store<F>(part + ((size_t)c * 2 + 1) * F, acc);
        }
    }
}

// one thread per entry: dL/dtheta of its F features, written once
template <int F>
__global__ __launch_bounds__(HG_THREADS) void hg_entries_kernel(HgTable tab, int N, const uint32_t* __restrict__ src,
                                                                const uint32_t* __restrict__ start, const float* __restrict__ x,
                                                                const float* __restrict__ G, const float* __restrict__ part,
                                                                float* __restrict__ dtheta) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t n_entries = tab.off[tab.L];
    const uint32_t e = blockIdx.x * HG_THREADS + threadIdx.x;
    const bool valid = e < n_entries;
    uint32_t beg = 0, end = 0;
    int l = 0;
    if (valid) {
        beg = start[e];
        end = start[e + 1];
        l = hg_level_of(tab, e);
    }
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = 0.0f;
    const bool heavy = end - beg > HG_HEAVY;
    if (!heavy) {
        const float sc = tab.scale[l];
        const int LF = tab.L * F;
        for (uint32_t p = beg; p < end; p++) {  // in list order
            const uint32_t v = src[p], i = v >> 3;
            float xi[3], g[F];
            hg_x(x, i, xi);
            hg_load<F>(G + (size_t)i * LF + l * F, g);
            const float w = hg_weight(hg_cell(sc, xi), (int)(v & 7u));
#pragma unroll
            for (int f = 0; f < F; f++) acc[f] += w * g[f];
        }
    }
    unsigned long long bal = __ballot(heavy);
    while (bal) {  // (wave-uniform) a long list: the wave sums it, or its chunk partials
        const int H = __ffsll((long long)bal) - 1;
        bal &= bal - 1;
        const uint32_t hb = (uint32_t)__shfl((int)beg, H), he = (uint32_t)__shfl((int)end, H);
        const int hl = __shfl(l, H);
        float h[F];
        if (he - hb <= HG_CHUNK) {
            hg_wave_list<F>(tab, N, hl, hb, he, src, x, G, h);
        } else {
            // chunks c0 .. c1 in chunk order: slot 0 where the list covers the chunk's first pair, else slot 1
            const uint32_t c0 = hb / HG_CHUNK, c1 = (he - 1) / HG_CHUNK;
            float s[F];
#pragma unroll
            for (int f = 0; f < F; f++) s[f] = 0.0f;
            for (uint32_t cc = c0 + lane; cc <= c1; cc += WAVE) {
                float pp[F];
                const uint32_t slot = hb <= cc * HG_CHUNK ? 0u : 1u;
                hg_load<F>(part + ((size_t)cc * 2 + slot) * F, pp);
#pragma unroll
                for (int f = 0; f < F; f++) s[f] += pp[f];
            }
#pragma unroll
            for (int f = 0; f < F; f++) h[f] = wave_sum(s[f]);
        }
        if (lane == H) {
#pragma unroll
            for (int f = 0; f < F; f++) acc[f] = h[f];
        }
    }
    if (valid) hg_store<F>(dtheta + (size_t)e * F, acc);
}

template <int F>
static int hg_backward(const HgTable& tab, int N, const float* x, const float* params, const float* dL_dout, float* dL_dx,
                       float* dL_dparams, void* workspace, hipStream_t s) {
    const HgWs w = hg_carve(tab, N, workspace);
    const long long M = 8ll * tab.L * N;
    const uint32_t n_entries = tab.off[tab.L];
    const int bits = hg_bits(n_entries);
    ZeroJob zj{nullptr, 0};
    if (dL_dparams) zj = w.sort.totals_job(M, bits);
    const int nb = N > 0 ? (N + HG_THREADS - 1) / HG_THREADS : 1;
    {
        StageScope st("hashgrid_points", s);
        hipLaunchKernelGGL(hg_points_kernel<F>, dim3(nb), dim3(HG_THREADS), 0, s, tab, N, x, params, dL_dout, dL_dx,
                           dL_dparams ? w.sort.k0 : nullptr, w.sort.v0, zj);
        GS_LAUNCH_CHECK("hashgrid_points", 0, s);
    }
    if (!dL_dparams) return GS_OK;
    {
        StageScope st("hashgrid_sort", s);
        const int rc = w.sort.sort(M, bits, s);
        if (rc != GS_OK) return rc;
    }
    const uint32_t* ks = w.sort.sorted_keys(bits);
    const uint32_t* src = w.sort.sorted_vals(bits);
    StageScope st("hashgrid_sum", s);
    const int nb_st = (int)((M + 1 + HG_THREADS - 1) / HG_THREADS);
    hipLaunchKernelGGL(hg_starts_kernel, dim3(nb_st), dim3(HG_THREADS), 0, s, n_entries, M, ks, w.start);
    GS_LAUNCH_CHECK("hashgrid_starts", 0, s);
    const long long nch = (M + HG_CHUNK - 1) / HG_CHUNK;
    if (nch > 0) {
        const int nb_ch = (int)((nch * WAVE + HG_THREADS - 1) / HG_THREADS);
        hipLaunchKernelGGL(hg_chunks_kernel<F>, dim3(nb_ch), dim3(HG_THREADS), 0, s, tab, N, M, ks, src, w.start, x, dL_dout,
                           w.part);
        GS_LAUNCH_CHECK("hashgrid_chunks", 0, s);
    }
    const int nb_e = (int)((n_entries + HG_THREADS - 1) / HG_THREADS);
    hipLaunchKernelGGL(hg_entries_kernel<F>, dim3(nb_e), dim3(HG_THREADS), 0, s, tab, N, src, w.start, x, dL_dout, w.part,
                       dL_dparams);
    GS_LAUNCH_CHECK("hashgrid_entries", 0, s);
    return GS_OK;
}

static int launch_hashgrid_backward(const HgTable& tab, int N, const float* x, const float* params, const float* dL_dout,
                                    float* dL_dx, float* dL_dparams, void* workspace, hipStream_t s) {
    switch (tab.F) {
        case 1: return hg_backward<1>(tab, N, x, params, dL_dout, dL_dx, dL_dparams, workspace, s);
        case 2: return hg_backward<2>(tab, N, x, params, dL_dout, dL_dx, dL_dparams, workspace, s);
        case 4: return hg_backward<4>(tab, N, x, params, dL_dout, dL_dx, dL_dparams, workspace, s);
        default: return hg_backward<8>(tab, N, x, params, dL_dout, dL_dx, dL_dparams, workspace, s);
    }
}

extern "C" {

int gs_hashgrid_levels(const GsHashGrid* grid, int32_t* offsets, float* scales, int32_t* resolutions, int32_t* n_params) {
    if (!grid) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    for (int l = 0; l <= t.L; l++) {
        if (offsets) offsets[l] = (int32_t)t.off[l];
        if (l == t.L) break;
        if (scales) scales[l] = t.scale[l];
        if (resolutions) resolutions[l] = (int32_t)t.res[l];
    }
    if (n_params) *n_params = (int32_t)(t.off[t.L] * (uint32_t)t.F);
    return GS_OK;
}
// the sort numbers the 8 L N (point, level, corner) pairs with 32-bit words
static bool hg_pairs_fit(const HgTable& t, int32_t N) { return (int64_t)8 * t.L * N < ((int64_t)1 << 31); }
int gs_hashgrid_workspace_bytes(const GsHashGrid* grid, int32_t N, size_t* out) {
    if (!grid || !out || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if (!hg_pairs_fit(t, N)) return GS_E_TOO_LARGE;
    *out = hashgrid_workspace_bytes(t, N);
    return GS_OK;
}
int gs_hashgrid_forward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, float* out, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!grid || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if ((int64_t)N * t.L >= ((int64_t)1 << 31)) return GS_E_TOO_LARGE;
    if (N == 0 || !out) return GS_OK;
    const size_t row = (size_t)4 * (t.F < 4 ? t.F : 4);  // a row of F features is read with loads of up to 16 bytes
    if (!x || !params || !aligned(params, row) || !aligned(out, row) || !aligned(x, 4)) return GS_E_BAD_ARG;
    return launch_hashgrid_forward(t, N, x, params, out, (hipStream_t)stream);
}
int gs_hashgrid_backward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, const float* dL_dout,
                         float* dL_dx, float* dL_dparams, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!grid || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if (dL_dparams && !hg_pairs_fit(t, N)) return GS_E_TOO_LARGE;
    if (!dL_dparams && (N == 0 || !dL_dx)) return GS_OK;
    if (N > 0 && (!x || !dL_dout || (dL_dx && !params))) return GS_E_BAD_ARG;
    const size_t row = (size_t)4 * (t.F < 4 ? t.F : 4);
    if (!aligned(params, row) || !aligned(dL_dout, row) || !aligned(dL_dparams, row) || !aligned(x, 4) || !aligned(dL_dx, 4))
        return GS_E_BAD_ARG;
    if (dL_dparams) {
        if (!workspace) return GS_E_BAD_ARG;
        if (workspace_bytes < hashgrid_workspace_bytes(t, N)) return GS_E_WORKSPACE;
    }
    return launch_hashgrid_backward(t, N, x, params, dL_dout, N > 0 ? dL_dx : nullptr, dL_dparams, workspace,
                                    (hipStream_t)stream);
}

}  // extern "C"
