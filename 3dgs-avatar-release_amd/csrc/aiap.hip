// aiap.hip -- the as-isometric-as-possible regularisers of the reference's training loop (utils/loss_utils.py:69-102,
// called at train.py:163-171 on every iteration, lambda_aiap_xyz = 1 and lambda_aiap_cov = 100 by default) as one
// forward launch, a stable reverse-adjacency build and one backward launch, instead of ~70 small torch operators whose
// index-backward scatter-adds are not deterministic.
//
// Spec (aiap_loss(x_canonical, x_deformed, n_neighbors = 5, nn_ix = None); this file reproduces it):
//   Inputs: xc, xd (N, D) fp32, D = 3 (positions) or 6 (strip_symmetric covariances, scene/gaussian_model.py:154);
//   idx (N, K) int64.  The torch form is cdist(x.unsqueeze(1), x[idx])[:, 0, 1:].
//   * Column 0 of idx is dropped, whatever it holds.  The pairs are (i, j = idx[i, k]) for k = 1 .. K-1, M = N (K-1).
//   * a_p = |xc_i - xc_j|_2, b_p = |xd_i - xd_j|_2, in fp32, as the sqrt of a sum of squared differences.
//   * L = (1 / M) sum_p |a_p - b_p|  (F.l1_loss, mean reduction).
//   * s_p = sign(a_p - b_p), 0 when they are equal; g = the upstream gradient scalar:
//       dL/dxc_i += g s_p / M (xc_i - xc_j) / a_p, dL/dxc_j -= the same (the term is 0 when a_p == 0, as torch's
//       _cdist_backward has it); dL/dxd_i -= g s_p / M (xd_i - xd_j) / b_p, dL/dxd_j += the same (0 when b_p == 0).
//   * Gradients reach all four tensors.  full_aiap_loss uses ONE idx (knn_points(xyz_can, K = n_neighbors): the point
//     itself and 4 neighbours) for both the position and the covariance loss: here both are one call (n_sets = 2).
//   The arithmetic is compiled with -ffp-contract=off (build.py STRICT): xd == xc bit for bit gives a_p == b_p exactly.
//
// Passes (forward):
//   aiap_fwd        one thread per source row: its K-1 pairs' |a - b| for every set, per-block partial sums (block_sum,
//                   waves pairwise: ordered_sum.h), per-block counts of idx values outside [0, N) (never
//                   dereferenced: such a pair adds nothing), and the (target, source) keys of the adjacency sort
//                   (target N for a bad index, so those sort last and fall outside every list).  It also clears the
//                   sort's digit totals, so the call needs no memset node.
//   radix sort      radix_sort.hip, stable LSD on the target: pairs of one target stay in (i, k) order.
//   aiap_offsets    start[t] = the first sorted pair whose target is >= t, t = 0 .. N (list_starts: sorted_lists.h);
//                   its last n_sets + 1 workgroups add the loss partials (in double, fixed order) and the bad counts.
// Backward: one thread per row writes every output row exactly once: its outgoing pairs, then its incoming pairs in
// adjacency order.  A row with more than AIAP_HEAVY incoming pairs (a hub) is taken over by its whole wave: lane l adds
// entries l, l + 64, ... and the DPP ladder adds the lanes.  No atomics anywhere: the same input gives the same bits.
// Rows are read with 4-byte loads (a D = 3 row is 12 bytes: any 4-byte-aligned base is accepted).
#include "common.h"
#include "boundary.h"
#include "ordered_sum.h"
#include "sorted_lists.h"

#define AIAP_THREADS 256
#define AIAP_HEAVY 64  // incoming pairs above which the wave takes a row over

static inline int aiap_blocks(int n) { return (n + AIAP_THREADS - 1) / AIAP_THREADS; }
static inline int aiap_bits(int N) {  // bits of a key in [0, N]
    int b = 1;
    while (b < 31 && ((uint32_t)N >> b) != 0u) b++;
    return b;
}

// workspace: misc u32[4] (word 0: bad index count) | partial f32[2][fwd blocks] | bad partial u32[fwd blocks] |
// the pair sort's buffers and tables for M pairs (PairSort) | start u32[N + 1]
struct AiapWs {
    uint32_t* misc;
    float* partial;
    uint32_t* badp;
    PairSort sort;
    uint32_t* start;
    size_t total;
};
static inline AiapWs aiap_carve(int N, int K, void* base) {
    const size_t M = (size_t)N * (size_t)(K - 1), nb = (size_t)aiap_blocks(N);
    Carver c(base);
    AiapWs w;
    w.misc = c.take<uint32_t>(4);
    w.partial = c.take<float>(2 * nb);
    w.badp = c.take<uint32_t>(nb);
    w.sort = PairSort::carve(c, M);
    w.start = c.take<uint32_t>((size_t)N + 1);
    w.total = c.o;
    return w;
}
static size_t aiap_workspace_bytes(int N, int K) { return aiap_carve(N, K, nullptr).total; }

struct AiapSet {
    const float* xc;
    const float* xd;
    float* gc;          // backward outputs (NULL: not wanted)
    float* gd;
    const float* grad;  // upstream scalar (NULL = 1)
    float* loss;        // forward output
};
static inline AiapSet aiap_set(const GsAiapSet* s) {
    if (!s) return AiapSet{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return AiapSet{s->xc, s->xd, s->dL_dxc, s->dL_dxd, s->dL_dloss, s->loss};
}

template <int D>
__device__ __forceinline__ void aiap_load(const float* __restrict__ x, uint32_t row, float* v) {
    const float* p = x + (size_t)row * D;
#pragma unroll
    for (int d = 0; d < D; d++) v[d] = p[d];
}
template <int D>
__device__ __forceinline__ float aiap_norm(const float* a, const float* b) {
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < D; d++) {
        const float t = a[d] - b[d];
        s += t * t;
    }
    return sqrtf(s);
}
__device__ __forceinline__ float aiap_sign(float a, float b) { return a > b ? 1.0f : (a < b ? -1.0f : 0.0f); }

// |a - b| of every pair of row i in one set
template <int D>
__device__ __forceinline__ float aiap_row_loss(const AiapSet& S, uint32_t i, const uint32_t* js, int nk) {
    if (D == 0) return 0.0f;
    float ci[D > 0 ? D : 1], di[D > 0 ? D : 1];
    aiap_load<D>(S.xc, i, ci);
    aiap_load<D>(S.xd, i, di);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 7; k++) {  // (constant indices: js stays in registers)
        if (k >= nk) break;
        const uint32_t j = js[k];
        if (j == 0xFFFFFFFFu) continue;
        float cj[D > 0 ? D : 1], dj[D > 0 ? D : 1];
        aiap_load<D>(S.xc, j, cj);
        aiap_load<D>(S.xd, j, dj);
        acc += fabsf(aiap_norm<D>(ci, cj) - aiap_norm<D>(di, dj));
    }
    return acc;
}

template <int D0, int D1>
__global__ __launch_bounds__(AIAP_THREADS) void aiap_fwd_kernel(int N, int K, const long long* __restrict__ idx, AiapSet s0,
                                                               AiapSet s1, AiapWs w, ZeroJob zj) {
    __shared__ float lds[2][AIAP_THREADS / WAVE];
    __shared__ uint32_t ldsb[AIAP_THREADS / WAVE];
    const uint32_t i = blockIdx.x * AIAP_THREADS + threadIdx.x;
    zero_job(zj);
    float l0 = 0.0f, l1 = 0.0f;
    uint32_t bad = 0;
    if (i < (uint32_t)N) {
        uint32_t js[7];
        const int nk = K - 1;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            if (k >= nk) break;
            const long long j = idx[(size_t)i * K + k + 1];
            const bool ok = j >= 0 && j < (long long)N;
            js[k] = ok ? (uint32_t)j : 0xFFFFFFFFu;
            bad += ok ? 0u : 1u;
            const size_t p = (size_t)i * nk + k;
            w.sort.k0[p] = ok ? (uint32_t)j : (uint32_t)N;  // (a bad index: key N, behind every list)
            w.sort.v0[p] = i;
        }
        l0 = aiap_row_loss<D0>(s0, i, js, nk);
        l1 = aiap_row_loss<D1>(s1, i, js, nk);
    }
    const float t0 = block_sum<AIAP_THREADS, WavesPairwise>(l0, lds[0]);
    const float t1 = D1 ? block_sum<AIAP_THREADS, WavesPairwise>(l1, lds[1]) : 0.0f;
    const uint32_t wb = wave_sum(bad);
    if ((threadIdx.x & (WAVE - 1)) == 0) ldsb[threadIdx.x / WAVE] = wb;
    __syncthreads();
    if (threadIdx.x == 0) {
        w.partial[blockIdx.x] = t0;
        w.partial[gridDim.x + blockIdx.x] = t1;
        w.badp[blockIdx.x] = (ldsb[0] + ldsb[1]) + (ldsb[2] + ldsb[3]);
    }
}

// start[t], t = 0 .. N, from the sorted targets; the last workgroups: losses and the bad count
__global__ __launch_bounds__(AIAP_THREADS) void aiap_offsets_kernel(int N, long long M, const uint32_t* __restrict__ ks,
                                                                   uint32_t* __restrict__ start, int nb_off, int nb_fwd,
                                                                   int n_sets, const float* __restrict__ partial,
                                                                   const uint32_t* __restrict__ badp, uint32_t* misc,
                                                                   float* loss0, float* loss1) {
    if ((int)blockIdx.x >= nb_off) {
        // loss of set `s` (or, past them, the bad-index count): thread t adds partials t, t + 256, ... in order (double)
        __shared__ double ld[AIAP_THREADS];
        const int s = blockIdx.x - nb_off;
        double acc = 0.0;
        for (int b = threadIdx.x; b < nb_fwd; b += AIAP_THREADS)
            acc += s < n_sets ? (double)partial[(size_t)s * nb_fwd + b] : (double)badp[b];
        ld[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int k = 0; k < AIAP_THREADS; k++) t += ld[k];
            if (s < n_sets) {
                float* out = s == 0 ? loss0 : loss1;
                out[0] = (float)(t / (double)M);
            } else {
                misc[0] = (uint32_t)t;
            }
        }
        return;
    }
    // (the keys are targets in [0, N] -- aiap_fwd stores a bad index as N -- so no list start needs clamping to N)
    list_starts(ks, M, (uint32_t)N, (long long)blockIdx.x * AIAP_THREADS + threadIdx.x, start);
}

static int launch_aiap_forward(int N, int K, const long long* idx, int n_sets, const GsAiapSet* sets, void* workspace, hipStream_t s) {
    const AiapWs w = aiap_carve(N, K, workspace);
    const long long M = (long long)N * (K - 1);
    const int bits = aiap_bits(N), nb = aiap_blocks(N);
    const ZeroJob zj = w.sort.totals_job(M, bits);
    const AiapSet s0 = aiap_set(&sets[0]), s1 = aiap_set(n_sets > 1 ? &sets[1] : nullptr);
    StageScope st("aiap_fwd", s);
#define AIAP_FWD(A, B) hipLaunchKernelGGL((aiap_fwd_kernel<A, B>), dim3(nb), dim3(AIAP_THREADS), 0, s, N, K, idx, s0, s1, w, zj)
    const int d0 = sets[0].D, d1 = n_sets > 1 ? sets[1].D : 0;
    if (d0 == 3 && d1 == 0) AIAP_FWD(3, 0);
    else if (d0 == 6 && d1 == 0) AIAP_FWD(6, 0);
    else if (d0 == 3 && d1 == 3) AIAP_FWD(3, 3);
    else if (d0 == 3 && d1 == 6) AIAP_FWD(3, 6);
    else if (d0 == 6 && d1 == 3) AIAP_FWD(6, 3);
    else AIAP_FWD(6, 6);
#undef AIAP_FWD
    GS_LAUNCH_CHECK("aiap_fwd", 0, s);
    const int rc = w.sort.sort(M, bits, s);
    if (rc != GS_OK) return rc;
    const uint32_t* ks = w.sort.sorted_keys(bits);
    const int nb_off = (int)((M + 1 + AIAP_THREADS - 1) / AIAP_THREADS);
    hipLaunchKernelGGL(aiap_offsets_kernel, dim3(nb_off + n_sets + 1), dim3(AIAP_THREADS), 0, s, N, M, ks, w.start, nb_off, nb,
                       n_sets, w.partial, w.badp, w.misc, s0.loss, s1.loss);
    GS_LAUNCH_CHECK("aiap_offsets", 0, s);
    return GS_OK;
}

// ---- backward
template <int D>
struct AiapAcc {
    float c[D > 0 ? D : 1], d[D > 0 ? D : 1];
};

// pair (r, o) seen from row r, whichever end of the pair r is (d|x_r - x_o| / dx_r = (x_r - x_o) / |x_r - x_o| either
// way): adds s / a (xc_r - xc_o) to c and -s / b (xd_r - xd_o) to d (the common factor g / M is applied at the end)
template <int D>
__device__ __forceinline__ void aiap_pair(const AiapSet& S, const float cr[], const float dr[], uint32_t o,
                                          AiapAcc<D>& acc) {
    if (D == 0) return;
    float co[D > 0 ? D : 1], dd[D > 0 ? D : 1];
    aiap_load<D>(S.xc, o, co);
    aiap_load<D>(S.xd, o, dd);
    const float a = aiap_norm<D>(cr, co), b = aiap_norm<D>(dr, dd);
    const float sg = aiap_sign(a, b);
    const float wa = a > 0.0f ? sg / a : 0.0f, wb = b > 0.0f ? sg / b : 0.0f;
#pragma unroll
    for (int k = 0; k < D; k++) {
        acc.c[k] += wa * (cr[k] - co[k]);
        acc.d[k] -= wb * (dr[k] - dd[k]);
    }
}

template <int D>
__device__ __forceinline__ void aiap_zero(AiapAcc<D>& a) {
#pragma unroll
    for (int k = 0; k < (D > 0 ? D : 1); k++) a.c[k] = a.d[k] = 0.0f;
}

template <int D0, int D1>
__global__ __launch_bounds__(AIAP_THREADS) void aiap_bwd_kernel(int N, int K, const long long* __restrict__ idx,
                                                               const uint32_t* __restrict__ start,
                                                               const uint32_t* __restrict__ src, float inv_m, AiapSet s0,
                                                               AiapSet s1) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t r = blockIdx.x * AIAP_THREADS + threadIdx.x;
    const bool valid = r < (uint32_t)N;
    const uint32_t rr = valid ? r : 0u;
    float c0[D0 > 0 ? D0 : 1], d0[D0 > 0 ? D0 : 1], c1[D1 > 0 ? D1 : 1], d1[D1 > 0 ? D1 : 1];
    if (D0) { aiap_load<D0>(s0.xc, rr, c0); aiap_load<D0>(s0.xd, rr, d0); }
    if (D1) { aiap_load<D1>(s1.xc, rr, c1); aiap_load<D1>(s1.xd, rr, d1); }
    AiapAcc<D0> A0;
    AiapAcc<D1> A1;
    aiap_zero(A0);
    aiap_zero(A1);
    uint32_t beg = 0, end = 0;
    if (valid) {
        for (int k = 1; k < K; k++) {  // outgoing pairs, in k order
            const long long j = idx[(size_t)r * K + k];
            if (j < 0 || j >= (long long)N) continue;
            aiap_pair<D0>(s0, c0, d0, (uint32_t)j, A0);
            aiap_pair<D1>(s1, c1, d1, (uint32_t)j, A1);
        }
        beg = start[r];
        end = start[r + 1];
    }
    const bool heavy = end - beg > AIAP_HEAVY;
    if (!heavy)
        for (uint32_t e = beg; e < end; e++) {  // incoming pairs, in adjacency order
            const uint32_t i = src[e];
            aiap_pair<D0>(s0, c0, d0, i, A0);
            aiap_pair<D1>(s1, c1, d1, i, A1);
        }
    unsigned long long bal = __ballot(heavy);
    while (bal) {  // (wave-uniform) a hub row: the wave adds its incoming pairs, lane l taking entries l, l + 64, ...
        const int L = __ffsll((long long)bal) - 1;
        bal &= bal - 1;
        const uint32_t hr = (uint32_t)__shfl((int)r, L), hb = (uint32_t)__shfl((int)beg, L), he = (uint32_t)__shfl((int)end, L);
        float hc0[D0 > 0 ? D0 : 1], hd0[D0 > 0 ? D0 : 1], hc1[D1 > 0 ? D1 : 1], hd1[D1 > 0 ? D1 : 1];
        if (D0) { aiap_load<D0>(s0.xc, hr, hc0); aiap_load<D0>(s0.xd, hr, hd0); }
        if (D1) { aiap_load<D1>(s1.xc, hr, hc1); aiap_load<D1>(s1.xd, hr, hd1); }
        AiapAcc<D0> H0;
        AiapAcc<D1> H1;
        aiap_zero(H0);
        aiap_zero(H1);
        for (uint32_t e = hb + lane; e < he; e += WAVE) {
            const uint32_t i = src[e];
            aiap_pair<D0>(s0, hc0, hd0, i, H0);
            aiap_pair<D1>(s1, hc1, hd1, i, H1);
        }
#pragma unroll
        for (int k = 0; k < D0; k++) {
            const float c = wave_sum(H0.c[k]), d = wave_sum(H0.d[k]);
            if (lane == L) { A0.c[k] += c; A0.d[k] += d; }
        }
#pragma unroll
        for (int k = 0; k < D1; k++) {
            const float c = wave_sum(H1.c[k]), d = wave_sum(H1.d[k]);
            if (lane == L) { A1.c[k] += c; A1.d[k] += d; }
        }
    }
    if (!valid) return;
    if (D0) {
        const float g = (s0.grad ? s0.grad[0] : 1.0f) * inv_m;
#pragma unroll
        for (int k = 0; k < D0; k++) {
            if (s0.gc) s0.gc[(size_t)r * D0 + k] = g * A0.c[k];
            if (s0.gd) s0.gd[(size_t)r * D0 + k] = g * A0.d[k];
        }
    }
    if (D1) {
        const float g = (s1.grad ? s1.grad[0] : 1.0f) * inv_m;
#pragma unroll
        for (int k = 0; k < D1; k++) {
            if (s1.gc) s1.gc[(size_t)r * D1 + k] = g * A1.c[k];
            if (s1.gd) s1.gd[(size_t)r * D1 + k] = g * A1.d[k];
        }
    }
}

static int launch_aiap_backward(int N, int K, const long long* idx, int n_sets, const GsAiapSet* sets, const void* workspace,
                                hipStream_t s) {
    const AiapWs w = aiap_carve(N, K, const_cast<void*>(workspace));
    const long long M = (long long)N * (K - 1);
    const uint32_t* src = w.sort.sorted_vals(aiap_bits(N));
    const float inv_m = (float)(1.0 / (double)M);
    const AiapSet s0 = aiap_set(&sets[0]), s1 = aiap_set(n_sets > 1 ? &sets[1] : nullptr);
    const int nb = aiap_blocks(N);
    StageScope st("aiap_bwd", s);
#define AIAP_BWD(A, B) \
    hipLaunchKernelGGL((aiap_bwd_kernel<A, B>), dim3(nb), dim3(AIAP_THREADS), 0, s, N, K, idx, w.start, src, inv_m, s0, s1)
    const int d0 = sets[0].D, d1 = n_sets > 1 ? sets[1].D : 0;
    if (d0 == 3 && d1 == 0) AIAP_BWD(3, 0);
    else if (d0 == 6 && d1 == 0) AIAP_BWD(6, 0);
    else if (d0 == 3 && d1 == 3) AIAP_BWD(3, 3);
    else if (d0 == 3 && d1 == 6) AIAP_BWD(3, 6);
    else if (d0 == 6 && d1 == 3) AIAP_BWD(6, 3);
    else AIAP_BWD(6, 6);
#undef AIAP_BWD
    GS_LAUNCH_CHECK("aiap_bwd", 0, s);
    return GS_OK;
}

extern "C" {

// M = N (K - 1) pairs stay below 2^31 (the sort and the adjacency index 32-bit words)
static bool aiap_shape_ok(int32_t N, int32_t K, int32_t n_sets) {
    return N >= 1 && K >= 2 && K <= 8 && (n_sets == 1 || n_sets == 2) && (int64_t)N * (K - 1) < ((int64_t)1 << 31);
}
static bool aiap_sets_ok(int32_t n_sets, const GsAiapSet* sets, bool forward) {
    if (!sets) return false;
    for (int k = 0; k < n_sets; k++) {
        const GsAiapSet& s = sets[k];
        if ((s.D != 3 && s.D != 6) || !s.xc || !s.xd || (forward && !s.loss)) return false;
    }
    return true;
}
int gs_aiap_workspace_bytes(int32_t N, int32_t K, int32_t n_sets, size_t* out) {
    if (!out || !aiap_shape_ok(N, K, n_sets)) return GS_E_BAD_ARG;
    *out = aiap_workspace_bytes(N, K);
    return GS_OK;
}
int gs_aiap_forward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets, void* workspace,
                    size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!aiap_shape_ok(N, K, n_sets) || !idx || !workspace || !aiap_sets_ok(n_sets, sets, true)) return GS_E_BAD_ARG;
    if (workspace_bytes < aiap_workspace_bytes(N, K)) return GS_E_WORKSPACE;
    return launch_aiap_forward(N, K, (const long long*)idx, n_sets, sets, workspace, (hipStream_t)stream);
}
int gs_aiap_backward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets,
                     const void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!aiap_shape_ok(N, K, n_sets) || !idx || !workspace || !aiap_sets_ok(n_sets, sets, false)) return GS_E_BAD_ARG;
    if (workspace_bytes < aiap_workspace_bytes(N, K)) return GS_E_WORKSPACE;
    return launch_aiap_backward(N, K, (const long long*)idx, n_sets, sets, workspace, (hipStream_t)stream);
}

}  // extern "C"
