// densify.hip -- the reference's densification cycle (scene/gaussian_model.py:263-266, 311-462; called from
// train.py:217-227 every 100 iterations up to 45 000, reset_opacity every 3 000) as three streaming passes and one
// gather, instead of ~40 small torch kernels with a nonzero() host sync per boolean-mask index.
//
// Spec (what GaussianModel.densify_and_prune / prune_points / reset_opacity compute; this file reproduces it):
//   Inputs, raw parameters: xyz [N,3], f_dc [N,1,3], f_rest [N,K,3], opacity [N,1] (logit), scaling [N,3] (log),
//   rotation [N,4] (w,x,y,z, not normalised); each one's Adam exp_avg / exp_avg_sq; the statistics
//   xyz_gradient_accum [N,1], denom [N,1], max_radii2D [N].
//   * g = accum / denom, NaN -> 0 (0 / 0); a zero denominator over a positive accum is +inf, which counts as selected.
//     The clone test takes torch.norm(g, dim=-1) of a one-element row, |g| here.
//   * smax = max_k exp(scaling_k).  Clone: g >= grad_threshold && smax <= percent_dense * extent.  Split:
//     g >= grad_threshold && smax > percent_dense * extent, decided on the ORIGINAL rows only (the clones get a padded
//     gradient of 0), so no Gaussian is both cloned and split.
//   * Split children, two copies per split source: position R(normalize(q)) (z (.) exp(s)) + xyz with z standard normal
//     (torch.normal(mean = 0, std) then bmm); scaling log(exp(s) / (0.8 * 2)); rotation, f_dc, f_rest, opacity copied raw.
//     A kernel cannot reproduce torch's RNG stream, so z is an input: noise [N,2,3], read for split sources only.
//   * Row order of the result: originals neither split nor pruned (index order), then the kept clones (source order),
//     then the kept first copies of the children, then the kept second copies (repeat(N, 1), cat, prune_filter and the
//     final prune_points).
//   * Prune, on the concatenated set (children with their own reduced scaling): sigmoid(opacity) < min_opacity, or,
//     when max_screen_size is set, max exp(scaling) > 0.1 * extent or max_radii2D > max_screen_size.  The last test
//     reads max_radii2D AFTER densification_postfix reset it to zeros: it is 0 > max_screen_size, which never fires
//     for a positive size (reproduced as that comparison, not dropped).
//   * Adam state: surviving rows keep exp_avg / exp_avg_sq, every new row (clone or child) starts at zero; `step` is
//     untouched (the host side moves the state dict to the new parameter).  The three statistics become zeros of the
//     new N.  prune_points alone (an external mask) keeps the surviving rows of everything, statistics included.
//   * reset_opacity: opacity' = logit(min(sigmoid(o), 0.01)), both moments zero.
//   * Thresholds are fp32 tensors compared with Python floats: torch rounds the double scalar to fp32 once and
//     compares in fp32 (checked on the CPU); the host passes (float)(percent_dense * extent) etc., formed in double.
//   The arithmetic that reproduces torch's formulas is compiled with -ffp-contract=off (build.py STRICT).
//
// Passes: classify (per source: which output slots it fills + per-block counts) -> one-workgroup scan of the block
// counts (three segments; the fourth, second copies, has the first copies' count) -> map (per block: ranks inside the
// block + block offsets -> dst -> (src | slot << 30)).  No atomics, no look-back: the same input gives the same map.
// The count N' stays on the device (and, optionally, is copied to a pinned host word); the apply launch then writes
// every output tensor by destination index.
#include "common.h"
#include "boundary.h"

#define DN_THREADS 256
#define DN_ITEMS 4                        // sources per thread in classify / map
#define DN_BLOCK (DN_THREADS * DN_ITEMS)  // sources per block
#define DN_SPLIT_DIV 1.6f                 // 0.8 * N with N = 2 (densify_and_split), 1.6000000000000001 -> fp32

// per-source flag bits: GS_DENSIFY_F_* (include/gsplat_mi355.h; the host reads them as the selection masks)
#define DNF_KEEP ((uint32_t)GS_DENSIFY_F_KEEP)
#define DNF_CLONE ((uint32_t)GS_DENSIFY_F_CLONE)
#define DNF_SPLIT ((uint32_t)GS_DENSIFY_F_SPLIT)
#define DNF_PRUNE ((uint32_t)GS_DENSIFY_F_PRUNE)
#define DNF_CHILD_PRUNE ((uint32_t)GS_DENSIFY_F_CHILD_PRUNE)
#define DNF_CLONE_KEPT ((uint32_t)GS_DENSIFY_F_CLONE_KEPT)
#define DNF_CHILDREN_KEPT ((uint32_t)GS_DENSIFY_F_CHILDREN_KEPT)

static inline int dn_blocks(int N) { return (N + DN_BLOCK - 1) / DN_BLOCK; }

// workspace layout: flags u8[N] | block counts u32[3, blocks] | block offsets u32[3, blocks] | totals u32[4] |
// map u32[2 N] (N' <= 2 N: a source fills at most two rows)
struct DnWs {
    uint8_t* flags;
    uint32_t* counts;
    uint32_t* offsets;
    uint32_t* totals;  // n_keep, n_clone, n_child, N'
    uint32_t* map;
};
static inline size_t dn_carve(int N, void* base, DnWs* w) {
    const size_t nb = (size_t)dn_blocks(N);
    Carver c(base);
    DnWs ws;
    ws.flags = c.take<uint8_t>((size_t)N);
    ws.counts = c.take<uint32_t>(3 * nb);
    ws.offsets = c.take<uint32_t>(3 * nb);
    ws.totals = c.take<uint32_t>(4);
    ws.map = c.take<uint32_t>(2 * (size_t)N);
    if (w) *w = ws;
    return c.o;
}
static size_t densify_workspace_bytes(int N) { return dn_carve(N, nullptr, nullptr); }

__device__ __forceinline__ float dn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// torch.max(exp(s), dim=1).values
__device__ __forceinline__ float dn_smax(float s0, float s1, float s2) { return fmaxf(fmaxf(expf(s0), expf(s1)), expf(s2)); }
// scaling_inverse_activation(get_scaling / (0.8 * N)): log(exp(s) / 1.6)
__device__ __forceinline__ float dn_child_scale(float s) { return logf(expf(s) / DN_SPLIT_DIV); }

// Sum of three per-thread counts over the workgroup; every thread gets its exclusive prefix (in thread order) and the
// block totals.  Deterministic: wave scans, then a fixed-order pass over the four waves' totals.
__device__ __forceinline__ void dn_block_scan3(uint32_t c[3], uint32_t excl[3], uint32_t tot[3]) {
    __shared__ uint32_t wtot[DN_THREADS / WAVE][3];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    uint32_t incl[3];
    for (int k = 0; k < 3; k++) {
        incl[k] = wave_scan_incl(c[k]);
        if (lane == WAVE - 1) wtot[wv][k] = incl[k];
    }
    __syncthreads();
    for (int k = 0; k < 3; k++) {
        uint32_t before = 0, all = 0;
        for (int j = 0; j < DN_THREADS / WAVE; j++) {
            if (j < wv) before += wtot[j][k];
            all += wtot[j][k];
        }
        excl[k] = before + incl[k] - c[k];
        tot[k] = all;
    }
}

struct DnPlanArgs {
    int N;
    const float* scaling;
    const float* opacity;
    const float* accum;
    const float* denom;
    const uint8_t* prune_mask;
    float grad_threshold, split_scale, min_opacity, max_world_scale, max_screen_size;
    int prune_size;
};

__global__ __launch_bounds__(DN_THREADS) void densify_classify_kernel(DnPlanArgs a, DnWs w) {
    uint32_t c[3] = {0, 0, 0};  // originals kept, clones kept, children kept (per copy)
    const int base = blockIdx.x * DN_BLOCK + threadIdx.x * DN_ITEMS;
#pragma unroll
    for (int j = 0; j < DN_ITEMS; j++) {
        const int i = base + j;
        if (i >= a.N) break;
        uint32_t f;
        if (a.prune_mask) {
            f = a.prune_mask[i] ? DNF_PRUNE : DNF_KEEP;
        } else {
            const float s0 = a.scaling[3 * (size_t)i], s1 = a.scaling[3 * (size_t)i + 1], s2 = a.scaling[3 * (size_t)i + 2];
            float g = a.accum[i] / a.denom[i];
            if (g != g) g = 0.0f;  // grads[grads.isnan()] = 0.0
            const bool sel = fabsf(g) >= a.grad_threshold;
            const float smax = dn_smax(s0, s1, s2);
            const bool clone = sel && smax <= a.split_scale, split = sel && smax > a.split_scale;
            const float op = dn_sigmoid(a.opacity[i]);
            // max_radii2D was zeroed by densification_postfix before the prune reads it
            const bool vs = a.prune_size && 0.0f > a.max_screen_size;
            const bool prune = op < a.min_opacity || vs || (a.prune_size && smax > a.max_world_scale);
            bool child_prune = false;
            if (split) {
                const float cmax = dn_smax(dn_child_scale(s0), dn_child_scale(s1), dn_child_scale(s2));
                child_prune = op < a.min_opacity || vs || (a.prune_size && cmax > a.max_world_scale);
            }
            f = (clone ? DNF_CLONE : 0u) | (split ? DNF_SPLIT : 0u) | (prune ? DNF_PRUNE : 0u) |
                (child_prune ? DNF_CHILD_PRUNE : 0u);
            if (!split && !prune) f |= DNF_KEEP;
            if (clone && !prune) f |= DNF_CLONE_KEPT;
            if (split && !child_prune) f |= DNF_CHILDREN_KEPT;
        }
        w.flags[i] = (uint8_t)f;
        c[0] += (f & DNF_KEEP) ? 1u : 0u;
        c[1] += (f & DNF_CLONE_KEPT) ? 1u : 0u;
        c[2] += (f & DNF_CHILDREN_KEPT) ? 1u : 0u;
    }
    uint32_t excl[3], tot[3];
    dn_block_scan3(c, excl, tot);
    if (threadIdx.x == 0) {
        const size_t nb = gridDim.x;
        for (int k = 0; k < 3; k++) w.counts[k * nb + blockIdx.x] = tot[k];
    }
}

// one workgroup: exclusive offsets of the block counts per segment, and the totals
__global__ __launch_bounds__(DN_THREADS) void densify_scan_kernel(int nb, DnWs w) {
    uint32_t carry[3] = {0, 0, 0};
    for (int start = 0; start < nb; start += DN_THREADS) {
        const int b = start + threadIdx.x;
        uint32_t c[3], excl[3], tot[3];
        for (int k = 0; k < 3; k++) c[k] = b < nb ? w.counts[(size_t)k * nb + b] : 0u;
        dn_block_scan3(c, excl, tot);
        if (b < nb)
            for (int k = 0; k < 3; k++) w.offsets[(size_t)k * nb + b] = carry[k] + excl[k];
        for (int k = 0; k < 3; k++) carry[k] += tot[k];
        __syncthreads();  // (the shared wave totals are rewritten by the next round)
    }
    if (threadIdx.x == 0) {
        w.totals[0] = carry[0];
        w.totals[1] = carry[1];
        w.totals[2] = carry[2];
        w.totals[3] = carry[0] + carry[1] + 2u * carry[2];
    }
}

// dst -> (src | slot << 30); slot 0 original, 1 clone, 2 first child, 3 second child
__global__ __launch_bounds__(DN_THREADS) void densify_map_kernel(int N, DnWs w) {
    const size_t nb = gridDim.x;
    const uint32_t n_keep = w.totals[0], n_clone = w.totals[1], n_child = w.totals[2];
    const int base = blockIdx.x * DN_BLOCK + threadIdx.x * DN_ITEMS;
    uint32_t f[DN_ITEMS];
    uint32_t c[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < DN_ITEMS; j++) {
        f[j] = base + j < N ? w.flags[base + j] : 0u;
        c[0] += (f[j] & DNF_KEEP) ? 1u : 0u;
        c[1] += (f[j] & DNF_CLONE_KEPT) ? 1u : 0u;
        c[2] += (f[j] & DNF_CHILDREN_KEPT) ? 1u : 0u;
    }
    uint32_t excl[3], tot[3];
    dn_block_scan3(c, excl, tot);
    uint32_t r0 = w.offsets[blockIdx.x] + excl[0];
    uint32_t r1 = n_keep + w.offsets[nb + blockIdx.x] + excl[1];
    uint32_t r2 = n_keep + n_clone + w.offsets[2 * nb + blockIdx.x] + excl[2];
#pragma unroll
    for (int j = 0; j < DN_ITEMS; j++) {
        const uint32_t i = (uint32_t)(base + j);
        if (f[j] & DNF_KEEP) w.map[r0++] = i;
        if (f[j] & DNF_CLONE_KEPT) w.map[r1++] = i | (1u << 30);
        if (f[j] & DNF_CHILDREN_KEPT) {
            w.map[r2] = i | (2u << 30);
            w.map[r2 + n_child] = i | (3u << 30);
            r2++;
        }
    }
}

static int launch_densify_plan(const GsDensifyPlan& p, void* workspace, int32_t* count_host, hipStream_t s) {
    DnWs w;
    dn_carve(p.N, (char*)workspace, &w);
    DnPlanArgs a{p.N, p.scaling, p.opacity, p.grad_accum, p.denom, p.prune_mask, p.grad_threshold, p.split_scale,
                 p.min_opacity, p.max_world_scale, p.max_screen_size, p.prune_size};
    const int nb = dn_blocks(p.N);
    StageScope st("densify_plan", s);
    if (nb > 0) {
        hipLaunchKernelGGL(densify_classify_kernel, dim3(nb), dim3(DN_THREADS), 0, s, a, w);
        GS_LAUNCH_CHECK("densify_classify", 0, s);
    }
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_THREADS), 0, s, nb, w);
    GS_LAUNCH_CHECK("densify_scan", 0, s);
    if (nb > 0) {
        hipLaunchKernelGGL(densify_map_kernel, dim3(nb), dim3(DN_THREADS), 0, s, p.N, w);
        GS_LAUNCH_CHECK("densify_map", 0, s);
    }
    if (count_host) {
        if (hipMemcpyAsync(count_host, w.totals + 3, 4, hipMemcpyDeviceToHost, s) != hipSuccess) {
            gs_set_error((int)hipGetLastError(), "densify_count");
            return GS_E_HIP;
        }
    }
    return GS_OK;
}

// ---- apply: every output row by destination index, all tensors in one launch (chunks of 1024 elements as AdamBatch)
struct DnApplyBatch {
    GsDensifyTensor t[GS_DENSIFY_MAX_TENSORS];
    long long elems[GS_DENSIFY_MAX_TENSORS];  // elements of the destination: N' x width
    long long start[GS_DENSIFY_MAX_TENSORS + 1];
    int n;
};

// child position R(normalize(q)) (z (.) exp(s)) + xyz, component c, in the reference's operation order
// (utils/general_utils.py build_rotation; torch.normal(mean = 0, std) = 0 + std z)
__device__ __forceinline__ float dn_child_pos(const float* __restrict__ xyz, const float* __restrict__ scaling,
                                              const float* __restrict__ rotation, const float* __restrict__ noise,
                                              uint32_t src, int copy, int c) {
    const float* q = rotation + 4 * (size_t)src;
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float nrm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / nrm, x = q1 / nrm, y = q2 / nrm, z = q3 / nrm;
    float R0, R1, R2;
    if (c == 0) {
        R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - r * z); R2 = 2.0f * (x * z + r * y);
    } else if (c == 1) {
        R0 = 2.0f * (x * y + r * z); R1 = 1.0f - 2.0f * (x * x + z * z); R2 = 2.0f * (y * z - r * x);
    } else {
        R0 = 2.0f * (x * z - r * y); R1 = 2.0f * (y * z + r * x); R2 = 1.0f - 2.0f * (x * x + y * y);
    }
    const float* zz = noise + 6 * (size_t)src + 3 * copy;
    const float* ss = scaling + 3 * (size_t)src;
    const float p0 = 0.0f + expf(ss[0]) * zz[0], p1 = 0.0f + expf(ss[1]) * zz[1], p2 = 0.0f + expf(ss[2]) * zz[2];
    return (R0 * p0 + R1 * p1 + R2 * p2) + xyz[3 * (size_t)src + c];
}

__global__ __launch_bounds__(256) void densify_apply_kernel(DnApplyBatch b, const uint32_t* __restrict__ map,
                                                            const uint32_t* __restrict__ totals, const float* __restrict__ scaling,
                                                            const float* __restrict__ rotation,
                                                            const float* __restrict__ noise) {
    const long long chunk = blockIdx.x;
    int k = 0;
    while (k + 1 < b.n && chunk >= b.start[k + 1]) k++;
    const GsDensifyTensor T = b.t[k];
    const uint32_t wd = (uint32_t)T.width;
    const long long n = b.elems[k], base = (chunk - b.start[k]) * 1024;
    const uint32_t n_dev = totals[3];  // rows past the plan's own count (a caller's N' too large) are written as zeros
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long e = base + j * 256 + threadIdx.x;
        if (e >= n) break;
        const uint32_t row = (uint32_t)(e / wd), c = (uint32_t)(e - (long long)row * wd);
        if (row >= n_dev) {
            T.dst[e] = 0.0f;
            continue;
        }
        const uint32_t m = map[row], src = m & 0x3FFFFFFFu, slot = m >> 30;
        float v;
        switch (T.kind) {
            case GS_DENSIFY_ZERO: v = 0.0f; break;
            case GS_DENSIFY_ZERO_IF_NEW: v = slot == 0 ? T.src[(size_t)src * wd + c] : 0.0f; break;
            case GS_DENSIFY_CHILD_SCALING:
                v = slot >= 2 ? dn_child_scale(T.src[(size_t)src * wd + c]) : T.src[(size_t)src * wd + c];
                break;
            case GS_DENSIFY_CHILD_POSITION:
                v = slot >= 2 ? dn_child_pos(T.src, scaling, rotation, noise, src, (int)slot - 2, (int)c)
                              : T.src[(size_t)src * wd + c];
                break;
            default: v = T.src[(size_t)src * wd + c]; break;
        }
        T.dst[e] = v;
    }
}

static int launch_densify_apply(int N, int N_new, const void* workspace, int n, const GsDensifyTensor* tensors,
                                const float* scaling, const float* rotation, const float* noise, hipStream_t s) {
    DnWs w;
    dn_carve(N, (char*)const_cast<void*>(workspace), &w);
    DnApplyBatch b;
    b.n = n;
    long long chunks = 0;
    for (int k = 0; k < n; k++) {
        b.t[k] = tensors[k];
        b.elems[k] = (long long)N_new * tensors[k].width;
        b.start[k] = chunks;
        chunks += (b.elems[k] + 1023) / 1024;
    }
    b.start[n] = chunks;
    if (chunks == 0) return GS_OK;
    StageScope st("densify_apply", s);
    hipLaunchKernelGGL(densify_apply_kernel, dim3((unsigned)chunks), dim3(256), 0, s, b, w.map, w.totals, scaling, rotation,
                       noise);
    GS_LAUNCH_CHECK("densify_apply", 0, s);
    return GS_OK;
}

// ---- reset_opacity: inverse_sigmoid(min(sigmoid(o), 0.01)) = log(x / (1 - x)); both moments zeroed
__global__ __launch_bounds__(256) void reset_opacity_kernel(int N, const float* __restrict__ in, float* __restrict__ out,
                                                            float* __restrict__ m, float* __restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float x = fminf(dn_sigmoid(in[i]), 0.01f);
    out[i] = logf(x / (1.0f - x));
    if (m) m[i] = 0.0f;
    if (v) v[i] = 0.0f;
}

static int launch_reset_opacity(int N, const float* in, float* out, float* exp_avg, float* exp_avg_sq, hipStream_t s) {
    StageScope st("reset_opacity", s);
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, in, out, exp_avg, exp_avg_sq);
    GS_LAUNCH_CHECK("reset_opacity", 0, s);
    return GS_OK;
}

extern "C" {

// N < 2^30: the map packs a source index and a two-bit slot into 32 bits, and N' <= 2 N stays an int32
#define GS_DENSIFY_MAX_N (1 << 30)
int gs_densify_workspace_bytes(int32_t N, size_t* out) {
    if (!out || N < 0 || N >= GS_DENSIFY_MAX_N) return GS_E_BAD_ARG;
    *out = densify_workspace_bytes(N);
    return GS_OK;
}
int gs_densify_plan(const GsDensifyPlan* p, void* workspace, size_t workspace_bytes, int32_t* count_host_pinned,
                    void* stream) {
    GS_CAPTURE_OK_IF(stream, count_host_pinned == nullptr);
    if (!p || !workspace || p->N < 0 || p->N >= GS_DENSIFY_MAX_N) return GS_E_BAD_ARG;
    if (p->N > 0 && !p->prune_mask && (!p->scaling || !p->opacity || !p->grad_accum || !p->denom)) return GS_E_BAD_ARG;
    if (workspace_bytes < densify_workspace_bytes(p->N)) return GS_E_WORKSPACE;
    return launch_densify_plan(*p, workspace, count_host_pinned, (hipStream_t)stream);
}
int gs_densify_apply(int32_t N, int32_t N_new, const void* workspace, size_t workspace_bytes, int32_t n_tensors,
                     const GsDensifyTensor* tensors, const float* scaling, const float* rotation, const float* noise,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || N >= GS_DENSIFY_MAX_N || N_new < 0 || N_new > 2 * N || !workspace || n_tensors < 0 ||
        n_tensors > GS_DENSIFY_MAX_TENSORS || (n_tensors > 0 && !tensors))
        return GS_E_BAD_ARG;
    if (workspace_bytes < densify_workspace_bytes(N)) return GS_E_WORKSPACE;
    for (int k = 0; k < n_tensors; k++) {
        const GsDensifyTensor& t = tensors[k];
        if (t.width <= 0 || t.kind < GS_DENSIFY_COPY || t.kind > GS_DENSIFY_CHILD_SCALING) return GS_E_BAD_ARG;
        if (N_new > 0 && (!t.dst || (t.kind != GS_DENSIFY_ZERO && !t.src))) return GS_E_BAD_ARG;
        if ((t.kind == GS_DENSIFY_CHILD_POSITION || t.kind == GS_DENSIFY_CHILD_SCALING) && t.width != 3) return GS_E_BAD_ARG;
        if (t.kind == GS_DENSIFY_CHILD_POSITION && N_new > 0 && (!scaling || !rotation || !noise)) return GS_E_BAD_ARG;
    }
    if (N_new == 0 || n_tensors == 0) return GS_OK;
    return launch_densify_apply(N, N_new, workspace, n_tensors, tensors, scaling, rotation, noise, (hipStream_t)stream);
}
int gs_reset_opacity(int32_t N, const float* opacity_in, float* opacity_out, float* exp_avg, float* exp_avg_sq,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (N > 0 && (!opacity_in || !opacity_out))) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_reset_opacity(N, opacity_in, opacity_out, exp_avg, exp_avg_sq, (hipStream_t)stream);
}

}  // extern "C"
