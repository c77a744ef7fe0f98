// skinloss.hip -- the rigid deformer's skinning regulariser (models/deformer/rigid.py SkinningField.sample_skinning_loss
// :173-187 and get_skinning_loss :198-212, AABB.normalize at utils/dataset_utils.py:72-76) on the device: the surface
// samples of the canonical mesh with their blended skinning weights in one launch, the loss in two and its gradient in
// one, instead of host sampling (trimesh, igl, numpy), two host-to-device copies and ~100 small torch operators.
//
// Spec (fp32 throughout unless said otherwise; nothing is contracted into FMAs):
//   Sampling, per sample i from three uniform draws u = draws[i] in [0, 1):
//   * face pick: pick = u0 * cdf[F-1] (one fp32 multiply), cdf (F) the non-decreasing cumulative face areas;
//     face = the smallest k with cdf[k] >= pick, by binary search, clamped to F-1: numpy's searchsorted(cdf, pick),
//     side "left".  A face of zero area after a face of positive area repeats its predecessor's cdf and is never the
//     smallest such k.
//   * barycentric draws: a = u1, b = u2; if a + b > 1 (the fp32 sum) then a = |a - 1|, b = |b - 1| (the fold of the unit
//     square that trimesh's sample_surface documents).
//   * point: p = (v0 + a (v1 - v0)) + b (v2 - v0) with (v0, v1, v2) the face's vertices; its barycentric weights are
//     bary = ((1 - a) - b, a, b) (the reference recomputes them from p with igl: the same numbers up to rounding).
//   * target (24) = (bary0 vweights[i0] + bary1 vweights[i1]) + bary2 vweights[i2], vweights the (V, 24) table.
//   * p_norm = (2 (p - aabb_min)) aabb_inv_extent - 1 (AABB.normalize(., sym=True) with the division turned into a
//     multiply by the reciprocal extent that the caller rounds once).
//   Vertex indices outside [0, V) are clamped into it (the caller validates the face list once on the host; the clamp
//   keeps a bad list from reading out of bounds).  The uniform draws are the caller's: the distribution is trimesh's,
//   the random stream is not numpy's.
//   Loss, from logits (n, 25) (GS_SKIN_HIERARCHICAL) or (n, 24) (GS_SKIN_SOFTMAX) and target (n, 24):
//   W = the activation of skinning.hip's spec; r_i = sum_j (W_ij - target_ij)^2 with j in order; loss = (sum_i r_i) / n
//   (mse_loss(., 'none').sum(-1).mean()).  The r_i of a block are added in double by a fixed tree (row t += row t + s for
//   s = 128, 64, .., 1), the blocks' sums in block order, in double; the quotient is rounded to fp32 once.
//   Gradient: dW_ij = (W_ij - target_ij) c with c = (2 g) / n, g = dL/dloss read from device memory (one multiply and
//   one correctly rounded division: with g = n, c = 2 exactly); dlogits = dW through the activation.  The target gets no
//   gradient.
//   n = 0: nothing is launched and the loss is 0 (torch's mean over no rows gives nan: that is not reproduced).
//
// Kernels (SKIN_THREADS threads, one per sample or row; a block's rows of odd width leave and enter as its contiguous
// slab with 16-byte accesses, as in skinning.hip, whose device functions skin_act.h shares):
//   skin_sample        the sampling above; p_norm and target, and face, bary, p when their pointers are given.
//   skin_loss_fwd      r_i per row, one double partial per block.
//   skin_loss_final    one wave: runs64_sum (ordered_sum.h) of the block partials, divided by n, into loss[0].
//   skin_loss_bwd      recomputes W and writes every dlogits row once.
// No atomics, no memsets, no host reads: every result is bitwise reproducible, and the calls are capture-safe.
#include "common.h"
#include "boundary.h"
#include "skin_act.h"

static inline int skinloss_blocks(int n) { return (n + SKIN_THREADS - 1) / SKIN_THREADS; }
static size_t skin_loss_workspace_bytes(int n) { return (size_t)skinloss_blocks(n) * sizeof(double); }

__device__ __forceinline__ int clamp_vertex(int i, int V) { return min(max(i, 0), V - 1); }

__global__ __launch_bounds__(SKIN_THREADS) void skin_sample_kernel(
    int n, int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ cdf,
    const float* __restrict__ vweights, const float* __restrict__ aabb_min, const float* __restrict__ aabb_inv_extent,
    const float* __restrict__ draws, float* __restrict__ p_norm, float* __restrict__ target, int* __restrict__ face_out,
    float* __restrict__ bary_out, float* __restrict__ p_out) {
    __shared__ float4 tgt4[SKIN_THREADS * 24 / 4];
    __shared__ float4 row4[SKIN_THREADS * 3 / 4];  // p_norm, then bary, then p
    float* tgt = reinterpret_cast<float*>(tgt4);
    float* row = reinterpret_cast<float*>(row4);
    const int row0 = blockIdx.x * SKIN_THREADS, cnt = min(SKIN_THREADS, n - row0), t = threadIdx.x;
    float pn[3] = {0.0f, 0.0f, 0.0f}, bc[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    if (t < cnt) {
        const size_t i = (size_t)row0 + t;
        const float u0 = draws[3 * i];
        float a = draws[3 * i + 1], b = draws[3 * i + 2];
        const float pick = u0 * cdf[F - 1];
        int lo = 0, hi = F;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] < pick) lo = mid + 1;
            else hi = mid;
        }
        const int f = min(lo, F - 1);
        if (face_out) face_out[i] = f;
        if (a + b > 1.0f) {
            a = fabsf(a - 1.0f);
            b = fabsf(b - 1.0f);
        }
        bc[0] = (1.0f - a) - b;
        bc[1] = a;
        bc[2] = b;
        int vi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) vi[k] = clamp_vertex(faces[3 * (size_t)f + k], V);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v0 = verts[3 * (size_t)vi[0] + c], v1 = verts[3 * (size_t)vi[1] + c], v2 = verts[3 * (size_t)vi[2] + c];
            p[c] = (v0 + a * (v1 - v0)) + b * (v2 - v0);
            pn[c] = (2.0f * (p[c] - aabb_min[c])) * aabb_inv_extent[c] - 1.0f;
        }
        const float4* w0 = reinterpret_cast<const float4*>(vweights + 24 * (size_t)vi[0]);
        const float4* w1 = reinterpret_cast<const float4*>(vweights + 24 * (size_t)vi[1]);
        const float4* w2 = reinterpret_cast<const float4*>(vweights + 24 * (size_t)vi[2]);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const float4 x = w0[k], y = w1[k], z = w2[k];
            tgt4[6 * t + k] = make_float4((bc[0] * x.x + bc[1] * y.x) + bc[2] * z.x, (bc[0] * x.y + bc[1] * y.y) + bc[2] * z.y,
                                          (bc[0] * x.z + bc[1] * y.z) + bc[2] * z.z, (bc[0] * x.w + bc[1] * y.w) + bc[2] * z.w);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) row[3 * t + c] = pn[c];
    }
    __syncthreads();
    skin_slab_store<24>(target, row0, cnt, tgt);
    skin_slab_store<3>(p_norm, row0, cnt, row);
    if (bary_out) {  // (uniform)
        __syncthreads();
        if (t < cnt) {
#pragma unroll
            for (int c = 0; c < 3; c++) row[3 * t + c] = bc[c];
        }
        __syncthreads();
        skin_slab_store<3>(bary_out, row0, cnt, row);
    }
    if (p_out) {  // (uniform)
        __syncthreads();
        if (t < cnt) {
#pragma unroll
            for (int c = 0; c < 3; c++) row[3 * t + c] = p[c];
        }
        __syncthreads();
        skin_slab_store<3>(p_out, row0, cnt, row);
    }
}

__device__ __forceinline__ void target_row(const float* __restrict__ target, size_t i, float* tg) {
    const float4* g = reinterpret_cast<const float4*>(target + 24 * i);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const float4 v = g[k];
        tg[4 * k] = v.x; tg[4 * k + 1] = v.y; tg[4 * k + 2] = v.z; tg[4 * k + 3] = v.w;
    }
}

template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_loss_fwd_kernel(int n, const float* __restrict__ logits,
                                                                     const float* __restrict__ target,
                                                                     double* __restrict__ partial) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 buf4[SKIN_THREADS * C / 4];
    __shared__ double srow[SKIN_THREADS];
    float* buf = reinterpret_cast<float*>(buf4);
    const int row0 = blockIdx.x * SKIN_THREADS, cnt = min(SKIN_THREADS, n - row0), t = threadIdx.x;
    skin_slab_load<C>(logits, row0, cnt, buf);
    __syncthreads();
    double r = 0.0;
    if (t < cnt) {
        float x[C], W[24], tg[24];
        row_from_lds<C>(buf, t, x);
        weights_fwd<KIND>(x, W);
        target_row(target, (size_t)row0 + t, tg);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 24; j++) {
            const float d = W[j] - tg[j];
            s += d * d;
        }
        r = (double)s;
    }
    srow[t] = r;
    __syncthreads();
    for (int s = SKIN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) srow[t] += srow[t + s];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = srow[0];
}

__global__ __launch_bounds__(64) void skin_loss_final_kernel(int n, int nb, const double* __restrict__ partial,
                                                             float* __restrict__ loss) {
    __shared__ double run[64];
    const double s = runs64_sum(partial, nb, run);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}

template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_loss_bwd_kernel(int n, const float* __restrict__ logits,
                                                                     const float* __restrict__ target,
                                                                     const float* __restrict__ dL_dloss,
                                                                     float* __restrict__ dL_dlogits) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 buf4[SKIN_THREADS * C / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    const int row0 = blockIdx.x * SKIN_THREADS, cnt = min(SKIN_THREADS, n - row0), t = threadIdx.x;
    skin_slab_load<C>(logits, row0, cnt, buf);
    __syncthreads();
    const float c = (2.0f * dL_dloss[0]) / (float)n;
    float dx[C];
    if (t < cnt) {
        float x[C], W[24], tg[24], dW[24];
        row_from_lds<C>(buf, t, x);
        weights_fwd<KIND>(x, W);
        target_row(target, (size_t)row0 + t, tg);
#pragma unroll
        for (int j = 0; j < 24; j++) dW[j] = (W[j] - tg[j]) * c;
        weights_bwd<KIND>(x, W, dW, dx);
    }
    __syncthreads();
    if (t < cnt) {
#pragma unroll
        for (int k = 0; k < C; k++) buf[t * C + k] = dx[k];
    }
    __syncthreads();
    skin_slab_store<C>(dL_dlogits, row0, cnt, buf);
}

// ---- launchers (the C ABI has checked every argument; n > 0)
static int launch_mesh_sample(int n, int V, int F, const float* verts, const int* faces, const float* cdf, const float* vweights,
                              const float* aabb_min, const float* aabb_inv_extent, const float* draws, float* p_norm, float* target,
                              int* face, float* bary, float* points, hipStream_t s) {
    StageScope st("skin_sample", s);
    hipLaunchKernelGGL(skin_sample_kernel, dim3(skinloss_blocks(n)), dim3(SKIN_THREADS), 0, s, n, V, F, verts, faces, cdf,
                       vweights, aabb_min, aabb_inv_extent, draws, p_norm, target, face, bary, points);
    GS_LAUNCH_CHECK("skin_sample", 0, s);
    return GS_OK;
}
static int launch_skin_loss_forward(int n, int kind, const float* logits, const float* target, float* loss, void* workspace,
                                    hipStream_t s) {
    StageScope st("skin_loss", s);
    const int nb = skinloss_blocks(n);
    double* partial = reinterpret_cast<double*>(workspace);
    if (kind == GS_SKIN_HIERARCHICAL)
        hipLaunchKernelGGL(skin_loss_fwd_kernel<GS_SKIN_HIERARCHICAL>, dim3(nb), dim3(SKIN_THREADS), 0, s, n, logits, target,
                           partial);
    else
        hipLaunchKernelGGL(skin_loss_fwd_kernel<GS_SKIN_SOFTMAX>, dim3(nb), dim3(SKIN_THREADS), 0, s, n, logits, target, partial);
    GS_LAUNCH_CHECK("skin_loss", 0, s);
    hipLaunchKernelGGL(skin_loss_final_kernel, dim3(1), dim3(64), 0, s, n, nb, partial, loss);
    GS_LAUNCH_CHECK("skin_loss_final", 0, s);
    return GS_OK;
}
static int launch_skin_loss_backward(int n, int kind, const float* logits, const float* target, const float* dL_dloss,
                                     float* dL_dlogits, hipStream_t s) {
    StageScope st("skin_loss_bwd", s);
    const int nb = skinloss_blocks(n);
    if (kind == GS_SKIN_HIERARCHICAL)
        hipLaunchKernelGGL(skin_loss_bwd_kernel<GS_SKIN_HIERARCHICAL>, dim3(nb), dim3(SKIN_THREADS), 0, s, n, logits, target,
                           dL_dloss, dL_dlogits);
    else
        hipLaunchKernelGGL(skin_loss_bwd_kernel<GS_SKIN_SOFTMAX>, dim3(nb), dim3(SKIN_THREADS), 0, s, n, logits, target,
                           dL_dloss, dL_dlogits);
    GS_LAUNCH_CHECK("skin_loss_bwd", 0, s);
    return GS_OK;
}

extern "C" {

static bool skin_loss_kind_ok(int32_t kind) { return kind == GS_SKIN_HIERARCHICAL || kind == GS_SKIN_SOFTMAX; }
int gs_mesh_sample(int32_t n, int32_t V, int32_t F, const float* verts, const int32_t* faces, const float* cdf,
                   const float* vweights, const float* aabb_min, const float* aabb_inv_extent, const float* draws,
                   float* points_norm, float* target, int32_t* face, float* bary, float* points, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || V < 1 || F < 1) return GS_E_BAD_ARG;
    if (!required(verts, 4) || !required(faces, 4) || !required(cdf, 4) || !required(vweights, 16) || !required(aabb_min, 4) ||
        !required(aabb_inv_extent, 4))
        return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!required(draws, 4) || !required(points_norm, 16) || !required(target, 16)) return GS_E_BAD_ARG;
    if (!aligned(face, 4) || !aligned(bary, 16) || !aligned(points, 16)) return GS_E_BAD_ARG;
    return launch_mesh_sample(n, V, F, verts, faces, cdf, vweights, aabb_min, aabb_inv_extent, draws, points_norm, target, face,
                              bary, points, (hipStream_t)stream);
}
int gs_skin_loss_workspace_bytes(int32_t n, size_t* out) {
    if (!out || n < 0) return GS_E_BAD_ARG;
    *out = skin_loss_workspace_bytes(n);
    return GS_OK;
}
int gs_skin_loss_forward(int32_t n, int32_t kind, const float* logits, const float* target, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || !skin_loss_kind_ok(kind)) return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!required(logits, 16) || !required(target, 16) || !required(loss, 4) || !required(workspace, 16)) return GS_E_BAD_ARG;
    if (workspace_bytes < skin_loss_workspace_bytes(n)) return GS_E_WORKSPACE;
    return launch_skin_loss_forward(n, kind, logits, target, loss, workspace, (hipStream_t)stream);
}
int gs_skin_loss_backward(int32_t n, int32_t kind, const float* logits, const float* target, const float* dL_dloss,
                          float* dL_dlogits, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || !skin_loss_kind_ok(kind)) return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!required(logits, 16) || !required(target, 16) || !required(dL_dloss, 4) || !required(dL_dlogits, 16)) return GS_E_BAD_ARG;
    return launch_skin_loss_backward(n, kind, logits, target, dL_dloss, dL_dlogits, (hipStream_t)stream);
}

}  // extern "C"
