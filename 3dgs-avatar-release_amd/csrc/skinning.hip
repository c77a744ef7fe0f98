// skinning.hip -- the rigid deformer's linear blend skinning (models/deformer/rigid.py SkinningField.forward :215-236,
// SMPLNN.forward :49-71, hierarchical_softmax :85-129, build_rotation at utils/general_utils.py:87-108) as one forward
// launch and one backward launch (plus a small reduction when the bone transforms want a gradient), instead of ~60 small
// torch operators and a GEMM backward whose summation order the project does not control.
//
// Spec (per Gaussian n; fp32 throughout, as the reference trains):
//   Weights W (24), from a row of one of three kinds:
//   * GS_SKIN_HIERARCHICAL, 25 logits x: s_k = sigmoid(x_k); starting from p = 1, in this order:
//       1. p1..3 = s0 softmax(x1..3); p0 = 1 - s0.
//       2. p4..6 = p1..3 s4..6, then p1..3 *= (1 - s4..6).
//       3. p7..9 = p4..6 s7..9, then p4..6 *= (1 - s7..9).
//       4. p10,11 = p7,8 s10,11, then p7,8 *= (1 - s10,11).
//       5. p12..14 = (p9 s24) softmax(x12..14), then p9 *= (1 - s24).
//       6. p15 = p12 s15, then p12 *= (1 - s15).
//       7. p16,17 = p13,14 s16,17, then p13,14 *= (1 - s16,17).
//       8. p18,19 = p16,17 s18,19, then p16,17 *= (1 - s18,19).
//       9. p20,21 = p18,19 s20,21, then p18,19 *= (1 - s20,21).
//      10. p22,23 = p20,21 s22,23, then p20,21 *= (1 - s22,23).
//     s1..3 and s12..14 are unused; both softmaxes subtract their maximum (F.softmax).  Every step but 1 and 5 is a
//     "split" of a parent slot P by the gate of its child slot C: p_C = v s_C, p_P = v (1 - s_C), v = p_P before it.
//   * GS_SKIN_SOFTMAX, 24 logits: F.softmax over the row.
//   * GS_SKIN_WEIGHTS, 24 given weights (SMPLNN: the nearest SMPL vertex's): W = the row.
//   T (4x4) = sum_j W_j tfs_j, tfs = camera.bone_transforms (24, 4, 4), all 16 entries (row 3 included); it is an output
//   (T_fwd, which the reference detaches: it carries no gradient).
//   xbar = T[:3,:3] x + T[:3,3]; Rbar = T[:3,:3] R(q), q = r / |r| (the raw (w,x,y,z) quaternion, no epsilon), R as
//   build_rotation (gs_math.h quat_to_R).
// Backward, from g = dL/dxbar (3) and G = dL/dRbar (3x3), either absent = 0:
//   dT[:3,:3] = g x^T + G R^T, dT[:3,3] = g, row 3 of dT = 0.
//   dW_j = <dT, tfs_j> over rows 0..2; dlogits = dW through the kind's activation (GS_SKIN_WEIGHTS: dW itself).
//   dtfs_j = sum_n W_nj dT_n (row 3 = 0).  dx = T[:3,:3]^T g (the direct term only).  dr = (dq - q (q . dq)) / |r| with
//   dq from T[:3,:3]^T G through build_rotation (gs_math.h quat_R_backward).
//
// Kernels (SKIN_THREADS threads, one per Gaussian or row; tfs is copied into LDS, every lane then reads the same word):
//   skin_weights_fwd / _bwd   the activation alone (get_skinning_loss's hierarchical_softmax / F.softmax).
//   skin_fwd                  W, T, xbar, Rbar; writes T_fwd with 16-byte stores, xbar and Rbar through LDS.
//   skin_bwd                  recomputes W, T and R from the inputs (nothing is kept from the forward) and writes dlogits
//                             (or dW), dx and dr, each row once; every row's W and dT pass through LDS.  With dtfs
//                             wanted, 216 threads sum W_nj dT_n over three fixed thirds of the block's rows in double; the
//                             thirds are added in order and the block's 24 x 12 partial (double) goes to the workspace.
//   skin_dtfs_reduce          one wave per dtfs element: runs64_sum (ordered_sum.h) of its block partials, rounded to
//                             fp32 once; rows 3 are written 0.
// Logit rows (100 or 96 bytes) and the outputs of odd width are moved between global memory and LDS as the block's
// contiguous slab, with 16-byte accesses: a block's slab starts at row 256 b, so a 16-byte aligned base keeps every slab
// 16-byte aligned.  No atomics, no memsets: every gradient is bitwise reproducible, and the calls are capture-safe.
// The activations and their reverses are in skin_act.h, which skinloss.hip shares; the slab moves are slab.h's.
#include "common.h"
#include "boundary.h"
#include "gs_math.h"
#include "skin_act.h"

#define SKIN_BONES GS_SKIN_BONES
#define SKIN_TASKS 72   // (bone, row) pairs of dtfs; each thread of a task sums four columns
#define SKIN_THIRD 86   // rows of one third of a block (the last has 84)

static inline int skin_blocks(int N) { return (N + SKIN_THREADS - 1) / SKIN_THREADS; }
static size_t skinning_workspace_bytes(int N) { return (size_t)skin_blocks(N) * (SKIN_BONES * 12) * sizeof(double); }

// ---- the activation alone
template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_weights_fwd_kernel(int N, const float* __restrict__ logits,
                                                                        float* __restrict__ weights) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 buf4[SKIN_THREADS * C / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    const int row0 = blockIdx.x * SKIN_THREADS, n = min(SKIN_THREADS, N - row0), t = threadIdx.x;
    skin_slab_load<C>(logits, row0, n, buf);
    __syncthreads();
    if (t >= n) return;
    float x[C], W[24];
    row_from_lds<C>(buf, t, x);
    weights_fwd<KIND>(x, W);
    float4* o = reinterpret_cast<float4*>(weights + (size_t)(row0 + t) * 24);
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = make_float4(W[4 * k], W[4 * k + 1], W[4 * k + 2], W[4 * k + 3]);
}

template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_weights_bwd_kernel(int N, const float* __restrict__ logits,
                                                                        const float* __restrict__ dL_dweights,
                                                                        float* __restrict__ dL_dlogits) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 buf4[SKIN_THREADS * C / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    const int row0 = blockIdx.x * SKIN_THREADS, n = min(SKIN_THREADS, N - row0), t = threadIdx.x;
    skin_slab_load<C>(logits, row0, n, buf);
    __syncthreads();
    float dx[C];
    if (t < n) {
        float x[C], W[24], dW[24];
        row_from_lds<C>(buf, t, x);
        if (KIND == GS_SKIN_SOFTMAX) weights_fwd<KIND>(x, W);
        const float4* g = reinterpret_cast<const float4*>(dL_dweights + (size_t)(row0 + t) * 24);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const float4 v = g[k];
            dW[4 * k] = v.x; dW[4 * k + 1] = v.y; dW[4 * k + 2] = v.z; dW[4 * k + 3] = v.w;
        }
        weights_bwd<KIND>(x, W, dW, dx);
    }
    __syncthreads();
    if (t < n) {
#pragma unroll
        for (int k = 0; k < C; k++) buf[t * C + k] = dx[k];
    }
    __syncthreads();
    skin_slab_store<C>(dL_dlogits, row0, n, buf);
}

// ---- skinning
__device__ __forceinline__ void load_tfs(const float* __restrict__ tfs, float4* s_tfs4) {
    if (threadIdx.x < SKIN_BONES * 4) s_tfs4[threadIdx.x] = reinterpret_cast<const float4*>(tfs)[threadIdx.x];
}
// T[e] = sum_j W_j tfs_j[e] for e < E (E = 16: the whole matrix; 12: rows 0..2)
template <int E>
__device__ __forceinline__ void blend(const float* W, const float* s_tfs, float* T) {
#pragma unroll
    for (int e = 0; e < E; e++) T[e] = W[0] * s_tfs[e];
#pragma unroll
    for (int j = 1; j < SKIN_BONES; j++)
#pragma unroll
        for (int e = 0; e < E; e++) T[e] += W[j] * s_tfs[16 * j + e];
}

template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_fwd_kernel(int N, const float* __restrict__ w, const float* __restrict__ tfs,
                                                                const float* __restrict__ xyz, const float* __restrict__ rot,
                                                                float* __restrict__ xyz_out, float* __restrict__ rot_out,
                                                                float* __restrict__ T_out) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 s_tfs4[SKIN_BONES * 4];
    __shared__ float4 buf4[SKIN_THREADS * C / 4];  // logit rows, then xbar (3) and Rbar (9) rows
    float* buf = reinterpret_cast<float*>(buf4);
    const float* s_tfs = reinterpret_cast<const float*>(s_tfs4);
    const int row0 = blockIdx.x * SKIN_THREADS, n = min(SKIN_THREADS, N - row0), t = threadIdx.x;
    load_tfs(tfs, s_tfs4);
    skin_slab_load<C>(w, row0, n, buf);
    __syncthreads();
    float W[24];
    if (t < n) {
        float x[C];
        row_from_lds<C>(buf, t, x);
        weights_fwd<KIND>(x, W);
    }
    __syncthreads();
    if (t < n) {
        const size_t i = (size_t)row0 + t;
        float T[16];
        blend<16>(W, s_tfs, T);
        float4* To = reinterpret_cast<float4*>(T_out + 16 * i);
#pragma unroll
        for (int r = 0; r < 4; r++) To[r] = make_float4(T[4 * r], T[4 * r + 1], T[4 * r + 2], T[4 * r + 3]);
        const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
#pragma unroll
        for (int r = 0; r < 3; r++) buf[3 * t + r] = T[4 * r] * px + T[4 * r + 1] * py + T[4 * r + 2] * pz + T[4 * r + 3];
        float nrm, R[3][3];
        quat_to_R(quat_normalize(reinterpret_cast<const float4*>(rot)[i], &nrm), R);
        float* Rb = buf + 3 * SKIN_THREADS + 9 * t;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) Rb[3 * r + c] = T[4 * r] * R[0][c] + T[4 * r + 1] * R[1][c] + T[4 * r + 2] * R[2][c];
    }
    __syncthreads();
    skin_slab_store<3>(xyz_out, row0, n, buf);
    skin_slab_store<9>(rot_out, row0, n, buf + 3 * SKIN_THREADS);
}

// LDS of the backward: the logit slab, then every row's W (stride 25: no bank conflicts) and dT (stride 12); the dlogit
// slab last.  W and dT pass through LDS even without dtfs: a blend over 24 bones fully unrolled on registers lets the
// scheduler hoist every tfs load and spill
#define SKIN_WS 25
#define SKIN_BWD_WORDS (SKIN_THREADS * (SKIN_WS + 12))

template <int KIND>
__global__ __launch_bounds__(SKIN_THREADS) void skin_bwd_kernel(int N, const float* __restrict__ w, const float* __restrict__ tfs,
                                                                const float* __restrict__ xyz, const float* __restrict__ rot,
                                                                const float* __restrict__ dxyz_out, const float* __restrict__ drot_out,
                                                                float* __restrict__ dw, float* __restrict__ dxyz,
                                                                float* __restrict__ drot, double* __restrict__ partial) {
    constexpr int C = SkinKind<KIND>::C;
    __shared__ float4 s_tfs4[SKIN_BONES * 4];
    __shared__ float4 buf4[SKIN_BWD_WORDS / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    float* sW = buf;                            // [256][25]
    float* sT = buf + SKIN_THREADS * SKIN_WS;   // [256][12]
    const float* s_tfs = reinterpret_cast<const float*>(s_tfs4);
    const int row0 = blockIdx.x * SKIN_THREADS, n = min(SKIN_THREADS, N - row0), t = threadIdx.x;
    load_tfs(tfs, s_tfs4);
    skin_slab_load<C>(w, row0, n, buf);
    __syncthreads();
    float x[C], dx[C];
    if (t < n) row_from_lds<C>(buf, t, x);
    __syncthreads();
    if (t < n) {
        const size_t i = (size_t)row0 + t;
        {
            float W[24];
            weights_fwd<KIND>(x, W);
#pragma unroll
            for (int j = 0; j < 24; j++) sW[SKIN_WS * t + j] = W[j];
        }
        float T[12];  // rows 0..2 of sum_j W_j tfs_j (-0 + a = a: the same bits as starting from the first term)
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = -0.0f;
#pragma unroll 4
        for (int j = 0; j < SKIN_BONES; j++) {
            const float wj = sW[SKIN_WS * t + j];
#pragma unroll
            for (int e = 0; e < 12; e++) T[e] += wj * s_tfs[16 * j + e];
        }
        float g[3] = {0.0f, 0.0f, 0.0f}, G[9];
        if (dxyz_out) {
#pragma unroll
            for (int r = 0; r < 3; r++) g[r] = dxyz_out[3 * i + r];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) G[k] = 0.0f;
        if (drot_out) {
#pragma unroll
            for (int k = 0; k < 9; k++) G[k] = drot_out[9 * i + k];
        }
        const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        float nrm, R[3][3];
        const float4 q = quat_normalize(reinterpret_cast<const float4*>(rot)[i], &nrm);
        quat_to_R(q, R);
        // dT[:3,:3] = g x^T + G R^T, dT[:3,3] = g
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                sT[12 * t + 4 * r + c] = g[r] * p[c] + (G[3 * r] * R[c][0] + G[3 * r + 1] * R[c][1] + G[3 * r + 2] * R[c][2]);
            sT[12 * t + 4 * r + 3] = g[r];
        }
        if (dxyz) {
#pragma unroll
            for (int a = 0; a < 3; a++) dxyz[3 * i + a] = T[a] * g[0] + T[4 + a] * g[1] + T[8 + a] * g[2];
        }
        if (drot) {
            float dR[3][3];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) dR[a][b] = T[a] * G[b] + T[4 + a] * G[3 + b] + T[8 + a] * G[6 + b];
            reinterpret_cast<float4*>(drot)[i] = quat_R_backward(q, nrm, dR);
        }
        if (dw) {
            float dW[24], W[24];  // dW_j = sum_e dT_e tfs_j[e], e in order
#pragma unroll
            for (int j = 0; j < 24; j++) dW[j] = -0.0f;
#pragma unroll 2
            for (int e = 0; e < 12; e++) {
                const float d = sT[12 * t + e];
#pragma unroll
                for (int j = 0; j < SKIN_BONES; j++) dW[j] += d * s_tfs[16 * j + e];
            }
            if (KIND == GS_SKIN_SOFTMAX) {
#pragma unroll
                for (int j = 0; j < 24; j++) W[j] = sW[SKIN_WS * t + j];
            }
            weights_bwd<KIND>(x, W, dW, dx);
        }
    }
    if (partial) {
        __syncthreads();
        // task = (bone j, row r): four columns; three threads per task sum fixed thirds of the block's rows
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        const int task = t % SKIN_TASKS, part = t / SKIN_TASKS, j = task / 3, r = task % 3;
        if (part < 3) {
            const int m1 = min(n, (part + 1) * SKIN_THIRD);
            for (int m = part * SKIN_THIRD; m < m1; m++) {
                const double wj = (double)sW[SKIN_WS * m + j];
                const float4 d = reinterpret_cast<const float4*>(sT + 12 * m)[r];
                acc[0] += wj * (double)d.x;
                acc[1] += wj * (double)d.y;
                acc[2] += wj * (double)d.z;
                acc[3] += wj * (double)d.w;
            }
        }
        __syncthreads();
        double* sP = reinterpret_cast<double*>(buf4);  // [3][72][4]
        if (part < 3) {
#pragma unroll
            for (int c = 0; c < 4; c++) sP[4 * t + c] = acc[c];
        }
        __syncthreads();
        if (t < SKIN_TASKS) {
            const size_t nb = gridDim.x;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const double a = sP[4 * t + c] + sP[4 * (SKIN_TASKS + t) + c] + sP[4 * (2 * SKIN_TASKS + t) + c];
                partial[(size_t)(12 * j + 4 * r + c) * nb + blockIdx.x] = a;
            }
        }
    }
    if (dw) {  // (uniform)
        __syncthreads();
        if (t < n) {
#pragma unroll
            for (int k = 0; k < C; k++) buf[t * C + k] = dx[k];
        }
        __syncthreads();
        skin_slab_store<C>(dw, row0, n, buf);
    }
}

// one wave per dtfs element o = 12 j + e (e < 12); the rows 3 are written by the waves of e = 0
__global__ __launch_bounds__(64) void skin_dtfs_reduce_kernel(int nb, const double* __restrict__ partial, float* __restrict__ dtfs) {
    __shared__ double run[64];
    const int o = blockIdx.x, l = threadIdx.x, j = o / 12, e = o % 12;
    const double s = runs64_sum(partial + (size_t)o * nb, nb, run);
    if (l == 0) dtfs[16 * j + e] = (float)s;
    if (e == 0 && l < 4) dtfs[16 * j + 12 + l] = 0.0f;
}

// ---- launchers (the C ABI has checked every argument)
#define SKIN_DISPATCH(kind, KERNEL, ...)                                                                            \
    switch (kind) {                                                                                                 \
        case GS_SKIN_HIERARCHICAL: hipLaunchKernelGGL(KERNEL<GS_SKIN_HIERARCHICAL>, __VA_ARGS__); break;           \
        case GS_SKIN_SOFTMAX: hipLaunchKernelGGL(KERNEL<GS_SKIN_SOFTMAX>, __VA_ARGS__); break;                     \
        default: hipLaunchKernelGGL(KERNEL<GS_SKIN_WEIGHTS>, __VA_ARGS__); break;                                  \
    }

static int launch_skin_weights_forward(int N, int kind, const float* logits, float* weights, hipStream_t s) {
    StageScope st("skin_weights", s);
    SKIN_DISPATCH(kind, skin_weights_fwd_kernel, dim3(skin_blocks(N)), dim3(SKIN_THREADS), 0, s, N, logits, weights)
    GS_LAUNCH_CHECK("skin_weights", 0, s);
    return GS_OK;
}
static int launch_skin_weights_backward(int N, int kind, const float* logits, const float* dL_dweights, float* dL_dlogits,
                                        hipStream_t s) {
    StageScope st("skin_weights_bwd", s);
    SKIN_DISPATCH(kind, skin_weights_bwd_kernel, dim3(skin_blocks(N)), dim3(SKIN_THREADS), 0, s, N, logits, dL_dweights,
                  dL_dlogits)
    GS_LAUNCH_CHECK("skin_weights_bwd", 0, s);
    return GS_OK;
}
static int launch_skinning_forward(int N, int kind, const float* w, const float* tfs, const float* xyz, const float* rot,
                                   float* xyz_out, float* rot_out, float* T_fwd, hipStream_t s) {
    StageScope st("skinning", s);
    SKIN_DISPATCH(kind, skin_fwd_kernel, dim3(skin_blocks(N)), dim3(SKIN_THREADS), 0, s, N, w, tfs, xyz, rot, xyz_out, rot_out,
                  T_fwd)
    GS_LAUNCH_CHECK("skinning", 0, s);
    return GS_OK;
}
static int launch_skinning_backward(int N, int kind, const float* w, const float* tfs, const float* xyz, const float* rot,
                                    const float* dxyz_out, const float* drot_out, float* dw, float* dtfs, float* dxyz, float* drot,
                                    void* workspace, hipStream_t s) {
    StageScope st("skinning_bwd", s);
    const int nb = skin_blocks(N);
    double* partial = dtfs ? reinterpret_cast<double*>(workspace) : nullptr;
    SKIN_DISPATCH(kind, skin_bwd_kernel, dim3(nb), dim3(SKIN_THREADS), 0, s, N, w, tfs, xyz, rot, dxyz_out, drot_out, dw, dxyz,
                  drot, partial)
    GS_LAUNCH_CHECK("skinning_bwd", 0, s);
    if (dtfs) {
        hipLaunchKernelGGL(skin_dtfs_reduce_kernel, dim3(SKIN_BONES * 12), dim3(64), 0, s, nb, partial, dtfs);
        GS_LAUNCH_CHECK("skinning_dtfs", 0, s);
    }
    return GS_OK;
}

extern "C" {

static bool skin_kind_ok(int32_t kind) { return kind == GS_SKIN_HIERARCHICAL || kind == GS_SKIN_SOFTMAX || kind == GS_SKIN_WEIGHTS; }
int gs_skin_weights_forward(int32_t N, int32_t kind, const float* logits, float* weights, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (kind != GS_SKIN_HIERARCHICAL && kind != GS_SKIN_SOFTMAX)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!required(logits, 16) || !required(weights, 16)) return GS_E_BAD_ARG;
    return launch_skin_weights_forward(N, kind, logits, weights, (hipStream_t)stream);
}
int gs_skin_weights_backward(int32_t N, int32_t kind, const float* logits, const float* dL_dweights, float* dL_dlogits,
                             void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (kind != GS_SKIN_HIERARCHICAL && kind != GS_SKIN_SOFTMAX)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!required(logits, 16) || !required(dL_dweights, 16) || !required(dL_dlogits, 16)) return GS_E_BAD_ARG;
    return launch_skin_weights_backward(N, kind, logits, dL_dweights, dL_dlogits, (hipStream_t)stream);
}
int gs_skinning_workspace_bytes(int32_t N, size_t* out) {
    if (!out || N < 0) return GS_E_BAD_ARG;
    *out = skinning_workspace_bytes(N);
    return GS_OK;
}
int gs_skinning_forward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                        float* xyz_out, float* rotation_out, float* T_fwd, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || !skin_kind_ok(kind)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!required(w, 16) || !required(tfs, 16) || !required(xyz, 4) || !required(rotation, 16) || !required(xyz_out, 16) ||
        !required(rotation_out, 16) || !required(T_fwd, 16))
        return GS_E_BAD_ARG;
    return launch_skinning_forward(N, kind, w, tfs, xyz, rotation, xyz_out, rotation_out, T_fwd, (hipStream_t)stream);
}
int gs_skinning_backward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                         const float* dL_dxyz_out, const float* dL_drotation_out, float* dL_dw, float* dL_dtfs,
                         float* dL_dxyz, float* dL_drotation, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || !skin_kind_ok(kind)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!required(w, 16) || !required(tfs, 16) || !required(xyz, 4) || !required(rotation, 16)) return GS_E_BAD_ARG;
    if (!aligned(dL_dxyz_out, 4) || !aligned(dL_drotation_out, 4) || !aligned(dL_dw, 16) || !aligned(dL_dtfs, 4) ||
        !aligned(dL_dxyz, 4) || !aligned(dL_drotation, 16))
        return GS_E_BAD_ARG;
    if (dL_dtfs) {
        if (!required(workspace, 16)) return GS_E_BAD_ARG;
        if (workspace_bytes < skinning_workspace_bytes(N)) return GS_E_WORKSPACE;
    }
    if (!dL_dw && !dL_dtfs && !dL_dxyz && !dL_drotation) return GS_OK;
    return launch_skinning_backward(N, kind, w, tfs, xyz, rotation, dL_dxyz_out, dL_drotation_out, dL_dw, dL_dtfs, dL_dxyz,
                                    dL_drotation, workspace, (hipStream_t)stream);
}

}  // extern "C"
