// pose.hip -- the SMPL forward of `pose_correction: direct` (models/pose_correction/pose_correction.py
// DirectPoseOptimization.pose_correct :225-252 through PoseCorrection._forward_smpl :131-188, get_transforms_02v :14-77
// and models/pose_correction/lbs.py) as two forward launches and one backward launch, instead of well over a hundred
// small torch operators, two host-built rotations copied to the device every step and an autograd replay of all of it.
//
// Spec (batch 1, 24 joints, fp32 throughout as the reference trains; V vertices and NB <= 16 betas at run time):
//   Rest joints    J_j = J_template_j + J_shapedirs_j . betas, with J_template = J_regressor v_template (24, 3) and
//                  J_shapedirs = J_regressor shapedirs (24, 3, NB) folded once by the caller: the joints are linear in
//                  betas and the regressor is never read here.
//   Statistics     of v_shaped = v_template + shapedirs . betas (V, 3), all three detached (no gradient): centre = its
//                  mean over the vertices (3); cmin / cmax = the smallest / largest of (v_shaped - centre) over all
//                  vertices and axes.  (Per axis, min_v (v - c) = (min_v v) - c exactly, rounding being monotonic.)
//   Jtrs_j         = (((J_j - centre) - cmin + 0.05 (cmax - cmin)) / (cmax - cmin) / 1.1 - 0.5) 2.
//   Rotations      pose = (root_orient, pose_body, pose_hand) as 24 axis-angle rows r.  a = |r + 1e-8| (the epsilon is
//                  added to every coordinate inside the norm only), n = r / a, K = [n]x, R = I + sin a K + (1 - cos a) K K.
//                  A zero row gives R = I and a finite gradient.
//   rots           (24, 9): row 0 the identity, rows 1..23 R_1..R_23.
//   Chain          G_0 = [R_0 | J_0]; for i = 1..23, p = parents[i] < i: rot G_i = rot G_p R_i, t G_i = rot G_p (J_i - J_p)
//                  + t G_p.  The relative transform is A_i = [rot G_i | t G_i - rot G_i J_i].
//   Star pose      The A-pose -> star-pose transform B_i is the identity except on the leg chains (1, 4, 7, 10), rotated
//                  about z by +45 degrees, and (2, 5, 8, 11), by -45 degrees.  Along a chain the reference accumulates
//                  t_k = Z (J_k - J_prev) + t_prev from t_hip = J_hip and then subtracts Z J_k: the sum telescopes, so
//                  every joint of a chain has the same translation (I - Z) J_hip.  B_i is rigid: with Q = Z^T,
//                  inv(B_i) = [Q | (I - Q) J_hip], and
//   bone_i         = A_i inv(B_i) + trans = [rot G_i Q | t G_i - rot G_i u_i + trans], u_i = J_i + (Q - I) J_hip
//                  (u_i = J_i off the chains); row 3 = (0, 0, 0, 1).
//   loss_pose      = mean((rots_gt - rots)^2) over the 216 entries, when rots_gt is given.
// Backward, from g_rots (24, 9), g_Jtrs (24, 3), g_bone (24, 4, 4; row 3 ignored) and g_loss (a device scalar), any of
// them absent = 0:
//   dJ_i = g_Jtrs_i 2 / (1.1 (cmax - cmin)) - rot G_i^T gt_i (gt_i = g_bone_i[:3, 3]), plus (Q - I)^T of that second
//   term onto the chain's hip, joints of a chain in order; d rot G_i = g_bone_i[:3,:3] Q^T - gt_i u_i^T; d t G_i = gt_i;
//   dtrans = sum_i gt_i, i ascending.  Then the tree from the leaves to the root, i = 23..1, p = parents[i]:
//   dR_i = rot G_p^T d rot G_i; e = rot G_p^T d t G_i, dJ_i += e, dJ_p -= e; d rot G_p += d rot G_i R_i^T + d t G_i
//   (J_i - J_p)^T; d t G_p += d t G_i; at the root dR_0 = d rot G_0, dJ_0 += d t G_0.  For i >= 1, dR_i += g_rots_i +
//   g_loss 2 (R_i - rots_gt_i) / 216.  Through Rodrigues: dK = sin a dR + (1 - cos a) (dR K^T + K^T dR), da = cos a
//   <dR, K> + sin a <dR, K K>, dn = the axial vector of dK - dK^T, da -= dn . r / a^2, dr = dn / a + da (r + 1e-8) / a.
//   dbetas_l = sum_{j,k} dJ_jk J_shapedirs_jkl, (j, k) ascending.
//
// Kernels:
//   pose_stats_kernel  at most POSE_MAX_BLOCKS blocks of 256 threads stride over the vertices; a lane past V contributes
//                      nothing (sum 0, min +inf, max -inf).  Per axis: the sum in double, min and max; a fixed tree over
//                      the block, then nine doubles per block to the workspace.
//   pose_fwd_kernel    one wave.  Lanes 0..8 fold the block partials in block order while the others shape the joints
//                      and run Rodrigues, one joint per lane; lane 0 walks the chain in LDS (23 dependent 3x3 products:
//                      there is nothing to spread); then one joint per lane writes bone_transforms.  It saves centre,
//                      cmin, cmax, J, R and rot G (GS_POSE_STATE_FLOATS floats) for the backward.
//   pose_bwd_kernel    one wave; reads the saved state, never the vertices.  Per-joint work is one joint per lane, the tree
//                      is walked by lane 0 alone, dbetas is one lane per beta: every sum has one fixed order.
// The launch boundary between the first two is the only cross-workgroup hand-off: no ticket, no grid barrier, no
// atomics, no memset.  Every gradient is bitwise reproducible and the calls are capture-safe.
#include "common.h"
#include "boundary.h"

#define POSE_BONES GS_POSE_BONES
#define POSE_THREADS 256
#define POSE_MAX_BLOCKS 32
#define POSE_WAVE 64
// the saved state, in floats
#define POSE_ST_STAT 0    // centre (3), cmin, cmax
#define POSE_ST_J 8       // (24, 3)
#define POSE_ST_R 80      // (24, 3, 3)
#define POSE_ST_G 296     // (24, 3, 3)
static_assert(POSE_ST_G + POSE_BONES * 9 == GS_POSE_STATE_FLOATS, "state layout");

struct PoseTree {
    int p[POSE_BONES];
};

static inline int pose_blocks(int V) {
    const int b = (V + POSE_THREADS - 1) / POSE_THREADS;
    return b < POSE_MAX_BLOCKS ? b : POSE_MAX_BLOCKS;
}
static size_t pose_workspace_bytes(int V) { return (size_t)pose_blocks(V) * 9 * sizeof(double); }

// ---- the statistics of the shaped template
__global__ __launch_bounds__(POSE_THREADS) void pose_stats_kernel(int V, int NB, const float* __restrict__ v_template,
                                                                  const float* __restrict__ shapedirs,
                                                                  const float* __restrict__ betas, double* __restrict__ partial) {
    __shared__ double red[9][POSE_THREADS];
    __shared__ float s_b[GS_POSE_MAX_BETAS];
    const int t = threadIdx.x;
    if (t < NB) s_b[t] = betas[t];
    __syncthreads();
    double sum[3] = {0.0, 0.0, 0.0};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t v = (size_t)blockIdx.x * POSE_THREADS + t; v < (size_t)V; v += (size_t)gridDim.x * POSE_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float* sd = shapedirs + (3 * v + k) * NB;
            float d = sd[0] * s_b[0];
            for (int l = 1; l < NB; l++) d += sd[l] * s_b[l];
            const float x = v_template[3 * v + k] + d;
            sum[k] += (double)x;
            lo[k] = fminf(lo[k], x);
            hi[k] = fmaxf(hi[k], x);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        red[k][t] = sum[k];
        red[3 + k][t] = (double)lo[k];
        red[6 + k][t] = (double)hi[k];
    }
    __syncthreads();
    for (int s = POSE_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                red[k][t] += red[k][t + s];
                red[3 + k][t] = fmin(red[3 + k][t], red[3 + k][t + s]);
                red[6 + k][t] = fmax(red[6 + k][t], red[6 + k][t + s]);
            }
        }
        __syncthreads();
    }
    if (t < 9) partial[9 * blockIdx.x + t] = red[t][0];
}

// ---- pieces shared by the forward and the backward
__device__ __forceinline__ const float* pose_row(int j, const float* root, const float* body, const float* hand) {
    return j == 0 ? root : j < 22 ? body + 3 * (j - 1) : hand + 3 * (j - 22);
}
__device__ __forceinline__ void skew_of(const float* n, float* K) {
    K[0] = 0.0f;  K[1] = -n[2]; K[2] = n[1];
    K[3] = n[2];  K[4] = 0.0f;  K[5] = -n[0];
    K[6] = -n[1]; K[7] = n[0];  K[8] = 0.0f;
}
__device__ __forceinline__ void mat3_mul(const float* A, const float* B, float* C) {  // C = A B
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ float rodrigues_angle(const float* r, float* n) {
    const float ex = r[0] + 1e-8f, ey = r[1] + 1e-8f, ez = r[2] + 1e-8f;
    const float a = sqrtf(ex * ex + ey * ey + ez * ez);
    n[0] = r[0] / a; n[1] = r[1] / a; n[2] = r[2] / a;
    return a;
}
__device__ __forceinline__ void rodrigues_fwd(const float* r, float* R) {
    float n[3], K[9], KK[9];
    const float a = rodrigues_angle(r, n);
    skew_of(n, K);
    mat3_mul(K, K, KK);
    const float s = sinf(a), c1 = 1.0f - cosf(a);
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = ((e % 4 == 0) ? 1.0f : 0.0f) + s * K[e] + c1 * KK[e];
}
__device__ __forceinline__ void rodrigues_bwd(const float* r, const float* dR, float* dr) {
    float n[3], K[9], KK[9];
    const float a = rodrigues_angle(r, n);
    skew_of(n, K);
    mat3_mul(K, K, KK);
    const float s = sinf(a), c = cosf(a), c1 = 1.0f - c;
    float ds = 0.0f, dc = 0.0f, dK[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        ds += dR[e] * K[e];
        dc += dR[e] * KK[e];
    }
    // dK = s dR + (1 - c) (dR K^T + K^T dR)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float m = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) m += dR[3 * i + k] * K[3 * j + k] + K[3 * k + i] * dR[3 * k + j];
            dK[3 * i + j] = s * dR[3 * i + j] + c1 * m;
        }
    const float dn[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    float da = c * ds + s * dc;
    da -= (dn[0] * r[0] + dn[1] * r[1] + dn[2] * r[2]) / (a * a);
#pragma unroll
    for (int k = 0; k < 3; k++) dr[k] = dn[k] / a + da * (r[k] + 1e-8f) / a;
}
// the star-pose rotation of joint i: sg = +1 on the left leg chain (1, 4, 7, 10), -1 on the right (2, 5, 8, 11), else 0;
// Q = [[c, sg s, 0], [-sg s, c, 0], [0, 0, 1]] with c = s = cos 45 degrees; *hip = the chain's first joint
#define POSE_C45 0.70710678118654752f
__device__ __forceinline__ float star_sign(int i, int* hip) {
    if (i >= 1 && i <= 11 && i % 3 != 0) {
        *hip = i % 3;
        return i % 3 == 1 ? 1.0f : -1.0f;
    }
    *hip = 0;
    return 0.0f;
}
// u_i = J_i + (Q - I) J_hip
__device__ __forceinline__ void star_offset(const float* J, int i, float sg, int hip, float* u) {
    u[0] = J[3 * i]; u[1] = J[3 * i + 1]; u[2] = J[3 * i + 2];
    if (sg != 0.0f) {
        const float x = J[3 * hip], y = J[3 * hip + 1], c1 = POSE_C45 - 1.0f, s = sg * POSE_C45;
        u[0] += c1 * x + s * y;
        u[1] += c1 * y - s * x;
    }
}

// ---- forward: everything but the vertex pass
__global__ __launch_bounds__(POSE_WAVE) void pose_fwd_kernel(PoseTree tree, int V, int NB, int nb, const double* __restrict__ partial,
                                                             const float* __restrict__ Jt, const float* __restrict__ Jsd,
                                                             const float* __restrict__ betas, const float* __restrict__ root,
                                                             const float* __restrict__ body, const float* __restrict__ hand,
                                                             const float* __restrict__ trans, const float* __restrict__ rots_gt,
                                                             float* __restrict__ rots, float* __restrict__ Jtrs,
                                                             float* __restrict__ bone, float* __restrict__ loss,
                                                             float* __restrict__ state) {
    __shared__ double s_red[9];
    __shared__ float s_J[POSE_BONES * 3], s_R[POSE_BONES * 9], s_G[POSE_BONES * 9], s_Gt[POSE_BONES * 3], s_l[POSE_BONES];
    __shared__ int s_par[POSE_BONES];
    const int t = threadIdx.x;
    if (t < 9) {  // block partials, in block order
        double a = partial[t];
        for (int b = 1; b < nb; b++) {
            const double v = partial[9 * b + t];
            a = t < 3 ? a + v : t < 6 ? fmin(a, v) : fmax(a, v);
        }
        s_red[t] = a;
    }
    if (t < POSE_BONES) {
        s_par[t] = t == 0 ? 0 : tree.p[t];
        rodrigues_fwd(pose_row(t, root, body, hand), s_R + 9 * t);
    }
    for (int e = t; e < POSE_BONES * 3; e += POSE_WAVE) {
        float j = Jt[e];
        for (int l = 0; l < NB; l++) j += Jsd[e * NB + l] * betas[l];
        s_J[e] = j;
    }
    __syncthreads();
    float center[3], cmin = INFINITY, cmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        center[k] = (float)(s_red[k] / (double)V);
        cmin = fminf(cmin, (float)s_red[3 + k] - center[k]);
        cmax = fmaxf(cmax, (float)s_red[6 + k] - center[k]);
    }
    const float extent = cmax - cmin, padding = extent * 0.05f;
    for (int e = t; e < POSE_BONES * 3; e += POSE_WAVE) {
        float x = s_J[e] - center[e % 3];
        x = (x - cmin + padding) / extent / 1.1f;
        x -= 0.5f;
        Jtrs[e] = x * 2.0f;
        state[POSE_ST_J + e] = s_J[e];
    }
    if (t < 3) state[POSE_ST_STAT + t] = center[t];
    if (t == 3) state[POSE_ST_STAT + 3] = cmin;
    if (t == 4) state[POSE_ST_STAT + 4] = cmax;
    if (t == 0) {  // the chain: parents[i] < i
#pragma unroll
        for (int e = 0; e < 9; e++) s_G[e] = s_R[e];
#pragma unroll
        for (int k = 0; k < 3; k++) s_Gt[k] = s_J[k];
        for (int i = 1; i < POSE_BONES; i++) {
            const int p = s_par[i];
            float P[9], Ri[9], rel[3], Gi[9];
#pragma unroll
            for (int e = 0; e < 9; e++) {
                P[e] = s_G[9 * p + e];
                Ri[e] = s_R[9 * i + e];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) rel[k] = s_J[3 * i + k] - s_J[3 * p + k];
            mat3_mul(P, Ri, Gi);
#pragma unroll
            for (int e = 0; e < 9; e++) s_G[9 * i + e] = Gi[e];
#pragma unroll
            for (int r = 0; r < 3; r++)
                s_Gt[3 * i + r] = P[3 * r] * rel[0] + P[3 * r + 1] * rel[1] + P[3 * r + 2] * rel[2] + s_Gt[3 * p + r];
        }
    }
    __syncthreads();
    for (int e = t; e < POSE_BONES * 9; e += POSE_WAVE) {
        const float r = s_R[e];
        rots[e] = e < 9 ? (e % 4 == 0 ? 1.0f : 0.0f) : r;
        state[POSE_ST_R + e] = r;
        state[POSE_ST_G + e] = s_G[e];
    }
    if (t < POSE_BONES) {
        int hip;
        const float sg = star_sign(t, &hip);
        float u[3], G[9];
        star_offset(s_J, t, sg, hip, u);
#pragma unroll
        for (int e = 0; e < 9; e++) G[e] = s_G[9 * t + e];
        float* o = bone + 16 * t;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (sg != 0.0f) {
                const float s = sg * POSE_C45;
                o[4 * r] = POSE_C45 * G[3 * r] - s * G[3 * r + 1];
                o[4 * r + 1] = s * G[3 * r] + POSE_C45 * G[3 * r + 1];
            } else {
                o[4 * r] = G[3 * r];
                o[4 * r + 1] = G[3 * r + 1];
            }
            o[4 * r + 2] = G[3 * r + 2];
            o[4 * r + 3] = s_Gt[3 * t + r] - (G[3 * r] * u[0] + G[3 * r + 1] * u[1] + G[3 * r + 2] * u[2]) + trans[r];
        }
        o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
    }
    if (rots_gt) {  // (uniform)
        if (t < POSE_BONES) {
            float a = 0.0f;
#pragma unroll
            for (int e = 0; e < 9; e++) {
                const float r = t == 0 ? (e % 4 == 0 ? 1.0f : 0.0f) : s_R[9 * t + e];
                const float d = rots_gt[9 * t + e] - r;
                a += d * d;
            }
            s_l[t] = a;
        }
        __syncthreads();
        if (t == 0) {
            float a = s_l[0];
            for (int j = 1; j < POSE_BONES; j++) a += s_l[j];
            *loss = a / (float)(POSE_BONES * 9);
        }
    }
}

// ---- backward
__global__ __launch_bounds__(POSE_WAVE) void pose_bwd_kernel(PoseTree tree, int NB, const float* __restrict__ Jsd,
                                                             const float* __restrict__ root, const float* __restrict__ body,
                                                             const float* __restrict__ hand, const float* __restrict__ rots_gt,
                                                             const float* __restrict__ state, const float* __restrict__ g_rots,
                                                             const float* __restrict__ g_Jtrs, const float* __restrict__ g_bone,
                                                             const float* __restrict__ g_loss, float* __restrict__ dbetas,
                                                             float* __restrict__ droot, float* __restrict__ dbody,
                                                             float* __restrict__ dhand, float* __restrict__ dtrans) {
    __shared__ float s_J[POSE_BONES * 3], s_R[POSE_BONES * 9], s_G[POSE_BONES * 9];
    __shared__ float s_dJ[POSE_BONES * 3], s_dG[POSE_BONES * 9], s_dGt[POSE_BONES * 3], s_dR[POSE_BONES * 9], s_hip[POSE_BONES * 2];
    __shared__ int s_par[POSE_BONES];
    const int t = threadIdx.x;
    for (int e = t; e < POSE_BONES * 3; e += POSE_WAVE) s_J[e] = state[POSE_ST_J + e];
    for (int e = t; e < POSE_BONES * 9; e += POSE_WAVE) {
        s_R[e] = state[POSE_ST_R + e];
        s_G[e] = state[POSE_ST_G + e];
    }
    if (t < POSE_BONES) s_par[t] = t == 0 ? 0 : tree.p[t];
    __syncthreads();
    if (t < POSE_BONES) {  // through bone_transforms and Jtrs, one joint per lane
        const float scale = 2.0f / (1.1f * (state[POSE_ST_STAT + 4] - state[POSE_ST_STAT + 3]));
        float gr[9], gt[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) gr[3 * r + c] = g_bone ? g_bone[16 * t + 4 * r + c] : 0.0f;
            gt[r] = g_bone ? g_bone[16 * t + 4 * r + 3] : 0.0f;
        }
        int hip;
        const float sg = star_sign(t, &hip), s = sg * POSE_C45;
        float u[3];
        star_offset(s_J, t, sg, hip, u);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            float q0 = gr[3 * r], q1 = gr[3 * r + 1];
            if (sg != 0.0f) {  // gr Q^T
                q0 = POSE_C45 * gr[3 * r] + s * gr[3 * r + 1];
                q1 = POSE_C45 * gr[3 * r + 1] - s * gr[3 * r];
            }
            s_dG[9 * t + 3 * r] = q0 - gt[r] * u[0];
            s_dG[9 * t + 3 * r + 1] = q1 - gt[r] * u[1];
            s_dG[9 * t + 3 * r + 2] = gr[3 * r + 2] - gt[r] * u[2];
            s_dGt[3 * t + r] = gt[r];
        }
        float du[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            du[k] = -(s_G[9 * t + k] * gt[0] + s_G[9 * t + 3 + k] * gt[1] + s_G[9 * t + 6 + k] * gt[2]);
            s_dJ[3 * t + k] = (g_Jtrs ? g_Jtrs[3 * t + k] * scale : 0.0f) + du[k];
        }
        // (Q - I)^T du, onto the hip
        s_hip[2 * t] = sg != 0.0f ? (POSE_C45 - 1.0f) * du[0] - s * du[1] : 0.0f;
        s_hip[2 * t + 1] = sg != 0.0f ? s * du[0] + (POSE_C45 - 1.0f) * du[1] : 0.0f;
    }
    if (t >= 32 && t < 35 && dtrans) {
        const int k = t - 32;
        float a = 0.0f;
        if (g_bone)
            for (int i = 0; i < POSE_BONES; i++) a += g_bone[16 * i + 4 * k + 3];
        dtrans[k] = a;
    }
    __syncthreads();
    if (t == 0) {
        for (int h = 1; h <= 2; h++)
            for (int i = h; i <= 9 + h; i += 3) {
                s_dJ[3 * h] += s_hip[2 * i];
                s_dJ[3 * h + 1] += s_hip[2 * i + 1];
            }
        for (int i = POSE_BONES - 1; i >= 1; i--) {  // leaves to root
            const int p = s_par[i];
            float P[9], Ri[9], dGi[9], dGti[3], rel[3];
#pragma unroll
            for (int e = 0; e < 9; e++) {
                P[e] = s_G[9 * p + e];
                Ri[e] = s_R[9 * i + e];
                dGi[e] = s_dG[9 * i + e];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                dGti[k] = s_dGt[3 * i + k];
                rel[k] = s_J[3 * i + k] - s_J[3 * p + k];
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    s_dR[9 * i + 3 * r + c] = P[r] * dGi[c] + P[3 + r] * dGi[3 + c] + P[6 + r] * dGi[6 + c];
                    s_dG[9 * p + 3 * r + c] += (dGi[3 * r] * Ri[3 * c] + dGi[3 * r + 1] * Ri[3 * c + 1] + dGi[3 * r + 2] * Ri[3 * c + 2])
                                               + dGti[r] * rel[c];
                }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float e = P[k] * dGti[0] + P[3 + k] * dGti[1] + P[6 + k] * dGti[2];
                s_dJ[3 * i + k] += e;
                s_dJ[3 * p + k] -= e;
                s_dGt[3 * p + k] += dGti[k];
            }
        }
#pragma unroll
        for (int e = 0; e < 9; e++) s_dR[e] = s_dG[e];
#pragma unroll
        for (int k = 0; k < 3; k++) s_dJ[k] += s_dGt[k];
    }
    __syncthreads();
    if (t < POSE_BONES) {
        float* out = t == 0 ? droot : t < 22 ? (dbody ? dbody + 3 * (t - 1) : nullptr) : (dhand ? dhand + 3 * (t - 22) : nullptr);
        if (out) {
            float dR[9], dr[3];
            const float gl = (g_loss && rots_gt) ? g_loss[0] * 2.0f / (float)(POSE_BONES * 9) : 0.0f;
#pragma unroll
            for (int e = 0; e < 9; e++) {
                dR[e] = s_dR[9 * t + e];
                if (t > 0) {  // rots[0] is the constant identity
                    float d = g_rots ? g_rots[9 * t + e] : 0.0f;
                    if (g_loss && rots_gt) d += gl * (s_R[9 * t + e] - rots_gt[9 * t + e]);
                    dR[e] += d;
                }
            }
            rodrigues_bwd(pose_row(t, root, body, hand), dR, dr);
            out[0] = dr[0]; out[1] = dr[1]; out[2] = dr[2];
        }
    } else if (t >= 32 && t < 32 + NB && dbetas) {
        const int l = t - 32;
        float a = 0.0f;
        for (int e = 0; e < POSE_BONES * 3; e++) a += s_dJ[e] * Jsd[e * NB + l];
        dbetas[l] = a;
    }
}

// ---- launchers (the C ABI has checked every argument)
static int launch_pose_forward(const GsPoseArgs* a, float* rots, float* Jtrs, float* bone, float* loss, float* state, void* workspace,
                               hipStream_t s) {
    StageScope st("pose", s);
    PoseTree tree;
    for (int i = 0; i < POSE_BONES; i++) tree.p[i] = a->parents[i];
    const int nb = pose_blocks(a->V);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pose_stats_kernel, dim3(nb), dim3(POSE_THREADS), 0, s, a->V, a->NB, a->v_template, a->shapedirs, a->betas,
                       partial);
    GS_LAUNCH_CHECK("pose_stats", 0, s);
    hipLaunchKernelGGL(pose_fwd_kernel, dim3(1), dim3(POSE_WAVE), 0, s, tree, a->V, a->NB, nb, partial, a->J_template,
                       a->J_shapedirs, a->betas, a->root_orient, a->pose_body, a->pose_hand, a->trans, a->rots_gt, rots, Jtrs,
                       bone, loss, state);
    GS_LAUNCH_CHECK("pose", 0, s);
    return GS_OK;
}
static int launch_pose_backward(const GsPoseArgs* a, const float* state, const float* g_rots, const float* g_Jtrs, const float* g_bone,
                                const float* g_loss, float* dbetas, float* droot, float* dbody, float* dhand, float* dtrans,
                                hipStream_t s) {
    StageScope st("pose_bwd", s);
    PoseTree tree;
    for (int i = 0; i < POSE_BONES; i++) tree.p[i] = a->parents[i];
    hipLaunchKernelGGL(pose_bwd_kernel, dim3(1), dim3(POSE_WAVE), 0, s, tree, a->NB, a->J_shapedirs, a->root_orient, a->pose_body,
                       a->pose_hand, a->rots_gt, state, g_rots, g_Jtrs, g_bone, g_loss, dbetas, droot, dbody, dhand, dtrans);
    GS_LAUNCH_CHECK("pose_bwd", 0, s);
    return GS_OK;
}

extern "C" {

static int pose_validate(const GsPoseArgs* a) {
    if (!a || a->V < 1 || a->NB < 1 || a->NB > GS_POSE_MAX_BETAS) return GS_E_BAD_ARG;
    for (int i = 1; i < GS_POSE_BONES; i++)
        if (a->parents[i] < 0 || a->parents[i] >= i) return GS_E_BAD_ARG;
    if (!required(a->J_shapedirs, 4) || !required(a->root_orient, 4) || !required(a->pose_body, 4) || !required(a->pose_hand, 4) ||
        !aligned(a->rots_gt, 4))
        return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_pose_workspace_bytes(int32_t V, size_t* out) {
    if (!out || V < 1) return GS_E_BAD_ARG;
    *out = pose_workspace_bytes(V);
    return GS_OK;
}
int gs_pose_forward(const GsPoseArgs* a, float* rots, float* Jtrs, float* bone_transforms, float* loss_pose, float* state,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = pose_validate(a)) return rc;
    if (!required(a->v_template, 4) || !required(a->shapedirs, 4) || !required(a->J_template, 4) || !required(a->betas, 4) ||
        !required(a->trans, 4) || !required(rots, 4) || !required(Jtrs, 4) || !required(bone_transforms, 4) || !required(state, 4) ||
        !aligned(loss_pose, 4) || (a->rots_gt && !loss_pose))
        return GS_E_BAD_ARG;
    if (!required(workspace, 8)) return GS_E_BAD_ARG;
    if (workspace_bytes < pose_workspace_bytes(a->V)) return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_pose_forward(a, rots, Jtrs, bone_transforms, loss_pose, state, workspace, (hipStream_t)stream);
}
int gs_pose_backward(const GsPoseArgs* a, const float* state, const float* dL_drots, const float* dL_dJtrs,
                     const float* dL_dbone_transforms, const float* dL_dloss_pose, float* dL_dbetas, float* dL_droot_orient,
                     float* dL_dpose_body, float* dL_dpose_hand, float* dL_dtrans, void* stream) {
    if (const int rc = pose_validate(a)) return rc;
    if (!required(state, 4) || !aligned(dL_drots, 4) || !aligned(dL_dJtrs, 4) || !aligned(dL_dbone_transforms, 4) ||
        !aligned(dL_dloss_pose, 4) || !aligned(dL_dbetas, 4) || !aligned(dL_droot_orient, 4) || !aligned(dL_dpose_body, 4) ||
        !aligned(dL_dpose_hand, 4) || !aligned(dL_dtrans, 4))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_dbetas && !dL_droot_orient && !dL_dpose_body && !dL_dpose_hand && !dL_dtrans) return GS_OK;
    return launch_pose_backward(a, state, dL_drots, dL_dJtrs, dL_dbone_transforms, dL_dloss_pose, dL_dbetas, dL_droot_orient,
                                dL_dpose_body, dL_dpose_hand, dL_dtrans, (hipStream_t)stream);
}

}  // extern "C"
