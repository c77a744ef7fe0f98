// nonrigid.hip -- the two torch parts of the non-rigid deformer (models/deformer/non_rigid.py MLP.forward :55-131 and
// HashGridwithMLP.forward :226-300) either side of its MLP: the hierarchical pose encoder in front of it
// (models/network_utils.py HierarchicalPoseEncoder.forward :151-180) and the application of the MLP's output to the
// Gaussians behind it, each as one forward launch and one backward launch (the regularisers add one small final sum),
// instead of well over a hundred dependent launches for ~25 kFLOP and ~15 memory-bound launches over N rows whose
// backward materialises four zero (N, 10 + F) tensors.
//
// Spec 1, the pose encoder (batch 1, 24 joints, rel_joints = False, d = dim_per_joint in 1..GS_POSE_ENC_MAX_DIM, m = 13 + d;
// fp32 throughout; nn.Linear layouts: W (out, in) row-major):
//   g      = W0 [rots (216) | Jtrs (72)] + b0                                                      (d values)
//   for j = 0..23 in index order (p = parents[j] < j; entry 0 is ignored):
//   in_j   = [rots_j (9) | Jtrs_j (3) | |Jtrs_j - Jtrs_p| (root: |Jtrs_0|) | out_p (root: g)]         (m values)
//   h_j    = relu(W1_j in_j + b1_j)  (m),   out_j = W2_j h_j + b2_j  (d)
//   output = (out_0 | ... | out_23), (1, 24 d).
// Backward from dL/doutput, the tree in reverse: dout_j = its slice + sum over the children c of j, c ascending, of
//   din_c[13:]; dh_j = W2_j^T dout_j; dpre_j = dh_j where h_j > 0, else 0 (torch's ReLU: 0 at a pre-activation <= 0);
//   din_j = W1_j^T dpre_j; dW2_j = dout_j h_j^T, db2_j = dout_j, dW1_j = dpre_j in_j^T, db1_j = dpre_j; dg = din_0[13:],
//   dW0 = dg x^T, db0 = dg, dx = W0^T dg.  drots_j = din_j[0:9] + dx.  dJtrs_j = din_j[9:12] (direct) + u_j - sum over
//   the children c of j, c ascending, of u_c (bone length; u_j = (Jtrs_j - Jtrs_p) din_j[12] / |Jtrs_j - Jtrs_p|, and 0
//   at a zero-length bone as torch's norm has it: no NaN) + dx (layer 0), added in this order.  Every dot product runs
//   over its index ascending from the first term.
//   The 98 parameter tensors are read through their own addresses, passed by value in GsPoseEncArgs (no pointer table
//   in device memory, nothing to upload or to invalidate under capture); their gradients go to one packed buffer
//   W0 | b0 | (W1_j | b1_j | W2_j | b2_j), j = 0..23.
// Kernels: one workgroup of ENC_THREADS threads each.  Thread t owns one row of W1 (joint t / m, row t % m) and one row
//   of W2 (forward), or one column of each (backward), and loads it into registers before the walk starts: every weight
//   is read once, all loads are in flight together, and the walk itself touches LDS only.  Joints of one tree depth run
//   side by side between two barriers; a row's sum is one thread's, so the result does not depend on that.
//   `state` (GS_POSE_ENC_STATE_FLOATS) carries in_j and h_j (stride 29) to the backward.
//
// Spec 2, the delta application (per row n of deltas (N, D), D = 10 + F; dx = deltas[0:3], ds = deltas[3:6],
// dr = deltas[6:10]):
//   xyz'      = xyz + dx
//   scaling'  = scaling + ds (GS_NR_SCALE_LOGIT) | log(max(exp(scaling) + ds, 1e-6)) (GS_NR_SCALE_EXP; the clamp passes
//               gradient where its argument is >= 1e-6) | scaling with ds taken as 0 (GS_NR_SCALE_ZERO)
//   rotation' = rotation + dr (GS_NR_ROT_ADD) | (1, dr1, dr2, dr3) (x) rotation (GS_NR_ROT_MULT: the Hamilton product, real
//               part first, unnormalised -- utils/general_utils.py quaternion_multiply :184-192)
//   feature   = deltas[10:], a contiguous (N, F) array of its own
//   nr_xyz = mean_n |dx|_2, nr_scale = mean_n |ds|_1, nr_rot = mean_n |dr|_1 (ADD) or |dr[1:]|_1 (MULT); the L2 norm's
//   gradient is 0 at a zero row and sign(0) = 0.
//   Deliberate difference: in MULT mode the reference writes 1 into column 6 of the MLP's output in place; here
//   `deltas` is never written.
// Backward, per row, from the upstream gradients of xyz', scaling', rotation', feature and the three scalars (device
//   floats), any of them absent = 0: dL/ddeltas (N, D) is written whole in one pass, zeros included (column 6 in MULT,
//   columns 3:6 in ZERO, the feature columns without an upstream feature gradient); dL/dscaling and dL/drotation.
//   dL/dxyz is the upstream gradient of xyz' itself and is not written.
// Kernels (NR_THREADS threads): a workgroup owns R = nr_rows(D) consecutive rows, R a multiple of 4 with R D <=
//   NR_LDS_FLOATS: its rows of deltas are one contiguous slab that starts 16-byte aligned (rows themselves, 40 + 4 F
//   bytes, generally do not), moved between global memory and LDS with 16-byte accesses; so is its slab of feature.
//   nr_apply_fwd   slab -> LDS; one thread per row reads the ten head columns from LDS and writes xyz', scaling',
//                  rotation'; all threads gather the feature columns from LDS into 16-byte stores; the three norms are
//                  summed over the block (block_sum, waves in order: ordered_sum.h) into partial[3][blocks].
//   (final)        three workgroups, one per regulariser, add the block partials: ordered_final_kernel (ordered_sum.h),
//                  waves in order, times 1 / N.
//   nr_apply_bwd   builds the block's slab of dL/ddeltas in LDS (head columns by the row's thread, feature columns
//                  scattered from 16-byte loads of the upstream feature slab) and stores it with 16-byte accesses.  The
//                  ten head columns of deltas are read from global memory directly (40 bytes a row).
// No atomics, no memsets, no host synchronisation: every output and gradient is bitwise reproducible and the calls are
// capture-safe.
#include "common.h"
#include "boundary.h"
#include "ordered_sum.h"
#include "slab.h"

// ---------------------------------------------------------------------------------------------
// 1. the pose encoder
// ---------------------------------------------------------------------------------------------
#define ENC_J GS_POSE_ENC_JOINTS
#define ENC_MAXD GS_POSE_ENC_MAX_DIM
#define ENC_MAXM (13 + ENC_MAXD)
#define ENC_X (12 * ENC_J)  // rots (216) | Jtrs (72)
#define ENC_THREADS 1024
#define ENC_L0_LANES 32     // threads per output of layer 0, nine inputs each
#define ENC_ST_IN 0
#define ENC_ST_H (ENC_J * ENC_MAXM)
static_assert(2 * ENC_J * ENC_MAXM == GS_POSE_ENC_STATE_FLOATS, "state layout");
static_assert(ENC_J * ENC_MAXM <= ENC_THREADS && ENC_MAXD * ENC_L0_LANES <= ENC_THREADS, "one thread per row");
static_assert(ENC_L0_LANES * 9 == ENC_X, "layer 0 split");

static size_t pose_encoder_grad_floats(int d) {
    const size_t m = 13 + (size_t)d;
    return (size_t)ENC_X * d + d + ENC_J * (m * m + m + d * m + d);
}

// parents and tree depths into LDS (thread 0; parents[j] < j)
__device__ __forceinline__ void enc_tree(const GsPoseEncArgs& a, int* s_par, int* s_depth, int* s_maxd) {
    if (threadIdx.x == 0) {
        s_par[0] = 0;
        s_depth[0] = 0;
        int mx = 0;
        for (int j = 1; j < ENC_J; j++) {
            const int p = a.parents[j];
            s_par[j] = p;
            s_depth[j] = s_depth[p] + 1;
            mx = max(mx, s_depth[j]);
        }
        *s_maxd = mx;
    }
}

__global__ __launch_bounds__(ENC_THREADS) void pose_enc_fwd_kernel(GsPoseEncArgs a, float* __restrict__ out,
                                                                   float* __restrict__ state) {
    __shared__ float s_x[ENC_X], s_len[ENC_J], s_g[ENC_MAXD], s_out[ENC_J * ENC_MAXD], s_h[ENC_J * ENC_MAXM];
    __shared__ float s_p0[ENC_MAXD * ENC_L0_LANES];
    __shared__ int s_par[ENC_J], s_depth[ENC_J], s_maxd;
    const int t = threadIdx.x, d = a.d, m = 13 + d;
    // this thread's rows, in registers before anything depends on anything
    const int j1 = t / m, r1 = t - j1 * m, j2 = t / d, r2 = t - j2 * d;
    const bool own1 = t < ENC_J * m, own2 = t < ENC_J * d;
    float w1[ENC_MAXM], w2[ENC_MAXM], bias1 = 0.0f, bias2 = 0.0f;
    {
        const float* W = own1 ? a.W1[j1] + r1 * m : nullptr;
#pragma unroll
        for (int k = 0; k < ENC_MAXM; k++) w1[k] = (own1 && k < m) ? W[k] : 0.0f;
        if (own1) bias1 = a.b1[j1][r1];
        const float* V = own2 ? a.W2[j2] + r2 * m : nullptr;
#pragma unroll
        for (int k = 0; k < ENC_MAXM; k++) w2[k] = (own2 && k < m) ? V[k] : 0.0f;
        if (own2) bias2 = a.b2[j2][r2];
    }
    const int r0 = t / ENC_L0_LANES, c0 = t % ENC_L0_LANES;
    float w0[9];
#pragma unroll
    for (int k = 0; k < 9; k++) w0[k] = r0 < d ? a.W0[r0 * ENC_X + 9 * c0 + k] : 0.0f;
    if (t < ENC_X) s_x[t] = t < 9 * ENC_J ? a.rots[t] : a.Jtrs[t - 9 * ENC_J];
    enc_tree(a, s_par, s_depth, &s_maxd);
    __syncthreads();
    if (r0 < d) {  // layer 0: nine inputs per thread, then the 32 runs in order
        float p = w0[0] * s_x[9 * c0];
#pragma unroll
        for (int k = 1; k < 9; k++) p += w0[k] * s_x[9 * c0 + k];
        s_p0[r0 * ENC_L0_LANES + c0] = p;
    }
    if (t < ENC_J) {
        const float* J = s_x + 9 * ENC_J;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = t == 0 ? J[c] : J[3 * t + c] - J[3 * s_par[t] + c];
        s_len[t] = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    }
    __syncthreads();
    if (t < d) {
        float g = a.b0[t];
        for (int c = 0; c < ENC_L0_LANES; c++) g += s_p0[t * ENC_L0_LANES + c];
        s_g[t] = g;
    }
    __syncthreads();
    const int maxd = s_maxd;
    const int dep1 = own1 ? s_depth[j1] : -1, dep2 = own2 ? s_depth[j2] : -1;
    for (int lvl = 0; lvl <= maxd; lvl++) {
        if (dep1 == lvl) {
            const float* up = j1 == 0 ? s_g : s_out + s_par[j1] * ENC_MAXD;
            float acc = bias1, mine = 0.0f;
#pragma unroll
            for (int k = 0; k < ENC_MAXM; k++) {
                if (k < m) {
                    const float x = k < 9 ? s_x[9 * j1 + k] : k < 12 ? s_x[9 * ENC_J + 3 * j1 + (k - 9)] : k == 12 ? s_len[j1] : up[k - 13];
                    acc += w1[k] * x;
                    if (k == r1) mine = x;
                }
            }
            const float h = acc <= 0.0f ? 0.0f : acc;
            s_h[j1 * ENC_MAXM + r1] = h;
            state[ENC_ST_H + j1 * ENC_MAXM + r1] = h;
            state[ENC_ST_IN + j1 * ENC_MAXM + r1] = mine;
        }
        __syncthreads();
        if (dep2 == lvl) {
            float acc = bias2;
#pragma unroll
            for (int k = 0; k < ENC_MAXM; k++)
                if (k < m) acc += w2[k] * s_h[j2 * ENC_MAXM + k];
            s_out[j2 * ENC_MAXD + r2] = acc;
            out[j2 * d + r2] = acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ENC_THREADS) void pose_enc_bwd_kernel(GsPoseEncArgs a, const float* __restrict__ state,
                                                                   const float* __restrict__ g_out, float* __restrict__ dparams,
                                                                   float* __restrict__ drots, float* __restrict__ dJtrs) {
    __shared__ float s_in[ENC_J * ENC_MAXM], s_h[ENC_J * ENC_MAXM], s_dpre[ENC_J * ENC_MAXM], s_din[ENC_J * ENC_MAXM];
    __shared__ float s_dout[ENC_J * ENC_MAXD], s_dx[ENC_X], s_u[ENC_J * 3];
    __shared__ int s_par[ENC_J], s_depth[ENC_J], s_maxd;
    const int t = threadIdx.x, d = a.d, m = 13 + d;
    // this thread's columns of W2_j and W1_j (joint t / m, column t % m), and of W0 (column t)
    const int j = t / m, k = t - j * m;
    const bool own = t < ENC_J * m;
    float w2c[ENC_MAXD], w1c[ENC_MAXM], w0c[ENC_MAXD];
    {
        const float* V = own ? a.W2[j] + k : nullptr;
#pragma unroll
        for (int r = 0; r < ENC_MAXD; r++) w2c[r] = (own && r < d) ? V[r * m] : 0.0f;
        const float* W = own ? a.W1[j] + k : nullptr;
#pragma unroll
        for (int r = 0; r < ENC_MAXM; r++) w1c[r] = (own && r < m) ? W[r * m] : 0.0f;
#pragma unroll
        for (int r = 0; r < ENC_MAXD; r++) w0c[r] = (t < ENC_X && r < d) ? a.W0[r * ENC_X + t] : 0.0f;
    }
    if (t < ENC_J * ENC_MAXM) {
        s_in[t] = state[ENC_ST_IN + t];
        s_h[t] = state[ENC_ST_H + t];
    }
    enc_tree(a, s_par, s_depth, &s_maxd);
    __syncthreads();
    const int maxd = s_maxd, dep = own ? s_depth[j] : -1;
    for (int lvl = maxd; lvl >= 0; lvl--) {  // the children of a joint are one level deeper: done before it
        if (dep == lvl && k < d) {
            float acc = g_out[j * d + k];
            for (int c = j + 1; c < ENC_J; c++)
                if (s_par[c] == j) acc += s_din[c * ENC_MAXM + 13 + k];
            s_dout[j * ENC_MAXD + k] = acc;
        }
        __syncthreads();
        if (dep == lvl) {
            float dh = w2c[0] * s_dout[j * ENC_MAXD];
#pragma unroll
            for (int r = 1; r < ENC_MAXD; r++)
                if (r < d) dh += w2c[r] * s_dout[j * ENC_MAXD + r];
            s_dpre[j * ENC_MAXM + k] = s_h[j * ENC_MAXM + k] > 0.0f ? dh : 0.0f;
        }
        __syncthreads();
        if (dep == lvl) {
            float di = w1c[0] * s_dpre[j * ENC_MAXM];
#pragma unroll
            for (int r = 1; r < ENC_MAXM; r++)
                if (r < m) di += w1c[r] * s_dpre[j * ENC_MAXM + r];
            s_din[j * ENC_MAXM + k] = di;
        }
        __syncthreads();
    }
    const float* dg = s_din + 13;  // of the root
    if (t < ENC_X) {
        float acc = w0c[0] * dg[0];
#pragma unroll
        for (int r = 1; r < ENC_MAXD; r++)
            if (r < d) acc += w0c[r] * dg[r];
        s_dx[t] = acc;
    }
    if (t < ENC_J) {  // the bone-length term of joint t
        const float len = s_in[t * ENC_MAXM + 12], dl = s_din[t * ENC_MAXM + 12];
        const float s = len > 0.0f ? dl / len : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = t == 0 ? s_in[9 + c] : s_in[t * ENC_MAXM + 9 + c] - s_in[s_par[t] * ENC_MAXM + 9 + c];
            s_u[3 * t + c] = len > 0.0f ? v * s : 0.0f;
        }
    }
    __syncthreads();
    if (drots && t < 9 * ENC_J) drots[t] = s_din[(t / 9) * ENC_MAXM + t % 9] + s_dx[t];
    if (dJtrs && t < 3 * ENC_J) {
        const int jj = t / 3, c = t % 3;
        float acc = s_din[jj * ENC_MAXM + 9 + c];
        acc += s_u[3 * jj + c];
        for (int ch = jj + 1; ch < ENC_J; ch++)
            if (s_par[ch] == jj) acc -= s_u[3 * ch + c];
        acc += s_dx[9 * ENC_J + t];
        dJtrs[t] = acc;
    }
    if (dparams) {  // the outer products, element by element of the packed buffer
        const int P0 = ENC_X * d, mm = m * m, B = mm + m + d * m + d, total = P0 + d + ENC_J * B;
        for (int e = t; e < total; e += ENC_THREADS) {
            float v;
            if (e < P0) {
                const int r = e / ENC_X, x = e - r * ENC_X;
                const float xv = x < 9 * ENC_J ? s_in[(x / 9) * ENC_MAXM + x % 9]
                                               : s_in[((x - 9 * ENC_J) / 3) * ENC_MAXM + 9 + (x - 9 * ENC_J) % 3];
                v = dg[r] * xv;
            } else if (e < P0 + d) {
                v = dg[e - P0];
            } else {
                const int q = e - P0 - d, jj = q / B;
                int o = q - jj * B;
                if (o < mm) {
                    v = s_dpre[jj * ENC_MAXM + o / m] * s_in[jj * ENC_MAXM + o % m];
                } else if ((o -= mm) < m) {
                    v = s_dpre[jj * ENC_MAXM + o];
                } else if ((o -= m) < d * m) {
                    v = s_dout[jj * ENC_MAXD + o / m] * s_h[jj * ENC_MAXM + o % m];
                } else {
                    v = s_dout[jj * ENC_MAXD + (o - d * m)];
                }
            }
            dparams[e] = v;
        }
    }
}

static int launch_pose_encoder_forward(const GsPoseEncArgs* a, float* out, float* state, hipStream_t s) {
    StageScope st("pose_encoder", s);
    hipLaunchKernelGGL(pose_enc_fwd_kernel, dim3(1), dim3(ENC_THREADS), 0, s, *a, out, state);
    GS_LAUNCH_CHECK("pose_encoder", 0, s);
    return GS_OK;
}
static int launch_pose_encoder_backward(const GsPoseEncArgs* a, const float* state, const float* g_out, float* dparams, float* drots,
                                        float* dJtrs, hipStream_t s) {
    StageScope st("pose_encoder_bwd", s);
    hipLaunchKernelGGL(pose_enc_bwd_kernel, dim3(1), dim3(ENC_THREADS), 0, s, *a, state, g_out, dparams, drots, dJtrs);
    GS_LAUNCH_CHECK("pose_encoder_bwd", 0, s);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------
// 2. the delta application
// ---------------------------------------------------------------------------------------------
#define NR_THREADS 256
#define NR_LDS_FLOATS 8192  // 32 KiB: the block's slab of deltas
static_assert(NR_LDS_FLOATS / GS_NONRIGID_MAX_D >= 4, "a block holds at least four rows");

// rows per workgroup: a multiple of 4 (every slab then starts 16-byte aligned), at most one per thread
static inline int nr_rows(int D) {
    const int r = (NR_LDS_FLOATS / D) & ~3;
    return r < NR_THREADS ? r : NR_THREADS;
}
static inline int nr_blocks(int N, int D) {
    const int R = nr_rows(D);
    return (N + R - 1) / R;
}
static size_t nonrigid_workspace_bytes(int N, int D) { return (size_t)3 * nr_blocks(N, D) * sizeof(float); }

__device__ __forceinline__ float nr_sign(float x) { return x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f; }

__global__ __launch_bounds__(NR_THREADS) void nr_apply_fwd_kernel(int N, int D, int R, int smode, int rmode,
                                                                  const float* __restrict__ deltas, const float* __restrict__ xyz,
                                                                  const float* __restrict__ scaling, const float* __restrict__ rot,
                                                                  float* __restrict__ xyz_o, float* __restrict__ scal_o,
                                                                  float* __restrict__ rot_o, float* __restrict__ feat,
                                                                  float* __restrict__ partial) {
    __shared__ float4 buf4[NR_LDS_FLOATS / 4];
    __shared__ float s_red[3][NR_THREADS / 64];
    float* buf = reinterpret_cast<float*>(buf4);
    const int t = threadIdx.x, F = D - 10;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int n = (int)min((size_t)R, (size_t)N - row0);
    slab_load<NR_THREADS>(deltas + row0 * D, n * D, buf);
    __syncthreads();
    float lx = 0.0f, ls = 0.0f, lr = 0.0f;
    if (t < n) {
        const size_t i = row0 + t;
        float dl[10];
#pragma unroll
        for (int c = 0; c < 10; c++) dl[c] = buf[t * D + c];
#pragma unroll
        for (int c = 0; c < 3; c++) xyz_o[3 * i + c] = xyz[3 * i + c] + dl[c];
        lx = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
        if (scal_o) {  // (ZERO: a copy, for a caller that wants one)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float s = scaling[3 * i + c];
                scal_o[3 * i + c] = smode == GS_NR_SCALE_LOGIT ? s + dl[3 + c]
                                    : smode == GS_NR_SCALE_EXP ? logf(fmaxf(expf(s) + dl[3 + c], 1e-6f)) : s;
            }
        }
        if (smode != GS_NR_SCALE_ZERO) ls = fabsf(dl[3]) + fabsf(dl[4]) + fabsf(dl[5]);
        const float4 q = reinterpret_cast<const float4*>(rot)[i];
        float4 o;
        if (rmode == GS_NR_ROT_ADD) {
            o = make_float4(q.x + dl[6], q.y + dl[7], q.z + dl[8], q.w + dl[9]);
            lr = fabsf(dl[6]) + fabsf(dl[7]) + fabsf(dl[8]) + fabsf(dl[9]);
        } else {  // (1, r1, r2, r3) (x) (s0, s1, s2, s3)
            const float r1 = dl[7], r2 = dl[8], r3 = dl[9], s0 = q.x, s1 = q.y, s2 = q.z, s3 = q.w;
            o.x = s0 - r1 * s1 - r2 * s2 - r3 * s3;
            o.y = s1 + r1 * s0 - r2 * s3 + r3 * s2;
            o.z = s2 + r1 * s3 + r2 * s0 - r3 * s1;
            o.w = s3 - r1 * s2 + r2 * s1 + r3 * s0;
            lr = fabsf(r1) + fabsf(r2) + fabsf(r3);
        }
        reinterpret_cast<float4*>(rot_o)[i] = o;
    }
    if (F > 0) {  // (uniform) feature[r][c] = slab[r D + 10 + c], four outputs per store
        const size_t foff = row0 * F;
        const int total = n * F, n4 = total >> 2;
        float4* o4 = reinterpret_cast<float4*>(feat + foff);
        for (int k = t; k < n4; k += NR_THREADS) {
            int r = (4 * k) / F, c = 4 * k - r * F;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                v[u] = buf[r * D + 10 + c];
                if (++c == F) {
                    c = 0;
                    r++;
                }
            }
            o4[k] = make_float4(v[0], v[1], v[2], v[3]);
        }
        for (int f = 4 * n4 + t; f < total; f += NR_THREADS) feat[foff + f] = buf[(f / F) * D + 10 + f % F];
    }
    if (partial) {  // (uniform; every lane takes part in the sums: the rows past n add zeros)
        const float sums[3] = {block_sum<NR_THREADS, WavesInOrder>(lx, s_red[0]), block_sum<NR_THREADS, WavesInOrder>(ls, s_red[1]),
                               block_sum<NR_THREADS, WavesInOrder>(lr, s_red[2])};
        if (t == 0)
            for (int q = 0; q < 3; q++) partial[(size_t)q * gridDim.x + blockIdx.x] = sums[q];
    }
}

__global__ __launch_bounds__(NR_THREADS) void nr_apply_bwd_kernel(int N, int D, int R, int smode, int rmode, float inv_n,
                                                                  const float* __restrict__ deltas, const float* __restrict__ scaling,
                                                                  const float* __restrict__ rot, const float* __restrict__ g_xyz,
                                                                  const float* __restrict__ g_scal, const float* __restrict__ g_rot,
                                                                  const float* __restrict__ g_feat, const float* __restrict__ g_nrx,
                                                                  const float* __restrict__ g_nrs, const float* __restrict__ g_nrr,
                                                                  float* __restrict__ ddeltas, float* __restrict__ dscal,
                                                                  float* __restrict__ drot) {
    __shared__ float4 buf4[NR_LDS_FLOATS / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    const int t = threadIdx.x, F = D - 10;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int n = (int)min((size_t)R, (size_t)N - row0);
    if (ddeltas && F > 0) {  // (uniform) the feature columns of the slab
        const int total = n * F, n4 = total >> 2;
        if (g_feat) {
            const size_t foff = row0 * F;
            const float4* g4 = reinterpret_cast<const float4*>(g_feat + foff);
            for (int k = t; k < n4; k += NR_THREADS) {
                const float4 v4 = g4[k];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                int r = (4 * k) / F, c = 4 * k - r * F;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    buf[r * D + 10 + c] = v[u];
                    if (++c == F) {
                        c = 0;
                        r++;
                    }
                }
            }
            for (int f = 4 * n4 + t; f < total; f += NR_THREADS) buf[(f / F) * D + 10 + f % F] = g_feat[foff + f];
        } else {
            for (int f = t; f < total; f += NR_THREADS) buf[(f / F) * D + 10 + f % F] = 0.0f;
        }
    }
    if (t < n) {
        const size_t i = row0 + t;
        const float* dr = deltas + i * D;
        float dl[10], dd[10];
#pragma unroll
        for (int c = 0; c < 10; c++) dl[c] = dr[c];
        const float wx = g_nrx ? g_nrx[0] * inv_n : 0.0f, wsc = g_nrs ? g_nrs[0] * inv_n : 0.0f, wr = g_nrr ? g_nrr[0] * inv_n : 0.0f;
        {
            const float nrm = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
            const float s = nrm > 0.0f ? wx / nrm : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) dd[c] = (g_xyz ? g_xyz[3 * i + c] : 0.0f) + (nrm > 0.0f ? dl[c] * s : 0.0f);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float g = g_scal ? g_scal[3 * i + c] : 0.0f;
            if (smode == GS_NR_SCALE_LOGIT) {
                dd[3 + c] = g + wsc * nr_sign(dl[3 + c]);
                if (dscal) dscal[3 * i + c] = g;
            } else if (smode == GS_NR_SCALE_EXP) {
                const float e = expf(scaling[3 * i + c]), arg = e + dl[3 + c];
                const float ga = arg >= 1e-6f ? g / arg : 0.0f;  // through log and the clamp
                dd[3 + c] = ga + wsc * nr_sign(dl[3 + c]);
                if (dscal) dscal[3 * i + c] = ga * e;
            } else {
                dd[3 + c] = 0.0f;
                if (dscal) dscal[3 * i + c] = g;
            }
        }
        const float4 g = g_rot ? reinterpret_cast<const float4*>(g_rot)[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (rmode == GS_NR_ROT_ADD) {
            dd[6] = g.x + wr * nr_sign(dl[6]);
            dd[7] = g.y + wr * nr_sign(dl[7]);
            dd[8] = g.z + wr * nr_sign(dl[8]);
            dd[9] = g.w + wr * nr_sign(dl[9]);
            if (drot) reinterpret_cast<float4*>(drot)[i] = g;
        } else {
            const float4 q = reinterpret_cast<const float4*>(rot)[i];
            const float r1 = dl[7], r2 = dl[8], r3 = dl[9], s0 = q.x, s1 = q.y, s2 = q.z, s3 = q.w;
            dd[6] = 0.0f;
            dd[7] = (-g.x * s1 + g.y * s0 + g.z * s3 - g.w * s2) + wr * nr_sign(r1);
            dd[8] = (-g.x * s2 - g.y * s3 + g.z * s0 + g.w * s1) + wr * nr_sign(r2);
            dd[9] = (-g.x * s3 + g.y * s2 - g.z * s1 + g.w * s0) + wr * nr_sign(r3);
            if (drot)
                reinterpret_cast<float4*>(drot)[i] = make_float4(g.x + g.y * r1 + g.z * r2 + g.w * r3, -g.x * r1 + g.y - g.z * r3 + g.w * r2,
                                                                 -g.x * r2 + g.y * r3 + g.z - g.w * r1, -g.x * r3 - g.y * r2 + g.z * r1 + g.w);
        }
        if (ddeltas) {
#pragma unroll
            for (int c = 0; c < 10; c++) buf[t * D + c] = dd[c];
        }
    }
    if (ddeltas) {  // (uniform)
        __syncthreads();
        slab_store<NR_THREADS>(ddeltas + row0 * D, n * D, buf);
    }
}

// ---- launchers (the C ABI has checked every argument)
static int launch_nonrigid_apply_forward(int N, int D, int smode, int rmode, const float* deltas, const float* xyz, const float* scaling,
                                         const float* rot, float* xyz_o, float* scal_o, float* rot_o, float* feat, float* losses,
                                         void* workspace, hipStream_t s) {
    StageScope st("nonrigid_apply", s);
    const int nb = nr_blocks(N, D);
    float* partial = losses ? reinterpret_cast<float*>(workspace) : nullptr;
    hipLaunchKernelGGL(nr_apply_fwd_kernel, dim3(nb), dim3(NR_THREADS), 0, s, N, D, nr_rows(D), smode, rmode, deltas, xyz, scaling,
                       rot, xyz_o, scal_o, rot_o, feat, partial);
    GS_LAUNCH_CHECK("nonrigid_apply", 0, s);
    if (losses) {
        hipLaunchKernelGGL((ordered_final_kernel<NR_THREADS, WavesInOrder, true>), dim3(3), dim3(NR_THREADS), 0, s,
                           (const float*)partial, nb, 1.0f / (float)N, losses);
        GS_LAUNCH_CHECK("nonrigid_final", 0, s);
    }
    return GS_OK;
}
static int launch_nonrigid_apply_backward(int N, int D, int smode, int rmode, const float* deltas, const float* scaling, const float* rot,
                                          const float* g_xyz, const float* g_scal, const float* g_rot, const float* g_feat,
                                          const float* g_nrx, const float* g_nrs, const float* g_nrr, float* ddeltas, float* dscal,
                                          float* drot, hipStream_t s) {
    StageScope st("nonrigid_apply_bwd", s);
    hipLaunchKernelGGL(nr_apply_bwd_kernel, dim3(nr_blocks(N, D)), dim3(NR_THREADS), 0, s, N, D, nr_rows(D), smode, rmode,
                       1.0f / (float)N, deltas, scaling, rot, g_xyz, g_scal, g_rot, g_feat, g_nrx, g_nrs, g_nrr, ddeltas, dscal,
                       drot);
    GS_LAUNCH_CHECK("nonrigid_apply_bwd", 0, s);
    return GS_OK;
}

extern "C" {

static int pose_enc_validate(const GsPoseEncArgs* a) {
    if (!a || a->d < 1 || a->d > GS_POSE_ENC_MAX_DIM) return GS_E_BAD_ARG;
    for (int i = 1; i < GS_POSE_ENC_JOINTS; i++)
        if (a->parents[i] < 0 || a->parents[i] >= i) return GS_E_BAD_ARG;
    if (!required(a->W0, 4)) return GS_E_BAD_ARG;
    for (int j = 0; j < GS_POSE_ENC_JOINTS; j++)
        if (!required(a->W1[j], 4) || !required(a->W2[j], 4)) return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_pose_encoder_grad_floats(int32_t d, size_t* out) {
    if (!out || d < 1 || d > GS_POSE_ENC_MAX_DIM) return GS_E_BAD_ARG;
    *out = pose_encoder_grad_floats(d);
    return GS_OK;
}
int gs_pose_encoder_forward(const GsPoseEncArgs* a, float* out, float* state, void* stream) {
    if (const int rc = pose_enc_validate(a)) return rc;
    if (!required(a->rots, 4) || !required(a->Jtrs, 4) || !required(a->b0, 4) || !required(out, 4) || !required(state, 4))
        return GS_E_BAD_ARG;
    for (int j = 0; j < GS_POSE_ENC_JOINTS; j++)
        if (!required(a->b1[j], 4) || !required(a->b2[j], 4)) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_pose_encoder_forward(a, out, state, (hipStream_t)stream);
}
int gs_pose_encoder_backward(const GsPoseEncArgs* a, const float* state, const float* dL_dout, float* dL_dparams,
                             float* dL_drots, float* dL_dJtrs, void* stream) {
    if (const int rc = pose_enc_validate(a)) return rc;
    if (!required(state, 4) || !required(dL_dout, 4) || !aligned(dL_dparams, 4) || !aligned(dL_drots, 4) || !aligned(dL_dJtrs, 4))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_dparams && !dL_drots && !dL_dJtrs) return GS_OK;
    return launch_pose_encoder_backward(a, state, dL_dout, dL_dparams, dL_drots, dL_dJtrs, (hipStream_t)stream);
}
static bool nr_shape_ok(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset) {
    return N >= 0 && D >= 10 && D <= GS_NONRIGID_MAX_D &&
           (scale_offset == GS_NR_SCALE_LOGIT || scale_offset == GS_NR_SCALE_EXP || scale_offset == GS_NR_SCALE_ZERO) &&
           (rot_offset == GS_NR_ROT_ADD || rot_offset == GS_NR_ROT_MULT);
}
int gs_nonrigid_workspace_bytes(int32_t N, int32_t D, size_t* out) {
    if (!out || N < 0 || D < 10 || D > GS_NONRIGID_MAX_D) return GS_E_BAD_ARG;
    *out = nonrigid_workspace_bytes(N, D);
    return GS_OK;
}
int gs_nonrigid_apply_forward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                              const float* xyz, const float* scaling, const float* rotation, float* xyz_out,
                              float* scaling_out, float* rotation_out, float* feature, float* losses, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!nr_shape_ok(N, D, scale_offset, rot_offset)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!deltas || !xyz || !rotation || !xyz_out || !rotation_out || (D > 10 && !feature)) return GS_E_BAD_ARG;
    if (scale_offset != GS_NR_SCALE_ZERO && (!scaling || !scaling_out)) return GS_E_BAD_ARG;
    if (scaling_out && !scaling) return GS_E_BAD_ARG;
    if (!aligned(deltas, 16) || !aligned(rotation, 16) || !aligned(rotation_out, 16) || !aligned(feature, 16) || !aligned(xyz, 4) ||
        !aligned(scaling, 4) || !aligned(xyz_out, 4) || !aligned(scaling_out, 4) || !aligned(losses, 4))
        return GS_E_BAD_ARG;
    if (losses) {
        if (!required(workspace, 4)) return GS_E_BAD_ARG;
        if (workspace_bytes < nonrigid_workspace_bytes(N, D)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    return launch_nonrigid_apply_forward(N, D, scale_offset, rot_offset, deltas, xyz, scaling, rotation, xyz_out, scaling_out,
                                         rotation_out, D > 10 ? feature : nullptr, losses, workspace, (hipStream_t)stream);
}
int gs_nonrigid_apply_backward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                               const float* scaling, const float* rotation, const float* dL_dxyz_out,
                               const float* dL_dscaling_out, const float* dL_drotation_out, const float* dL_dfeature,
                               const float* dL_dnr_xyz, const float* dL_dnr_scale, const float* dL_dnr_rot,
                               float* dL_ddeltas, float* dL_dscaling, float* dL_drotation, void* stream) {
    if (!nr_shape_ok(N, D, scale_offset, rot_offset)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!deltas || (scale_offset == GS_NR_SCALE_EXP && !scaling) || (rot_offset == GS_NR_ROT_MULT && !rotation)) return GS_E_BAD_ARG;
    if (!aligned(deltas, 16) || !aligned(rotation, 16) || !aligned(dL_drotation_out, 16) || !aligned(dL_dfeature, 16) ||
        !aligned(dL_ddeltas, 16) || !aligned(dL_drotation, 16) || !aligned(scaling, 4) || !aligned(dL_dxyz_out, 4) ||
        !aligned(dL_dscaling_out, 4) || !aligned(dL_dnr_xyz, 4) || !aligned(dL_dnr_scale, 4) || !aligned(dL_dnr_rot, 4) ||
        !aligned(dL_dscaling, 4))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_ddeltas && !dL_dscaling && !dL_drotation) return GS_OK;
    return launch_nonrigid_apply_backward(N, D, scale_offset, rot_offset, deltas, scaling, rotation, dL_dxyz_out, dL_dscaling_out,
                                          dL_drotation_out, D > 10 ? dL_dfeature : nullptr, dL_dnr_xyz, dL_dnr_scale, dL_dnr_rot,
                                          dL_ddeltas, dL_dscaling, dL_drotation, (hipStream_t)stream);
}

}  // extern "C"
