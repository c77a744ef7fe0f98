// texture.hip -- the input of the ColorMLP texture (models/texture/texture.py ColorMLP.compose_input :74-118): the (N, D)
// matrix the colour MLP reads, as one forward launch and one backward launch (the latent code adds one small final sum),
// instead of several dozen dependent launches (get_features' cat, repeat, a batched 3x3 matmul, the view-noise matmul, a
// norm and a division, eval_sh_bases' fifteen indexed assignments, three cats that each copy the whole matrix again, an
// expand), about twice that in the autograd replay, and two host-to-device copies per step.  The MLP behind it stays a
// torch module.
//
// Spec (fp32 throughout; every array row-major and contiguous).  The columns of inp (N, D):
//   [ before_0 | .. | before_{B-1} | sh_embed | after_0 | .. | after_{A-1} | latent ],  B <= 6, A <= 2, D <= GS_TEXTURE_MAX_D
//   before_b (N, w), after_a (N, w): copied into place (the reference's features, xyz_norm / cov / normal; non_rigid_feature).
//   sh_embed: the (deg + 1)^2 - 1 real spherical-harmonics bases above the constant one at the unit view direction
//     (utils/sh_utils.py eval_sh_bases(deg, unit)[..., 1:]), deg in 0..4 (none at 0):
//       v = xyz - campos;  with fwd_transform: v = R^T v, R the 3x3 of the row's forward transform;  with a noise
//       matrix: v = v @ noise;  u = (x, y, z) = v / (|v| + 1e-12)                      (texture.py:90-101, as prepass.hip's view_dir)
//       l = 1:  -C1 y,  C1 z,  -C1 x                                                    C1 = sqrt(3 / (4 pi))
//       l = 2:  C2_0 xy, C2_1 yz, C2_2 (2 zz - xx - yy), C2_3 xz, C2_4 (xx - yy)        C2 = (1, -1, 1 / (2 sqrt 3), -1, 1 / 2) sqrt(15 / (4 pi))
//       l = 3:  C3_0 y (3 xx - yy), C3_1 xyz, C3_2 y (4 zz - xx - yy), C3_3 z (2 zz - 3 xx - 3 yy), C3_4 x (4 zz - xx - yy),
//               C3_5 z (xx - yy), C3_6 x (xx - 3 yy)                                    (gs_math.h SH_C3)
//       l = 4:  C4_0 xy (xx - yy), C4_1 yz (3 xx - yy), C4_2 xy (7 zz - 1), C4_3 yz (7 zz - 3), C4_4 (zz (35 zz - 30) + 3),
//               C4_5 xz (7 zz - 3), C4_6 (xx - yy) (7 zz - 1), C4_7 xz (xx - 3 yy), C4_8 (xx (xx - 3 yy) - yy (3 xx - yy))
//               C4 = (3/4 sqrt(35/pi), -3/4 sqrt(35/(2 pi)), 3/4 sqrt(5/pi), -3/4 sqrt(5/(2 pi)), 3/16 sqrt(1/pi),
//                     -3/4 sqrt(5/(2 pi)), 3/8 sqrt(5/pi), -3/4 sqrt(35/(2 pi)), 3/16 sqrt(35/pi))
//     (the degree-4 forms with 7 zz - 1 and 7 zz - 3 are harmonic on the unit sphere only; they are evaluated, and
//     differentiated, as the polynomials written here -- a row with xyz = campos has u = 0 and the bases of u = 0)
//   latent (Lt,): one row, broadcast to every row (Lt may be 0).
// Backward from g = dL/dinp (N, D):
//   dL/dbefore_b, dL/dafter_a: the block's columns of g, each as its own contiguous (N, w) array;
//   dL/dxyz (N, 3): du = sum_k g_k dB_k/du;  dv = du / (l + eps) - v (v . du) / (l (l + eps)^2), l = |v| (the second term 0
//     at l = 0, as torch's norm has it);  through the noise: dv = noise dv;  through R^T: dv = R dv;  dL/dxyz = dv;
//   dL/dlatent (Lt,): the column sums of g's latent columns over all rows.
//   fwd_transform, campos and the noise matrix take no gradient (the reference detaches T_fwd).  A gradient nobody asked
//   for is neither computed nor written (NULL).
// Kernels (TX_THREADS threads): a workgroup owns R = tx_rows(D) consecutive rows, R a multiple of 4 with R D <=
//   TX_LDS_FLOATS, at most one per thread: its rows of inp are one contiguous slab that starts 16-byte aligned for every
//   D (rows themselves, 4 D bytes, generally do not), and so is its slab of every block.
//   tx_input_fwd   the blocks' slabs are read with 16-byte loads and scattered into the slab of inp in LDS; one thread per
//                  row computes the direction and writes its bases there; the latent row is spread over the rows; the
//                  slab goes out with 16-byte stores.
//   tx_input_bwd   the slab of g comes into LDS with 16-byte loads; the wanted block gradients are gathered from it into
//                  16-byte stores; one thread per row reads its bases' gradients from LDS and writes dL/dxyz; the latent
//                  columns are summed over the block's rows (S = max(1, min(16, TX_THREADS / Lt)) interleaved runs per column, each
//                  in row order, then the runs in order) into partial[Lt][blocks].
//   (final)        one workgroup per latent column adds its block partials: ordered_final_kernel (ordered_sum.h), waves
//                  in order, no scale.
//   The partition of the rows into partials depends on N, D and Lt alone -- never on the device.  No atomics, no memsets, no
//   host synchronisation, no host memory traffic: every gradient is bitwise reproducible and the calls are capture-safe.
#include "common.h"
#include "boundary.h"
#include "gs_math.h"
#include "ordered_sum.h"
#include "slab.h"

#define TX_THREADS 256
#define TX_LDS_FLOATS 8192  // 32 KiB: the block's slab of inp
#define TX_MAX_SH 24        // (4 + 1)^2 - 1
#define TX_SEG_MAX 16       // interleaved runs per latent column inside a block
static_assert(TX_LDS_FLOATS / GS_TEXTURE_MAX_D >= 4, "a block holds at least four rows");
static_assert(GS_TEXTURE_MAX_D >= TX_THREADS, "s_part holds TX_SEG_MAX runs of a narrow latent code or one of the widest");

__device__ __constant__ static const float SH_C4[9] = {2.5033429417967046f, -1.7701307697799304f, 0.9461746957575601f,
                                                       -0.6690465435572892f, 0.10578554691520431f, -0.6690465435572892f,
                                                       0.47308734787878004f, -1.7701307697799304f, 0.6258357354491761f};

// rows per workgroup: a multiple of 4 (every slab then starts 16-byte aligned), at most one per thread
static inline int tx_rows(int D) {
    const int r = (TX_LDS_FLOATS / D) & ~3;
    return r < TX_THREADS ? r : TX_THREADS;
}
static inline int tx_blocks(int N, int D) {
    const int R = tx_rows(D);
    return (N + R - 1) / R;
}
static size_t texture_workspace_bytes(int N, int D, int latent_dim) {
    return (size_t)latent_dim * tx_blocks(N, D) * sizeof(float);
}
// the block gradients' addresses, passed to the backward kernel by value
struct TxGrads {
    float* before[GS_TEXTURE_MAX_BEFORE];
    float* after[GS_TEXTURE_MAX_AFTER];
};

// n rows of a contiguous (., w) block at src (16-byte aligned) -> columns [col, col + w) of the slab in LDS
__device__ __forceinline__ void tx_scatter(float* buf, int D, int col, const float* __restrict__ src, int n, int w) {
    const int t = threadIdx.x, total = n * w, n4 = total >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int k = t; k < n4; k += TX_THREADS) {
        const float4 v4 = s4[k];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        int r = (4 * k) / w, c = 4 * k - r * w;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            buf[r * D + col + c] = v[u];
            if (++c == w) {
                c = 0;
                r++;
            }
        }
    }
    for (int f = 4 * n4 + t; f < total; f += TX_THREADS) buf[(f / w) * D + col + f % w] = src[f];
}
// columns [col, col + w) of the slab in LDS -> n rows of a contiguous (., w) block at dst (16-byte aligned)
__device__ __forceinline__ void tx_gather(const float* buf, int D, int col, float* __restrict__ dst, int n, int w) {
    const int t = threadIdx.x, total = n * w, n4 = total >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int k = t; k < n4; k += TX_THREADS) {
        int r = (4 * k) / w, c = 4 * k - r * w;
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            v[u] = buf[r * D + col + c];
            if (++c == w) {
                c = 0;
                r++;
            }
        }
        d4[k] = make_float4(v[0], v[1], v[2], v[3]);
    }
    for (int f = 4 * n4 + t; f < total; f += TX_THREADS) dst[f] = buf[(f / w) * D + col + f % w];
}

__device__ __forceinline__ Mat3 tx_noise(const GsTextureArgs& a) {
    Mat3 m;
#pragma unroll
    for (int k = 0; k < 9; k++) m.m[k] = a.noise[k];
    return m;
}
__device__ __forceinline__ void tx_view_dir(const GsTextureArgs& a, int i, float v[3], float* len) {
    view_dir(a.xyz, a.campos, a.fwd_transform, a.rot_stride, a.rot_row, a.use_noise, tx_noise(a), i, v, len);
}

// b[k - 1] = basis k = 1 .. (deg + 1)^2 - 1 at (x, y, z)
__device__ __forceinline__ void tx_sh_bases(int deg, float x, float y, float z, float* b) {
    b[0] = -SH_C1 * y;
    b[1] = SH_C1 * z;
    b[2] = -SH_C1 * x;
    if (deg < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[3] = SH_C2[0] * xy;
    b[4] = SH_C2[1] * yz;
    b[5] = SH_C2[2] * (2.0f * zz - xx - yy);
    b[6] = SH_C2[3] * xz;
    b[7] = SH_C2[4] * (xx - yy);
    if (deg < 3) return;
    b[8] = SH_C3[0] * y * (3.0f * xx - yy);
    b[9] = SH_C3[1] * xy * z;
    b[10] = SH_C3[2] * y * (4.0f * zz - xx - yy);
    b[11] = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    b[12] = SH_C3[4] * x * (4.0f * zz - xx - yy);
    b[13] = SH_C3[5] * z * (xx - yy);
    b[14] = SH_C3[6] * x * (xx - 3.0f * yy);
    if (deg < 4) return;
    b[15] = SH_C4[0] * xy * (xx - yy);
    b[16] = SH_C4[1] * yz * (3.0f * xx - yy);
    b[17] = SH_C4[2] * xy * (7.0f * zz - 1.0f);
    b[18] = SH_C4[3] * yz * (7.0f * zz - 3.0f);
    b[19] = SH_C4[4] * (zz * (35.0f * zz - 30.0f) + 3.0f);
    b[20] = SH_C4[5] * xz * (7.0f * zz - 3.0f);
    b[21] = SH_C4[6] * (xx - yy) * (7.0f * zz - 1.0f);
    b[22] = SH_C4[7] * xz * (xx - 3.0f * yy);
    b[23] = SH_C4[8] * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
}

// du = sum_k g[k - 1] d basis_k / d (x, y, z)
__device__ __forceinline__ void tx_sh_bases_bwd(int deg, float x, float y, float z, const float* g, float du[3]) {
#define G(k) g[(k) - 1]
    float dx = -SH_C1 * G(3), dy = -SH_C1 * G(1), dz = SH_C1 * G(2);
    if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        dx += SH_C2[0] * y * G(4) - 2.0f * SH_C2[2] * x * G(6) + SH_C2[3] * z * G(7) + 2.0f * SH_C2[4] * x * G(8);
        dy += SH_C2[0] * x * G(4) + SH_C2[1] * z * G(5) - 2.0f * SH_C2[2] * y * G(6) - 2.0f * SH_C2[4] * y * G(8);
        dz += SH_C2[1] * y * G(5) + 4.0f * SH_C2[2] * z * G(6) + SH_C2[3] * x * G(7);
        if (deg > 2) {
            dx += SH_C3[0] * G(9) * 6.0f * xy + SH_C3[1] * G(10) * yz - SH_C3[2] * G(11) * 2.0f * xy - SH_C3[3] * G(12) * 6.0f * xz +
                  SH_C3[4] * G(13) * (4.0f * zz - 3.0f * xx - yy) + SH_C3[5] * G(14) * 2.0f * xz + SH_C3[6] * G(15) * 3.0f * (xx - yy);
            dy += SH_C3[0] * G(9) * 3.0f * (xx - yy) + SH_C3[1] * G(10) * xz + SH_C3[2] * G(11) * (4.0f * zz - xx - 3.0f * yy) -
                  SH_C3[3] * G(12) * 6.0f * yz - SH_C3[4] * G(13) * 2.0f * xy - SH_C3[5] * G(14) * 2.0f * yz -
                  SH_C3[6] * G(15) * 6.0f * xy;
            dz += SH_C3[1] * G(10) * xy + SH_C3[2] * G(11) * 8.0f * yz + SH_C3[3] * G(12) * 3.0f * (2.0f * zz - xx - yy) +
                  SH_C3[4] * G(13) * 8.0f * xz + SH_C3[5] * G(14) * (xx - yy);
            if (deg > 3) {
                const float a = 7.0f * zz - 1.0f, b = 7.0f * zz - 3.0f, c = 21.0f * zz - 3.0f;
                const float p = 3.0f * xx - yy, q = xx - 3.0f * yy, e = xx - yy;  // d(xy e)/dx = y p, d(xy e)/dy = x q
                dx += SH_C4[0] * G(16) * y * p + SH_C4[1] * G(17) * 6.0f * xy * z + SH_C4[2] * G(18) * y * a + SH_C4[5] * G(21) * z * b +
                      SH_C4[6] * G(22) * 2.0f * x * a + SH_C4[7] * G(23) * 3.0f * z * e + SH_C4[8] * G(24) * 4.0f * x * q;
                dy += SH_C4[0] * G(16) * x * q + SH_C4[1] * G(17) * 3.0f * z * e + SH_C4[2] * G(18) * x * a + SH_C4[3] * G(19) * z * b -
                      SH_C4[6] * G(22) * 2.0f * y * a - SH_C4[7] * G(23) * 6.0f * xy * z - SH_C4[8] * G(24) * 4.0f * y * p;
                dz += SH_C4[1] * G(17) * y * p + SH_C4[2] * G(18) * 14.0f * xy * z + SH_C4[3] * G(19) * y * c +
                      SH_C4[4] * G(20) * z * (140.0f * zz - 60.0f) + SH_C4[5] * G(21) * x * c + SH_C4[6] * G(22) * 14.0f * z * e +
                      SH_C4[7] * G(23) * x * q;
            }
        }
    }
#undef G
    du[0] = dx;
    du[1] = dy;
    du[2] = dz;
}

// first columns of sh_embed, after_0 and latent
__device__ __forceinline__ void tx_columns(const GsTextureArgs& a, int* sh_col, int* nsh, int* after_col, int* lat_col) {
    int c = 0;
    for (int b = 0; b < a.n_before; b++) c += a.before_w[b];
    *sh_col = c;
    *nsh = (a.sh_degree + 1) * (a.sh_degree + 1) - 1;
    c += *nsh;
    *after_col = c;
    for (int b = 0; b < a.n_after; b++) c += a.after_w[b];
    *lat_col = c;
}

__global__ __launch_bounds__(TX_THREADS) void tx_input_fwd_kernel(GsTextureArgs a, int R, float* __restrict__ inp) {
    __shared__ float4 buf4[TX_LDS_FLOATS / 4];
    float* buf = reinterpret_cast<float*>(buf4);
    const int t = threadIdx.x, D = a.D;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int n = (int)min((size_t)R, (size_t)a.N - row0);
    int sh_col, nsh, after_col, lat_col;
    tx_columns(a, &sh_col, &nsh, &after_col, &lat_col);
    for (int b = 0, col = 0; b < a.n_before; col += a.before_w[b], b++)
        tx_scatter(buf, D, col, a.before[b] + row0 * a.before_w[b], n, a.before_w[b]);
    for (int b = 0, col = after_col; b < a.n_after; col += a.after_w[b], b++)
        tx_scatter(buf, D, col, a.after[b] + row0 * a.after_w[b], n, a.after_w[b]);
    if (nsh > 0 && t < n) {
        float v[3], len, sh[TX_MAX_SH];
        tx_view_dir(a, (int)(row0 + t), v, &len);
        const float den = len + 1e-12f;
        tx_sh_bases(a.sh_degree, v[0] / den, v[1] / den, v[2] / den, sh);
#pragma unroll
        for (int k = 0; k < TX_MAX_SH; k++)
            if (k < nsh) buf[t * D + sh_col + k] = sh[k];
    }
    if (a.latent_dim > 0) {
        const int Lt = a.latent_dim, total = n * Lt;
        for (int f = t; f < total; f += TX_THREADS) {
            const int r = f / Lt, c = f - r * Lt;
            buf[r * D + lat_col + c] = a.latent[c];
        }
    }
    __syncthreads();
    slab_store<TX_THREADS>(inp + row0 * D, n * D, buf);
}

__global__ __launch_bounds__(TX_THREADS) void tx_input_bwd_kernel(GsTextureArgs a, int R, const float* __restrict__ g, TxGrads gr,
                                                                  float* __restrict__ dxyz, float* __restrict__ partial) {
    __shared__ float4 buf4[TX_LDS_FLOATS / 4];
    __shared__ float s_part[GS_TEXTURE_MAX_D];
    float* buf = reinterpret_cast<float*>(buf4);
    const int t = threadIdx.x, D = a.D;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int n = (int)min((size_t)R, (size_t)a.N - row0);
    int sh_col, nsh, after_col, lat_col;
    tx_columns(a, &sh_col, &nsh, &after_col, &lat_col);
    slab_load<TX_THREADS>(g + row0 * D, n * D, buf);
    __syncthreads();
    for (int b = 0, col = 0; b < a.n_before; col += a.before_w[b], b++)
        if (gr.before[b]) tx_gather(buf, D, col, gr.before[b] + row0 * a.before_w[b], n, a.before_w[b]);
    for (int b = 0, col = after_col; b < a.n_after; col += a.after_w[b], b++)
        if (gr.after[b]) tx_gather(buf, D, col, gr.after[b] + row0 * a.after_w[b], n, a.after_w[b]);
    if (dxyz && t < n) {
        const size_t i = row0 + t;
        float v[3], len, gs[TX_MAX_SH], du[3];
        tx_view_dir(a, (int)i, v, &len);
        const float inv = 1.0f / (len + 1e-12f);
#pragma unroll
        for (int k = 0; k < TX_MAX_SH; k++) gs[k] = k < nsh ? buf[t * D + sh_col + k] : 0.0f;
        tx_sh_bases_bwd(a.sh_degree, v[0] * inv, v[1] * inv, v[2] * inv, gs, du);
        // u = v / (l + eps):  du/dv = I / (l + eps) - v v^T / (l (l + eps)^2)
        const float dotv = v[0] * du[0] + v[1] * du[1] + v[2] * du[2];
        const float k2 = len > 0.0f ? dotv * inv * inv / len : 0.0f;
        float gv[3] = {du[0] * inv - v[0] * k2, du[1] * inv - v[1] * k2, du[2] * inv - v[2] * k2};
        if (a.use_noise) {  // v_out = v_in @ noise  ->  g_in = noise g_out
            const float* m = a.noise;
            const float w[3] = {m[0] * gv[0] + m[1] * gv[1] + m[2] * gv[2], m[3] * gv[0] + m[4] * gv[1] + m[5] * gv[2],
                                m[6] * gv[0] + m[7] * gv[1] + m[8] * gv[2]};
            gv[0] = w[0]; gv[1] = w[1]; gv[2] = w[2];
        }
        if (a.fwd_transform) {  // v_out = R^T v_in  ->  g_in = R g_out
            const float* Rm = a.fwd_transform + i * (size_t)a.rot_stride;
            const int rs = a.rot_row;
            const float w[3] = {Rm[0] * gv[0] + Rm[1] * gv[1] + Rm[2] * gv[2], Rm[rs] * gv[0] + Rm[rs + 1] * gv[1] + Rm[rs + 2] * gv[2],
                                Rm[2 * rs] * gv[0] + Rm[2 * rs + 1] * gv[1] + Rm[2 * rs + 2] * gv[2]};
            gv[0] = w[0]; gv[1] = w[1]; gv[2] = w[2];
        }
        dxyz[3 * i] = gv[0];
        dxyz[3 * i + 1] = gv[1];
        dxyz[3 * i + 2] = gv[2];
    }
    if (partial) {  // (uniform) column c: S runs of rows s, s + S, .., each in row order, then the runs in order
        const int Lt = a.latent_dim, S = max(1, min(TX_SEG_MAX, TX_THREADS / Lt));
        for (int e = t; e < S * Lt; e += TX_THREADS) {
            const int s = e / Lt, c = e - s * Lt;
            float acc = 0.0f;
            for (int r = s; r < n; r += S) acc += buf[r * D + lat_col + c];
            s_part[e] = acc;
        }
        __syncthreads();
        for (int c = t; c < Lt; c += TX_THREADS) {
            float acc = s_part[c];
            for (int s = 1; s < S; s++) acc += s_part[s * Lt + c];
            partial[(size_t)c * gridDim.x + blockIdx.x] = acc;
        }
    }
}

// ---- launchers (the C ABI has checked every argument)
static int launch_texture_input_forward(const GsTextureArgs* a, float* inp, hipStream_t s) {
    StageScope st("texture_input", s);
    hipLaunchKernelGGL(tx_input_fwd_kernel, dim3(tx_blocks(a->N, a->D)), dim3(TX_THREADS), 0, s, *a, tx_rows(a->D), inp);
    GS_LAUNCH_CHECK("texture_input", 0, s);
    return GS_OK;
}
static int launch_texture_input_backward(const GsTextureArgs* a, const float* g, const TxGrads& grads, float* dxyz, float* dlatent,
                                         void* workspace, hipStream_t s) {
    StageScope st("texture_input_bwd", s);
    const int nb = tx_blocks(a->N, a->D);
    float* partial = dlatent ? reinterpret_cast<float*>(workspace) : nullptr;
    hipLaunchKernelGGL(tx_input_bwd_kernel, dim3(nb), dim3(TX_THREADS), 0, s, *a, tx_rows(a->D), g, grads, dxyz, partial);
    GS_LAUNCH_CHECK("texture_input_bwd", 0, s);
    if (dlatent) {
        hipLaunchKernelGGL((ordered_final_kernel<TX_THREADS, WavesInOrder, false>), dim3(a->latent_dim), dim3(TX_THREADS), 0, s,
                           (const float*)partial, nb, 1.0f, dlatent);
        GS_LAUNCH_CHECK("texture_final", 0, s);
    }
    return GS_OK;
}

extern "C" {

static int texture_validate(const GsTextureArgs* a) {
    if (!a || a->N < 0 || a->sh_degree < 0 || a->sh_degree > 4 || a->n_before < 0 || a->n_before > GS_TEXTURE_MAX_BEFORE ||
        a->n_after < 0 || a->n_after > GS_TEXTURE_MAX_AFTER || a->latent_dim < 0 || a->latent_dim > GS_TEXTURE_MAX_D)
        return GS_E_BAD_ARG;
    int64_t sum = (a->sh_degree + 1) * (a->sh_degree + 1) - 1 + a->latent_dim;
    for (int b = 0; b < a->n_before; b++) {
        if (a->before_w[b] < 1 || a->before_w[b] > GS_TEXTURE_MAX_D) return GS_E_BAD_ARG;
        sum += a->before_w[b];
    }
    for (int b = 0; b < a->n_after; b++) {
        if (a->after_w[b] < 1 || a->after_w[b] > GS_TEXTURE_MAX_D) return GS_E_BAD_ARG;
        sum += a->after_w[b];
    }
    if (a->D < 1 || a->D > GS_TEXTURE_MAX_D || sum != a->D) return GS_E_BAD_ARG;
    return GS_OK;
}
// what the view direction is made of (sh_degree > 0)
static bool texture_dir_ok(const GsTextureArgs* a) {
    if (!required(a->xyz, 4) || !required(a->campos, 4) || !aligned(a->fwd_transform, 4)) return false;
    return !a->fwd_transform || (a->rot_row >= 3 && a->rot_stride >= 2 * (int64_t)a->rot_row + 3);
}
int gs_texture_workspace_bytes(int32_t N, int32_t D, int32_t latent_dim, size_t* out) {
    if (!out || N < 0 || D < 1 || D > GS_TEXTURE_MAX_D || latent_dim < 0 || latent_dim > D) return GS_E_BAD_ARG;
    *out = texture_workspace_bytes(N, D, latent_dim);
    return GS_OK;
}
int gs_texture_input_forward(const GsTextureArgs* a, float* inp, void* stream) {
    if (const int rc = texture_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!required(inp, 16)) return GS_E_BAD_ARG;
    for (int b = 0; b < a->n_before; b++)
        if (!required(a->before[b], 16)) return GS_E_BAD_ARG;
    for (int b = 0; b < a->n_after; b++)
        if (!required(a->after[b], 16)) return GS_E_BAD_ARG;
    if (a->latent_dim > 0 && !required(a->latent, 4)) return GS_E_BAD_ARG;
    if (a->sh_degree > 0 && !texture_dir_ok(a)) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_texture_input_forward(a, inp, (hipStream_t)stream);
}
int gs_texture_input_backward(const GsTextureArgs* a, const float* dL_dinp, float* const* dL_dbefore, float* const* dL_dafter,
                              float* dL_dxyz, float* dL_dlatent, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = texture_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!required(dL_dinp, 16)) return GS_E_BAD_ARG;
    TxGrads gr = {};
    bool any = dL_dxyz || dL_dlatent;
    for (int b = 0; b < a->n_before; b++) {
        gr.before[b] = dL_dbefore ? dL_dbefore[b] : nullptr;
        if (!aligned(gr.before[b], 16)) return GS_E_BAD_ARG;
        any = any || gr.before[b];
    }
    for (int b = 0; b < a->n_after; b++) {
        gr.after[b] = dL_dafter ? dL_dafter[b] : nullptr;
        if (!aligned(gr.after[b], 16)) return GS_E_BAD_ARG;
        any = any || gr.after[b];
    }
    if (dL_dxyz && (a->sh_degree == 0 || !aligned(dL_dxyz, 4) || !texture_dir_ok(a))) return GS_E_BAD_ARG;
    if (dL_dlatent) {
        if (a->latent_dim == 0 || !aligned(dL_dlatent, 4) || !required(workspace, 4)) return GS_E_BAD_ARG;
        if (workspace_bytes < texture_workspace_bytes(a->N, a->D, a->latent_dim)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    if (!any) return GS_OK;
    return launch_texture_input_backward(a, dL_dinp, gr, dL_dxyz, dL_dlatent, workspace, (hipStream_t)stream);
}

}  // extern "C"
