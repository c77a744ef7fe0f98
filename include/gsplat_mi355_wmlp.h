/*
 * gsplat_mi355_wmlp.h -- C ABI of the wide fused MLP of libgsplat_mi355.so (csrc/mlp_wide.hip), the module beside the
 * entry points of gsplat_mi355.h.  Same conventions: plain pointers and sizes only, every pointer a device pointer unless
 * it says host, `stream` a hipStream_t (NULL: the null stream), the return value one of gsplat_mi355.h's status codes
 * (GS_OK 0, GS_E_BAD_ARG -1, GS_E_HIP -4, GS_E_WORKSPACE -5, GS_E_CAPTURE -6; gs_status_string names them).
 * The Python binding is gsplat_mi355/_wide_lib.py; tests/test_wide_mlp_host.py holds the two together.
 */
#ifndef GSPLAT_MI355_WMLP_H
#define GSPLAT_MI355_WMLP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the wide coordinate networks (models/network_utils.py VanillaCondMLP with a frequency encoding, skip connections
 * or width 256; HannwCondMLP) as one fused op on the exact-fp32 MFMA, beside gs_mlp_* (gsplat_mi355.h) and by the same rules.  The full
 * semantics, every gradient included, are spelled out at the top of csrc/mlp_wide.hip.  All arrays are fp32, row-major,
 * contiguous.
 *   Encoding e = enc(x), E columns: multires == 0: e = x, E = dim_x (include_input is not read).  multires = m > 0: the
 *     block x (with include_input = 1), then for k = 0 .. m - 1 the blocks band_w[k] sin(2^k x), band_w[k] cos(2^k x),
 *     dim_x columns each, in that order: E = dim_x (include_input + 2 m).  band_w are host floats passed by value (all 1
 *     for VanillaCondMLP, the Hann window for HannwCondMLP); sin and cos are the accurate sinf / cosf.
 *   Layers: h_0 = e; layer l reads v_0 = [h_0 | cond], v_l = [h_l | e] / sqrt(2) where bit l of skip_mask is set, else
 *     v_l = h_l;  z_l = v_l W_l^T + b_l;  h_{l+1} = z_l > 0 ? z_l : slope z_l for l < n_hidden;  y = z_{n_hidden}.  A
 *     layer that feeds a skip layer has width - E outputs: W[0] [out_0, E + dim_cond], W[l] [out_l, width], out_l =
 *     dim_out for l = n_hidden, width - E where bit l + 1 of skip_mask is set, else width.
 *   Backward from dL_dy: dW[l], db[l] (shaped as W[l], b[l]), dcond [dim_cond], and dx [N, dim_x] through the skip
 *     connections and the encoding, which is recomputed from x.  NULL = not wanted, and then neither computed nor written.
 * GsWideMlpArgs (handed to the kernels by value): N rows; dim_x >= 1; multires in 0..GS_WMLP_MAX_FREQS; include_input 0 or
 *   1; E in 1..GS_WMLP_MAX_ENC; dim_cond in 0..GS_WMLP_MAX_COND; width a multiple of 32 in 32..GS_WMLP_MAX_WIDTH; n_hidden
 *   in 1..GS_WMLP_MAX_HIDDEN; dim_out in 1..GS_WMLP_MAX_OUT; skip_mask a subset of the bits 1..n_hidden, and E < width where
 *   it is not empty; slope >= 0 (0: ReLU); x [N, dim_x]; cond [dim_cond], ONE row (NULL at dim_cond 0).
 * gs_wmlp_forward (one launch; one small launch in front of it at dim_cond > 0): y [N, dim_out]; saved (16-byte aligned,
 *   gs_wmlp_saved_bytes(a) bytes: [n_hidden, N, width], every hidden layer's output as the next layer reads it), what
 *   gs_wmlp_backward reads, NULL = not saved.  `workspace`: gs_wmlp_workspace_bytes(a, 0) bytes (none at dim_cond 0).
 * gs_wmlp_backward (at most three launches): from dL_dy [N, dim_out] (16-byte aligned) and saved to the wanted gradients.
 *   `workspace` (16-byte aligned): gs_wmlp_workspace_bytes(a, 1) bytes -- the layers' pre-activation gradients, the
 *   encoding's gradient at multires > 0, and at most GS_WMLP_MAX_PARTIALS partial parameter gradients, each over
 *   max(GS_WMLP_PARTIAL_MIN_ROWS, ceil(N / GS_WMLP_MAX_PARTIALS) rounded up to 32) consecutive rows and summed in index
 *   order: no atomics, bitwise reproducible, the partition a function of N alone.  A forward tile is GS_WMLP_TILE_ROWS rows.
 * N == 0 does nothing, and both byte counts are 0.  GS_E_BAD_ARG (before any HIP call): a NULL args, N < 0, a size outside
 *   the ranges above, a skip at layer 0 or past n_hidden, E >= width with a skip, a negative or NaN slope, a NaN band
 *   weight, a NULL required pointer or a misaligned one (16 bytes for saved, dL_dy and the backward's workspace, else fp32
 *   alignment), dcond at dim_cond 0.  GS_E_WORKSPACE: the workspace is smaller than gs_wmlp_workspace_bytes says.
 * Capture-safe (kernel launches only, no host wait), with the stage timer off: gs_wmlp_forward, gs_wmlp_backward. ---- */
#define GS_WMLP_MAX_WIDTH 256
#define GS_WMLP_MAX_HIDDEN 8
#define GS_WMLP_MAX_LAYERS 9
#define GS_WMLP_MAX_FREQS 10
#define GS_WMLP_MAX_ENC 512
#define GS_WMLP_MAX_COND 512
#define GS_WMLP_MAX_OUT 64
#define GS_WMLP_TILE_ROWS 128
#define GS_WMLP_PARTIAL_MIN_ROWS 256
#define GS_WMLP_MAX_PARTIALS 128
typedef struct GsWideMlpArgs {
    int32_t N, dim_x, multires, include_input, dim_cond, width, n_hidden, dim_out;
    uint32_t skip_mask;
    float slope;
    float band_w[GS_WMLP_MAX_FREQS];
    const float *x, *cond;
    const float* W[GS_WMLP_MAX_LAYERS];
    const float* b[GS_WMLP_MAX_LAYERS];
    float* dW[GS_WMLP_MAX_LAYERS];
    float* db[GS_WMLP_MAX_LAYERS];
    float *dx, *dcond;
} GsWideMlpArgs;
int gs_wmlp_workspace_bytes(const GsWideMlpArgs* a, int32_t backward, size_t* out);
int gs_wmlp_saved_bytes(const GsWideMlpArgs* a, size_t* out);
int gs_wmlp_forward(const GsWideMlpArgs* a, float* y, float* saved, void* workspace, size_t workspace_bytes, void* stream);
int gs_wmlp_backward(const GsWideMlpArgs* a, const float* saved, const float* dL_dy, void* workspace, size_t workspace_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_MI355_WMLP_H */
