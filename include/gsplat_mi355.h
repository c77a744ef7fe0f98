/*
 * gsplat_mi355.h -- C ABI of libgsplat_mi355.so: the MI355X (gfx950) differentiable
 * Gaussian-splat rasterizer and the distCUDA2 K-NN initialiser.
 *
 * Drop-in boundary.  The reference reaches this path through two Python imports of
 * third-party torch C++ extensions whose source is NOT vendored in the reference tree:
 *   - `from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer`
 *     (gaussian_renderer/__init__.py:17; settings built at :85-98, module at :100, calls at
 *     :121-129 and :133-141)  ->  upstream `_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward`,
 *     `_C.mark_visible`
 *   - `from simple_knn._C import distCUDA2` (scene/gaussian_model.py:20, call at :186)
 * Each entry point below names the upstream binding it replaces.  Plain pointers and sizes only:
 * no torch types.  Every pointer is a DEVICE pointer unless it says "host".  The library never
 * allocates or frees device memory and never synchronises the stream except where stated; all
 * work is enqueued on the caller's `stream` (a hipStream_t passed as void*), so calls are
 * re-entrant across streams and devices (the caller selects the device).
 *
 * All entry points return 0 on success, a negative GS_E_* code on failure; `gs_status_string`
 * turns a code into text.  A NULL optional pointer means "absent", mirroring the upstream
 * wrapper's empty-tensor convention (gaussian_renderer/__init__.py:107-129).
 */
#ifndef GSPLAT_MI355_H
#define GSPLAT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK 0
#define GS_E_BAD_ARG (-1)      /* NULL required pointer, non-positive size, bad sh degree, M > 16, rotations / dL_drotations not 16-byte aligned */
#define GS_E_EXCLUSIVE (-2)    /* both / neither of (shs | colors_precomp) or (scales+rotations | cov3D_precomp) */
#define GS_E_TOO_LARGE (-3)    /* num_rendered or tile count exceeds the 32-bit index space  */
#define GS_E_HIP (-4)          /* a HIP launch or API call failed (see gs_last_hip_error)    */
#define GS_E_WORKSPACE (-5)    /* a caller-provided buffer is smaller than gs_*_bytes says    */
#define GS_E_CAPTURE (-6)      /* `stream` is being captured into a hipGraph and this call, with these arguments, is not
                                * capture-safe (see "Stream capture" below); nothing was enqueued */

/* ---- Stream capture (hipGraph).  Every entry point that takes a stream asks hipStreamIsCapturing first.  A call that
 * would wait for the GPU, copy to or store into host memory, or enqueue anything but kernel launches returns
 * GS_E_CAPTURE without enqueuing anything -- it never leaves the capture half-built or faults on replay.  Capture-safe
 * (kernel launches only, every pointer a device pointer, no host wait):
 *   gs_forward_preprocess  with count_host_pinned == NULL (the count stays in the geom state: gs_geom_field GS_GEOM_COUNT)
 *   gs_forward_render      with a->frame_stats == NULL, at a fixed capacity (a frame whose count exceeds it renders
 *                          empty: read the count afterwards, outside the graph)
 *   gs_forward_shared (P > 0), gs_opacity_image, gs_backward, gs_backward_with_opacity, gs_backward_with_second,
 *   (with GsSecondImage.dL_dcolors, too: kernel launches only),
 *   gs_mark_visible, gs_l1_loss, gs_bce_loss, gs_ssim_*, gs_build_covariance*, gs_sh2rgb* (view_noise_host == NULL),
 *   gs_densify_stats, gs_densify_plan (count_host_pinned == NULL), gs_densify_apply, gs_reset_opacity,
 *   gs_aiap_forward, gs_aiap_backward, gs_hashgrid_forward, gs_hashgrid_backward, gs_skin_weights_forward,
 *   gs_skin_weights_backward, gs_skinning_forward, gs_skinning_backward, gs_mesh_sample, gs_skin_loss_forward,
 *   gs_skin_loss_backward, gs_pose_forward, gs_pose_backward,
 *   gs_pose_encoder_forward, gs_pose_encoder_backward, gs_nonrigid_apply_forward, gs_nonrigid_apply_backward,
 *   gs_texture_input_forward, gs_texture_input_backward, gs_mlp_forward, gs_mlp_backward,
 *   gs_lpips_forward, gs_lpips_backward, gs_lpips_conv, gs_lpips_pool,
 *   gs_grad_norm, gs_grad_scale, gs_adam_step_ex (every tensor with a device-resident step number)
 * -- all of them with a->debug == 0 and the stage timer (gs_profile_enable) off.  Not capture-safe: gs_forward (it waits
 * for the pair count on the host), gs_adam_step (the step number is a host scalar: a replay would repeat the captured
 * step's bias correction; gs_adam_step_ex likewise for a tensor without a device step), knn_dist2 / knn_points (their sorts clear tables with memset nodes: untested under replay),
 * anything in debug mode.  GsFwdArgs.antialiasing changes nothing about capture safety: it is a kernel argument of launches that are there either way. */

/* Arguments of one rasterizer call: the fields of GaussianRasterizationSettings
 * (gaussian_renderer/__init__.py:85-98) plus the tensors of GaussianRasterizer.forward
 * (:121-129), flattened.  Shapes (fp32, contiguous): means3D[P,3], opacities[P], shs[P,M,3]
 * (coefficient-major, channel-minor; scene/gaussian_model.py:145-148), colors_precomp[P,3],
 * scales[P,3], rotations[P,4] (w,x,y,z; utils/general_utils.py:94-97; 16-byte aligned), cov3D_precomp[P,6]
 * ([xx,xy,xz,yy,yz,zz]; utils/general_utils.py:73-85), viewmatrix[16] and projmatrix[16]
 * (row-vector convention, scene/cameras.py:35-39), campos[3], bg[3]. */
typedef struct GsFwdArgs {
    int32_t P;          /* number of Gaussians                                  */
    int32_t sh_degree;  /* active SH degree 0..3 (settings.sh_degree)           */
    int32_t M;          /* SH coefficients present per channel: shs.shape[1]    */
    int32_t W, H;       /* image_width, image_height                            */
    const float* bg;
    const float* means3D;
    const float* shs;            /* NULL if colors_precomp given */
    const float* colors_precomp; /* NULL if shs given            */
    const float* opacities;
    const float* scales;         /* NULL if cov3D_precomp given  */
    const float* rotations;      /* NULL if cov3D_precomp given  */
    const float* cov3D_precomp;  /* NULL if scales/rotations     */
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    float scale_modifier, tanfovx, tanfovy;
    int32_t prefiltered; /* accepted for API parity; culled points are skipped either way */
    int32_t debug;       /* !=0: synchronise + check after every kernel, name the failing stage */
    int32_t tile_rect;   /* which tiles a Gaussian is binned into.  0: upstream's square of half-width ceil(3 sigma_max)
                          * around the centre.  1: the bounding box of the region where its alpha can reach 1/255
                          * (half-widths sqrt(2 ln(255 opacity) Sigma_xx), sqrt(... Sigma_yy)), intersected with the
                          * square: every tile left out contributes nothing to any pixel, so colour, radii and all
                          * gradients are those of mode 0 while num_rendered and the tile lists are ~40 % shorter */
    int32_t long_lists;  /* 0: the machinery for frames of few, long tile lists (four waves per quadrant in the forward on
                          * the tiles whose list is long against the frame's total, backward in chunks from checkpoints of
                          * the forward) is used on images of up to 2048 tiles only.  1: on this image whatever its size --
                          * the image state is then larger (gs_image_bytes_for).  A frame that fills the chip with one wave
                          * per quadrant is ~10 % slower with it, one of few long lists (a trained avatar filling a sixth of
                          * 1024 x 1024) 1.45 x faster; outputs agree to fp32 rounding.  The SAME value must be passed to the
                          * backward (and to gs_forward_shared) of a forward */
    int64_t* frame_stats; /* NULL, or two words the forward writes (device-visible host memory or device memory), for the
                          * caller to choose long_lists for the NEXT frame: [0] tiles whose list is long against this
                          * frame's total (the tiles the four-wave forward takes), [1] the longest tile list */
    /* ---- L1 image loss fused into the rasterizer (train.py:121 `Ll1 = l1_loss(image, gt_image)`,
     * utils/loss_utils.py:21-22).  l1_target (NULL = off): the target image [3,H,W].  The forward's render launch then also
     * adds up |out_color - l1_target| over the pixels it has just composited and l1_loss[0] (device float, required with
     * l1_target) receives the mean over the 3 H W elements -- the image is not read again.  The backward (the same
     * argument block) forms dL/d out_color of that loss itself, per pixel, in the prologue of its render pass:
     * sign(out_color - l1_target) / (3 H W) times l1_grad[0] (device float = dLoss/d l1_loss; NULL = 1), ADDED to the
     * dL_dpix the caller passes (which may then be NULL) -- no gradient image is written or read.  Supported by
     * gs_forward / gs_forward_render and every gs_backward*; gs_forward_shared ignores it. */
    const float* l1_target;
    float* l1_loss;
    const float* l1_grad;
    int32_t forward_only; /* !=0: no backward will follow this forward (a frame rendered under no_grad): the render launch does
                           * not prepare the backward's row marks on the side (55 MB of streaming stores at config 3).  A
                           * backward that is run on the state anyway prepares them itself, as after a first backward */
    int32_t antialiasing; /* upstream's `antialiasing` setting (the Mip-Splatting compensation).  Let (a0, b, c0) be the
                           * EWA-projected 2-D covariance before the 0.3 px^2 screen-space dilation, a = a0 + 0.3, c = c0 + 0.3,
                           * det0 = a0 c0 - b^2, det1 = a c - b^2, s = sqrt(max(0.000025, det0 / det1)).  !=0: the opacity
                           * everything downstream of the projection sees is o' = o s (the tile_rect = 1 box, the splat record
                           * and through it the render loops, the 1 - T opacity image and gs_forward_shared); radii, conic,
                           * depth, colour, the 3-sigma square and culling do not depend on it.  0: o' = o.  Every gs_backward*
                           * of such a forward (the SAME value must be passed) returns dL/do = s dL/do' and, where
                           * det0 / det1 > 0.000025, adds dL/do' o' (1/2) (c0/det0 - c/det1), dL/do' o' (1/2) (a0/det0 - a/det1)
                           * and dL/do' o' b (1/det1 - 1/det0) to dL/da, dL/dc and dL/db (b the one off-diagonal parameter) in
                           * front of the chain to cov3D (scales, rotations) and means3D; where the clamp is active (det0 <= 0
                           * included) nothing is added and dL/do = 0.005 dL/do'.  Takes the place of tail padding: no
                           * offset and no state-buffer layout changes */
} GsFwdArgs;

/* The eight gradient outputs of upstream `rasterize_gaussians_backward`, in the order the
 * autograd wrapper returns them.  Every non-NULL array is written IN FULL by the call (zeros for
 * culled Gaussians): the caller does not need to pre-zero.  dL_dsh may be NULL when shs is absent,
 * dL_dscales / dL_drotations when cov3D_precomp was given. */
typedef struct GsGrads {
    float* dL_dmeans3D;  /* [P,3] */
    float* dL_dmeans2D;  /* [P,3]  x,y = d/d(NDC centre), z = 0 (consumed as .grad[:, :2], scene/gaussian_model.py:464-466) */
    float* dL_dsh;       /* [P,M,3] */
    float* dL_dcolors;   /* [P,3]  gradient of colors_precomp (or of the SH colour before the clamp mask) */
    float* dL_dopacity;  /* [P,1] */
    float* dL_dscales;   /* [P,3] */
    float* dL_drotations;/* [P,4] */
    float* dL_dcov3D;    /* [P,6] */
} GsGrads;

/* ---- state-buffer sizes (the caller owns every allocation; upstream grew torch byte tensors
 * through a resize callback: geomBuffer / binningBuffer / imgBuffer) ---- */
int gs_geom_bytes(int32_t P, size_t* out);
int gs_image_bytes(int32_t W, int32_t H, size_t* out);
int gs_binning_bytes(int64_t num_rendered, int32_t W, int32_t H, size_t* out);
int gs_backward_scratch_bytes(int64_t num_rendered, int32_t P, int32_t W, int32_t H, size_t* out);

/* ---- forward, phase 1 (replaces the first half of upstream rasterize_gaussians: preprocess +
 * prefix sum).  Runs: per-Gaussian preprocess (cull, EWA projection, conic, radius, tile rect,
 * SH->RGB), a stable depth sort of the Gaussians, and the prefix sum of tiles touched.
 * Writes radii[P] (int32).  The number of (tile, Gaussian) pairs `num_rendered` is left in the geom
 * state and, if `count_host_pinned` is non-NULL, copied asynchronously (same stream) into that
 * HOST-pinned int64; the caller synchronises before reading it.  No implicit synchronisation. */
int gs_forward_preprocess(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* img, size_t img_bytes,
                          int32_t* radii, int64_t* count_host_pinned, void* stream);

/* ---- forward, phase 2 (second half of upstream rasterize_gaussians: duplicateWithKeys, sort,
 * identifyTileRanges, render).  `num_rendered` is the number of pairs the binning state is carved for: the value
 * phase 1 produced, or any larger capacity (the kernels read the frame's own count from the geom state).  Writes
 * out_color[3,H,W]. */
int gs_forward_render(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                      void* img, size_t img_bytes, int64_t num_rendered, float* out_color, void* stream);

/* ---- forward, both phases in one call (the whole of upstream rasterize_gaussians), with NO GPU idle stretch for the
 * pair count.  Upstream blocks on a device-to-host copy of num_rendered between its two halves, because the count
 * sizes the binning buffer.  Here the caller passes a binning state sized for `capacity` pairs
 * (gs_binning_bytes(capacity); e.g. the previous frame's count + 1/8); phase 2 is enqueued right behind phase 1 with
 * grids sized by the capacity, its kernels reading the count on the device, and only then does the host wait for the
 * count (stored by the device straight into the HOST-pinned `count_host_pinned`) -- the GPU is already busy with
 * phase 2.  Returns GS_OK with *num_rendered set when the count fits the capacity.  Returns GS_E_WORKSPACE with
 * *num_rendered set when it does not (phase 2 has then rendered an empty frame, nothing out of bounds), or when
 * capacity is 0 (only phase 1 ran): the caller allocates gs_binning_bytes(*num_rendered) and calls
 * gs_forward_render.  A state carved for `capacity` pairs is passed on with num_rendered = capacity to
 * gs_backward / gs_forward_shared / gs_binning_field (the carve is a function of that number). */
int gs_forward(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes, int64_t capacity,
               void* img, size_t img_bytes, int32_t* radii, int64_t* count_host_pinned, float* out_color,
               int64_t* num_rendered, void* stream);

/* ---- shared-geometry forward (no upstream counterpart).  The reference's render()
 * rasterizes twice per step with identical geometry -- colour pass, then an opacity pass with
 * colors = 1 (gaussian_renderer/__init__.py:121-142).  Given the geom / binning / image state of a
 * previous gs_forward_* call on the SAME means3D, opacities, covariance inputs and camera, this renders
 * new colours (a->shs or a->colors_precomp) without repeating preprocess, sorts and binning: it fills
 * a fresh geom / image state (usable by gs_backward) and shares the binning state.  The image is composited from the
 * quadrant lists the first render recorded (same bits as a stand-alone render); if colors_precomp is all ones -- found
 * out on the device, one word of geom_src is written -- it is instead written as 1 - T of the first render (+ T bg),
 * equal to the composited image to fp32 rounding.  Pass the SAME a->long_lists as to the first render, and the SAME
 * a->antialiasing: the records are copied, so this render has the first render's effective opacities whatever it is told,
 * and its backward must scale them the same way.  Its gradients
 * can be had together with the first render's in one pass: gs_backward_with_second. */
int gs_forward_shared(const GsFwdArgs* a, const void* geom_src, const void* img_src, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* img, size_t img_bytes, int64_t num_rendered,
                      float* out_color, void* stream);

/* ---- backward (replaces upstream rasterize_gaussians_backward).  `out_color` is the forward's
 * output image, `radii` the forward's radii, `dL_dpix` = dL/d out_color [3,H,W] (NULL allowed when a->l1_target is set: the
 * fused L1 loss is then the only consumer of the image).  `num_rendered` is the number of
 * pairs the forward's binning state was carved for (the capacity given to gs_forward, or the count given to
 * gs_forward_render).  `scratch` holds gs_backward_scratch_bytes(num_rendered, P, W, H) bytes.
 * The binning state also holds the mark word of every gradient row the backward writes (all "unwritten" on entry): the
 * forward's render launch sets them on the side and says so in a state word; a backward that finds them used by an
 * earlier backward of the same forward sets them itself.  A backward therefore WRITES that part of `binning` (which is
 * why the pointer is not const; the lists and ranges it only reads); two backwards of one forward must not run concurrently. */
int gs_backward(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes, void* binning,
                size_t binning_bytes, const void* img, size_t img_bytes, int64_t num_rendered,
                const float* out_color, const float* dL_dpix, void* scratch, size_t scratch_bytes,
                const GsGrads* grads, void* stream);

/* ---- opacity render fused into the colour render (second form).  The reference obtains
 * its opacity image with a SECOND rasterizer call with colours = 1 (gaussian_renderer/__init__.py:132-142; used by
 * the mask loss, train.py:143-153, lambda_mask = 0.1 in configs/config.yaml).  That image is
 * (1 - final_T) + final_T * bg[0] per pixel and the forward already holds final_T: gs_opacity_image writes it
 * ([H,W] floats) from the image state of a finished forward, and gs_backward_with_opacity takes the gradient of
 * that image as a fourth channel of the same backward pass (its background value is bg[0], as in the reference) --
 * one render and one backward instead of two of each. ---- */
int gs_opacity_image(const GsFwdArgs* a, const void* img, size_t img_bytes, float* opacity, void* stream);
int gs_backward_with_opacity(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes,
                             void* binning, size_t binning_bytes, const void* img, size_t img_bytes,
                             int64_t num_rendered, const float* out_color, const float* dL_dpix,
                             const float* dL_dopacity_img, void* scratch, size_t scratch_bytes, const GsGrads* grads,
                             void* stream);

/* A SECOND image rendered from the same geometry with other colours (gs_forward_shared: the reference's opacity pass,
 * gaussian_renderer/__init__.py:132-142) differentiated in the same pass as the first: alpha and T are shared, so the
 * second image adds one dot product per (pixel, Gaussian) step and one term to Gtot instead of a whole second backward.
 * The gradients are the SUM of both images' gradients w.r.t. the shared inputs; dL_dcolors / dL_dsh of `grads` are the
 * first image's, and the second image's colours get theirs when asked (GsSecondImage.dL_dcolors).  `img` = the image
 * state gs_forward_shared filled for the second render (its checkpoints; a word of it says whether that render's colours
 * were all (1, 1, 1), in which case the pass needs no second colours at all: the reference's case), `long_lists` the
 * value that render was given.
 * GsSecondImage.dL_dcolors, when not NULL, adds two launches behind the per-Gaussian backward (three where the tile lists
 * are few and long): a walk of the tile lists that writes one row of sum alpha T dL_dpix per pair into the rows region of
 * `scratch`, free by then, and a per-Gaussian sum of the rows.  No atomics: the same bits on every run.  A frame whose
 * pair count exceeds `D` (it rendered empty) gets zeros.  NULL: the call is what it was without the field, launch for
 * launch. */
typedef struct GsSecondImage {
    const float* colors;    /* [P,3] colors_precomp of the second render */
    const float* out_color; /* [3,H,W] its result */
    const float* dL_dpix;   /* [3,H,W] its gradient */
    const void* img;        /* its image state */
    size_t img_bytes;
    int32_t long_lists;
    float* dL_dcolors;      /* [P,3] or NULL: the gradient of `colors`, every row written (zeros for culled Gaussians) */
} GsSecondImage;
int gs_backward_with_second(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes,
                            void* binning, size_t binning_bytes, const void* img, size_t img_bytes, int64_t D,
                            const float* out_color, const float* dL_dpix, const GsSecondImage* second, void* scratch,
                            size_t scratch_bytes, const GsGrads* grads, void* stream);

/* ---- upstream mark_visible / GaussianRasterizer.markVisible: present[i] = (z_view > 0.2) ---- */
int gs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, void* stream);

/* ---- simple_knn._C.distCUDA2 (scene/gaussian_model.py:186): mean squared distance to the three
 * nearest other points.  points[P,3] fp32 -> mean_d2[P] fp32. ---- */
int knn_workspace_bytes(int32_t P, size_t* out);
int knn_dist2(int32_t P, const float* points, float* mean_d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- pre-rasterizer per-Gaussian chains.
 * gs_build_covariance: scene/gaussian_model.py:28-32 build_covariance_from_scaling_rotation =
 *   strip_symmetric(L L^T), L = R diag(scaling_modifier * scaling) (utils/general_utils.py:73-85,194-207);
 *   `rotation` is N quaternions (w,x,y,z), normalised as build_rotation does (general_utils.py:87-108), or,
 *   with rotation_is_matrix, N row-major 3x3 matrices (the rigid deformer's rotation_precomp,
 *   models/deformer/rigid.py:229-231).  cov6 = [xx, xy, xz, yy, yz, zz].  The backward gives what autograd
 *   derives for that chain (d/dscaling, d/drotation in the input's own parametrisation).
 * gs_sh2rgb: models/texture/texture.py:21-38 SH2RGB.forward: direction xyz - campos, optionally rotated by the
 *   transpose of fwd_rotation[N,3,3] (cano_view_dir: T_fwd[:, :3, :3]) and multiplied from the right by a 3x3
 *   view-noise matrix given as 9 HOST floats (NULL = none), normalised with +1e-12, eval_sh of degree
 *   sh_degree over shs[N,M,3], +0.5, clamp at 0.  `clamped` (N bytes, bit c = channel c clamped) feeds the
 *   backward, which returns d/dshs and d/dxyz (fwd_rotation carries no gradient: it is detached upstream,
 *   rigid.py:223). ---- */
int gs_build_covariance(int32_t N, const float* scaling, float scaling_modifier, const float* rotation,
                        int32_t rotation_is_matrix, float* cov6, void* stream);
int gs_build_covariance_backward(int32_t N, const float* scaling, float scaling_modifier, const float* rotation,
                                 int32_t rotation_is_matrix, const float* dL_dcov6, float* dL_dscaling,
                                 float* dL_drotation, void* stream);
int gs_sh2rgb(int32_t N, int32_t sh_degree, int32_t M, const float* shs, const float* xyz, const float* campos,
              const float* fwd_rotation, const float* view_noise_host, float* colors, uint8_t* clamped, void* stream);
int gs_sh2rgb_backward(int32_t N, int32_t sh_degree, int32_t M, const float* shs, const float* xyz, const float* campos,
                       const float* fwd_rotation, const float* view_noise_host, const uint8_t* clamped,
                       const float* dL_dcolors, float* dL_dshs, float* dL_dxyz, void* stream);

/* ---- image-side L1 loss: the reference computes
 * torch.abs(network_output - gt).mean() (utils/loss_utils.py:21-22, called at train.py:121) and lets
 * autograd derive d(loss)/d(network_output).  One call here: loss[0] = mean |x - y| and
 * dL_dx[i] = sign(x[i] - y[i]) / n, for n fp32 elements (pointers 16-byte aligned); deterministic. ---- */
int gs_l1_loss_workspace_bytes(int64_t n, size_t* out);
int gs_l1_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace,
               size_t workspace_bytes, void* stream);

/* Mask loss, BCE form (train.py:146-148, mask_loss_type = 'bce'; the 'l1' form is gs_l1_loss):
 * loss[0] = mean of binary_cross_entropy(clamp(x, 1e-3, 1 - 1e-3), y), dL_dx its gradient w.r.t. x (zero where the
 * clamp is active).  Workspace: gs_l1_loss_workspace_bytes(n). */
int gs_bce_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace,
                size_t workspace_bytes, void* stream);

/* SSIM half of row N2: utils/loss_utils.py:27-67 `ssim(img1, img2)` (window 11, sigma 1.5, zero padding,
 * C1 = 0.01^2, C2 = 0.03^2, mean over all C*H*W elements; train.py:123 uses 1 - ssim as the D-SSIM loss).
 * gs_ssim_forward writes ssim_out[0] and, when the three map pointers are non-NULL (all or none), the
 * per-element partial derivatives of the SSIM map w.r.t. the window mean, variance and covariance, each
 * C*H*W floats.  gs_ssim_backward turns them into dL/dimg1 given the device scalar dL/dssim. ---- */
int gs_ssim_workspace_bytes(int32_t C, int32_t H, int32_t W, size_t* out);
int gs_ssim_forward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_out,
                    float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* workspace, size_t workspace_bytes,
                    void* stream);
int gs_ssim_backward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* dm_dmu1,
                     const float* dm_dsigma1_sq, const float* dm_dsigma12, const float* dL_dssim, float* dL_dimg1,
                     void* stream);

/* ---- K nearest neighbours: pytorch3d.ops.knn_points as the reference calls it
 * (utils/loss_utils.py:76-79,92-96: K = 5 / 6 self-KNN of the canonical Gaussians for the AIAP loss;
 * models/deformer/rigid.py:43: nearest SMPL vertex, K = 1).  For every query the K (<= 8) nearest points of
 * `ref`: squared distances ascending and their indices into `ref` (ties: smaller index first; -1 / FLT_MAX when
 * ref has fewer than K points).  A query that is itself in `ref` is returned as its own first neighbour, as
 * pytorch3d does.  Exact (no approximation).  Workspace: knn_workspace_bytes(Nr). ---- */
int knn_points(int32_t Nq, const float* queries, int32_t Nr, const float* ref, int32_t K, float* dists, int64_t* idx,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---- training-step bookkeeping after the backward pass.
 * gs_densify_stats: train.py:219-220 + scene/gaussian_model.py:464-466, for every Gaussian with radii > 0:
 *   max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |viewspace_grad[:2]|; denom += 1
 *   (viewspace_grad is the (N,3) gradient of the screen-space points the rasterizer returns for means2D).
 * gs_adam_step: torch.optim.Adam as scene/gaussian_model.py:201-216 sets it up (one learning rate per tensor,
 *   shared betas / eps, no weight decay, no amsgrad), step number `step` >= 1, all tensors in ONE launch;
 *   exp_avg / exp_avg_sq are the optimizer's state tensors and are updated in place, as is param. ---- */
#define GS_ADAM_MAX_TENSORS 16
typedef struct GsAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;   /* elements */
    float lr;
} GsAdamTensor;
int gs_densify_stats(int32_t N, const int32_t* radii, const float* viewspace_grad, float* max_radii2D,
                     float* xyz_gradient_accum, float* denom, void* stream);
int gs_adam_step(int32_t n_tensors, const GsAdamTensor* tensors, double beta1, double beta2, double eps, int64_t step,
                 void* stream);

/* ---- the converter's optimizer step (models/gaussian_converter.py:22-39,61-67): clip_grad_norm_ + torch.optim.Adam
 * with per-group weight decay over ~130 parameter tensors, in a handful of launches, with no host synchronisation and a
 * step number that may live on the device (so that the step can be captured into a hipGraph).
 *
 * gs_grad_norm: the global L2 norm of all `tensors` (fp32, contiguous; any alignment).  Every workgroup sums the squares
 *   of one fixed chunk of one tensor into a partial in `workspace` (gs_grad_norm_workspace_bytes of the SAME tensor
 *   list); one workgroup adds the partials in a fixed order.  No atomics: the same gradients give the same bits on
 *   every run.  out[0] = total_norm, out[1] = clip_coef = max_norm / (total_norm + 1e-6) limited to 1 the way
 *   torch.clamp(max=1.0) limits it: a NaN norm gives a NaN coefficient (and an infinite one gives 0).
 * gs_grad_scale: grad *= *clip_coef in place, for the stand-alone clip_grad_norm_.
 * gs_adam_step_ex: gs_adam_step's arithmetic on the effective gradient  *clip_coef * grad + weight_decay * param
 *   (torch's Adam, not AdamW; clip_coef == NULL means 1).  THE GRADIENTS ARE NOT REWRITTEN: after the call they still hold
 *   the unclipped values (torch.nn.utils.clip_grad_norm_ scales them in place; gs_grad_scale does that where it is wanted).
 *   Per tensor: `step` == NULL takes the call's host `step` (>= 1); otherwise `step` points to the tensor's device-resident
 *   fp32 step number, which the call increments by one (in a launch of its own, in front of the update; also for a tensor
 *   with n == 0, whose update is skipped) and then reads: every workgroup forms 1 - beta1^step and sqrt(1 - beta2^step) in
 *   double and rounds them to fp32 once, as the host does for a host step.  `lr_dev` == NULL takes `lr`; otherwise the
 *   learning rate is read from that device fp32 scalar (torch's convention for capturable optimizers: a scheduler's
 *   change is seen by a replayed graph).
 * The tensor tables travel to the kernels by value in batches of GS_GRAD_NORM_BATCH / GS_ADAM_EX_BATCH (kernel
 * arguments are limited to 4 KB); the entry points take up to GS_OPTIM_MAX_TENSORS tensors and loop over the batches.
 * GS_E_BAD_ARG (before any HIP call): a count outside 0..GS_OPTIM_MAX_TENSORS, a NULL table with a positive count, a
 * negative n, a NULL pointer of a tensor with n > 0, NULL out / workspace / clip_coef (gs_grad_scale), a negative or NaN
 * max_norm, step < 1 while some tensor has no device step.  GS_E_TOO_LARGE: a tensor of 2^41 elements or more.
 * GS_E_WORKSPACE: the workspace is smaller than gs_grad_norm_workspace_bytes says.  Zero tensors: GS_OK with nothing
 * enqueued (`out` is then left as it is; tensors that are all empty give total_norm = 0, clip_coef = 1).  All four are capture-safe when every step number is device-resident; gs_adam_step_ex with
 * a host step number on a capturing stream answers GS_E_CAPTURE with nothing enqueued. ---- */
#define GS_OPTIM_MAX_TENSORS 4096
#define GS_GRAD_NORM_BATCH 192  /* tensors per launch of the norm / scale kernels  */
#define GS_ADAM_EX_BATCH 48     /* tensors per launch of the extended Adam update   */
#define GS_ADAM_STEP_BATCH 384  /* device step numbers per launch of the begin-step pass */
typedef struct GsGradTensor {
    float* grad;
    int64_t n;   /* elements */
} GsGradTensor;
typedef struct GsAdamTensorEx {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;            /* elements */
    float lr;             /* used when lr_dev == NULL */
    float weight_decay;
    float* step;          /* device fp32 step number, incremented by the call; NULL: the call's host `step` */
    const float* lr_dev;  /* device fp32 learning rate; NULL: `lr` */
} GsAdamTensorEx;
int gs_grad_norm_workspace_bytes(int32_t n_tensors, const GsGradTensor* tensors, size_t* out);
int gs_grad_norm(int32_t n_tensors, const GsGradTensor* tensors, float max_norm, float* out, void* workspace,
                 size_t workspace_bytes, void* stream);
int gs_grad_scale(int32_t n_tensors, const GsGradTensor* tensors, const float* clip_coef, void* stream);
int gs_adam_step_ex(int32_t n_tensors, const GsAdamTensorEx* tensors, double beta1, double beta2, double eps, int64_t step,
                    const float* clip_coef, void* stream);

/* ---- densification cycle (scene/gaussian_model.py:263-266,311-462; train.py:217-227): clone, split and prune with the
 * Adam-state surgery, and reset_opacity.  The full semantics are spelled out at the top of csrc/densify.hip.
 * gs_densify_plan: classifies the N sources (clone / split / prune, or prune by `prune_mask` alone), and builds in
 *   `workspace` (gs_densify_workspace_bytes(N) bytes) the destination -> source map of the result and its row count N'.
 *   N' stays on the device; if `count_host_pinned` is non-NULL it is also copied there (HOST-pinned int32, same stream;
 *   the caller synchronises before reading it).  Workspace byte 0..N-1 = the per-source GS_DENSIFY_F_* flags.
 * gs_densify_apply: writes every output tensor of the cycle in ONE launch, by destination row: dst [N_new, width] from
 *   src [N, width] through the plan's map, per the tensor's kind.  `N_new` is the plan's N' (rows past the plan's own
 *   count are written as zeros).  A GS_DENSIFY_CHILD_POSITION tensor (xyz, width 3) also reads `scaling` [N,3],
 *   `rotation` [N,4] and `noise` [N,2,3] (standard-normal z of the two children of every source; only split sources'
 *   rows are read); a GS_DENSIFY_CHILD_SCALING tensor has width 3.  dst must not alias any source.
 * gs_reset_opacity: opacity_out = logit(min(sigmoid(opacity_in), 0.01)) (in place allowed); exp_avg / exp_avg_sq (each
 *   NULL or [N]) are zeroed.
 * N = 0 and N' = 0 are legal (nothing to write).  The library allocates nothing. ---- */
#define GS_DENSIFY_MAX_TENSORS 24
#define GS_DENSIFY_COPY 0            /* dst row = src row of its source (a clone or child copies its source's row)        */
#define GS_DENSIFY_ZERO_IF_NEW 1     /* an Adam moment: surviving originals copy, clones and children start at zero      */
#define GS_DENSIFY_ZERO 2            /* a statistic: zeros of the new N (src may be NULL)                                 */
#define GS_DENSIFY_CHILD_POSITION 3  /* xyz: children get R(normalize(q)) (z (.) exp(scaling)) + xyz                      */
#define GS_DENSIFY_CHILD_SCALING 4   /* scaling: children get log(exp(s) / 1.6)                                           */
#define GS_DENSIFY_F_KEEP 1          /* flags: the original row survives                                                  */
#define GS_DENSIFY_F_CLONE 2         /* selected for cloning                                                              */
#define GS_DENSIFY_F_SPLIT 4         /* selected for splitting                                                            */
#define GS_DENSIFY_F_PRUNE 8         /* the source's own values are pruned (its row, and its clone's)                     */
#define GS_DENSIFY_F_CHILD_PRUNE 16  /* its children are pruned                                                           */
#define GS_DENSIFY_F_CLONE_KEPT 32
#define GS_DENSIFY_F_CHILDREN_KEPT 64
typedef struct GsDensifyPlan {
    int32_t N;
    const float* scaling;      /* [N,3] log scales */
    const float* opacity;      /* [N] logits */
    const float* grad_accum;   /* [N] xyz_gradient_accum (densify mode) */
    const float* denom;        /* [N] (densify mode) */
    const uint8_t* prune_mask; /* NULL: densify mode.  Else prune_points(mask): rows with mask != 0 go, nothing is added,
                                * and scaling / opacity / grad_accum / denom are not read (may be NULL) */
    float grad_threshold;      /* (float) opt.densify_grad_threshold */
    float split_scale;         /* (float)(percent_dense * extent), the product taken in double */
    float min_opacity;         /* (float) opt.opacity_threshold */
    float max_world_scale;     /* (float)(0.1 * extent) */
    float max_screen_size;     /* (float) max_screen_size */
    int32_t prune_size;        /* max_screen_size is set (truthy): the world-size and screen-size prune tests apply */
} GsDensifyPlan;
typedef struct GsDensifyTensor {
    const float* src; /* [N, width] */
    float* dst;       /* [N_new, width] */
    int32_t width;    /* floats per row, > 0 */
    int32_t kind;     /* GS_DENSIFY_* */
} GsDensifyTensor;
int gs_densify_workspace_bytes(int32_t N, size_t* out);
int gs_densify_plan(const GsDensifyPlan* plan, void* workspace, size_t workspace_bytes, int32_t* count_host_pinned,
                    void* stream);
int gs_densify_apply(int32_t N, int32_t N_new, const void* workspace, size_t workspace_bytes, int32_t n_tensors,
                     const GsDensifyTensor* tensors, const float* scaling, const float* rotation, const float* noise,
                     void* stream);
int gs_reset_opacity(int32_t N, const float* opacity_in, float* opacity_out, float* exp_avg, float* exp_avg_sq,
                     void* stream);

/* ---- as-isometric-as-possible regularisers (utils/loss_utils.py:69-102; train.py:163-171): per set,
 * L = mean over the pairs (i, idx[i, k]), k = 1 .. K-1, of | |xc_i - xc_j| - |xd_i - xd_j| |, and its gradients w.r.t.
 * xc and xd.  The full semantics are spelled out at the top of csrc/aiap.hip.  One or two sets share one neighbour list
 * (full_aiap_loss: positions, D = 3, and strip_symmetric covariances, D = 6).
 * gs_aiap_forward: writes every set's loss[0] (device float) and builds in `workspace` (gs_aiap_workspace_bytes(N, K,
 *   n_sets) bytes) the stable reverse adjacency of idx that gs_aiap_backward reuses: call the backward with the same
 *   N, K, idx, sets and workspace.  idx is [N, K] int64, contiguous; a value of columns 1 .. K-1 outside [0, N) is never
 *   dereferenced (the pair adds nothing) and is counted: workspace word 0 (uint32) holds the count after the forward.
 * gs_aiap_backward: writes every non-NULL dL_dxc / dL_dxd [N, D] row exactly once (no atomics: bitwise reproducible),
 *   scaled by the device scalar dL_dloss (NULL = 1).
 * Rows are read and written with 4-byte accesses: xc, xd and the gradients need only fp32 alignment.
 * GS_E_BAD_ARG: N < 1, K < 2, K > 8, n_sets not 1 or 2, a D not 3 or 6, N (K - 1) >= 2^31, or a NULL required pointer
 * (idx, sets, workspace, xc, xd; loss in the forward).  GS_E_WORKSPACE: the workspace is too small. ---- */
typedef struct GsAiapSet {
    const float* xc;       /* [N, D] canonical */
    const float* xd;       /* [N, D] deformed */
    int32_t D;             /* 3 or 6 */
    float* loss;           /* forward: device float */
    const float* dL_dloss; /* backward: device float, NULL = 1 */
    float* dL_dxc;         /* backward: [N, D] or NULL (not wanted) */
    float* dL_dxd;         /* backward: [N, D] or NULL */
} GsAiapSet;
int gs_aiap_workspace_bytes(int32_t N, int32_t K, int32_t n_sets, size_t* out);
int gs_aiap_forward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets, void* workspace,
                    size_t workspace_bytes, void* stream);
int gs_aiap_backward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets,
                     const void* workspace, size_t workspace_bytes, void* stream);

/* ---- multiresolution hash-grid encoding (tcnn.Encoding(3, {"otype": "HashGrid", ...}) of the reference's non-rigid
 * deformer, models/network_utils.py:329-343): 3-D input, linear interpolation, fp32 parameters and arithmetic.  The full
 * semantics (level table, cell, corner index, weights, gradients) are spelled out at the top of csrc/hashgrid.hip.
 * gs_hashgrid_levels: host only (no device, no stream).  Fills offsets[L + 1] (the first table row of every level, in rows
 *   of F features; offsets[L] = the number of rows), scales[L] (the float32 scale_l the kernels use), resolutions[L] and
 *   *n_params = offsets[L] * F; any of the four may be NULL.
 * gs_hashgrid_forward: out [N, L F] fp32, row-major, from x [N, 3] fp32 and params [n_params] fp32.
 * gs_hashgrid_backward: from dL_dout [N, L F]: dL_dx [N, 3] (gather only: every row written once) and dL_dparams
 *   [n_params] (every element written exactly once, 0 where no point reaches it; no atomics: bitwise reproducible).
 *   Either may be NULL (not wanted); `workspace` (gs_hashgrid_workspace_bytes) is needed only with dL_dparams, params
 *   only with dL_dx.  The forward and the backward are independent: the backward keeps nothing from the forward.
 * x needs fp32 alignment; params, out, dL_dout and dL_dparams need 4 min(F, 4)-byte alignment.
 * GS_E_BAD_ARG: a NULL required pointer or grid, N < 0, a misaligned pointer, or a config outside: 1 <= n_levels <=
 * GS_HASHGRID_MAX_LEVELS, n_features_per_level in {1, 2, 4, 8}, 1 <= log2_hashmap_size <= 30, base_resolution >= 1,
 * 1 <= per_level_scale <= 1e4.  GS_E_TOO_LARGE: n_params >= 2^31 or a level's resolution beyond 32 bits; N L >= 2^31 (forward);
 * 8 L N >= 2^31 with dL_dparams (the sort's 32-bit pair index).  GS_E_WORKSPACE: the workspace is too small. ---- */
#define GS_HASHGRID_MAX_LEVELS 32
typedef struct GsHashGrid {
    int32_t n_levels;             /* L */
    int32_t n_features_per_level; /* F */
    int32_t log2_hashmap_size;    /* T */
    int32_t base_resolution;      /* N0 */
    float per_level_scale;        /* b (float32, as tcnn's host code reads it) */
} GsHashGrid;
int gs_hashgrid_levels(const GsHashGrid* grid, int32_t* offsets, float* scales, int32_t* resolutions, int32_t* n_params);
int gs_hashgrid_workspace_bytes(const GsHashGrid* grid, int32_t N, size_t* out);
int gs_hashgrid_forward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, float* out, void* stream);
int gs_hashgrid_backward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, const float* dL_dout,
                         float* dL_dx, float* dL_dparams, void* workspace, size_t workspace_bytes, void* stream);

/* ---- linear blend skinning of the rigid deformer (models/deformer/rigid.py: SkinningField.forward with its
 * hierarchical_softmax / F.softmax, SMPLNN.forward with given weights; build_rotation at utils/general_utils.py:87-108).
 * The full semantics (the three weight kinds, T_fwd, x_bar, R_bar and every gradient) are spelled out at the top of
 * csrc/skinning.hip.  All arrays are fp32, row-major, contiguous.  `w` is [N, 25] logits (GS_SKIN_HIERARCHICAL), [N, 24]
 * logits (GS_SKIN_SOFTMAX) or [N, 24] weights (GS_SKIN_WEIGHTS); tfs [24, 4, 4] (camera.bone_transforms); xyz [N, 3];
 * rotation [N, 4] raw (w,x,y,z) quaternions (normalised inside, no epsilon).
 * gs_skin_weights_forward / _backward: the activation alone (kind 0 or 1): weights [N, 24] from logits, and dL_dlogits
 *   from dL_dweights [N, 24].
 * gs_skinning_forward: xyz_out [N, 3] = T[:3,:3] x + T[:3,3], rotation_out [N, 3, 3] = T[:3,:3] R(q), T_fwd [N, 4, 4] =
 *   sum_j W_j tfs_j.
 * gs_skinning_backward: from dL_dxyz_out [N, 3] and dL_drotation_out [N, 3, 3] (either NULL = zero): dL_dw (shaped as
 *   w), dL_dtfs [24, 4, 4] (rows 3 are 0), dL_dxyz [N, 3] (the direct term T[:3,:3]^T g) and dL_drotation [N, 4]; any
 *   of the four may be NULL (not wanted).  Every row is written exactly once and dL_dtfs is summed in a fixed order
 *   (no atomics: bitwise reproducible).  `workspace` (gs_skinning_workspace_bytes(N)) is needed only with dL_dtfs.  The
 *   backward recomputes everything from its inputs: it keeps nothing from the forward.
 * Alignment: w, dL_dw, weights, dL_dweights, dL_dlogits, tfs, rotation, rotation_out, dL_drotation, xyz_out and T_fwd
 * need 16 bytes (16-byte accesses); the other arrays fp32 alignment.  N = 0 touches nothing (dL_dtfs included).
 * GS_E_BAD_ARG (before any HIP call): N < 0, an unknown kind (GS_SKIN_WEIGHTS in gs_skin_weights_*), a NULL required
 * pointer or a misaligned one.  GS_E_WORKSPACE: the workspace is smaller than gs_skinning_workspace_bytes(N). ---- */
#define GS_SKIN_BONES 24
enum { GS_SKIN_HIERARCHICAL = 0 /* 25 logits */, GS_SKIN_SOFTMAX = 1 /* 24 logits */, GS_SKIN_WEIGHTS = 2 /* 24 weights */ };
int gs_skin_weights_forward(int32_t N, int32_t kind, const float* logits, float* weights, void* stream);
int gs_skin_weights_backward(int32_t N, int32_t kind, const float* logits, const float* dL_dweights, float* dL_dlogits,
                             void* stream);
int gs_skinning_workspace_bytes(int32_t N, size_t* out);
int gs_skinning_forward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                        float* xyz_out, float* rotation_out, float* T_fwd, void* stream);
int gs_skinning_backward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                         const float* dL_dxyz_out, const float* dL_drotation_out, float* dL_dw, float* dL_dtfs,
                         float* dL_dxyz, float* dL_drotation, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the rigid deformer's skinning regulariser (models/deformer/rigid.py: SkinningField.sample_skinning_loss and
 * get_skinning_loss; AABB.normalize at utils/dataset_utils.py:72-76): surface samples of the canonical mesh with their
 * blended skinning weights, and the mean over rows of the summed squared error between the activated logits and those
 * weights.  The full semantics (face pick, the fold of the barycentric draws, the summation orders, the gradient) are
 * spelled out at the top of csrc/skinloss.hip.  All arrays are contiguous, row-major device arrays.
 * gs_mesh_sample: n samples from draws [n, 3] (fp32 uniforms in [0, 1): the caller's random stream) on the mesh verts
 *   [V, 3] fp32, faces [F, 3] int32, with cdf [F] fp32 the non-decreasing cumulative face areas (cdf[F-1] the total) and
 *   vweights [V, 24] fp32 the vertices' skinning weights; aabb_min [3] and aabb_inv_extent [3] fp32.  Writes points_norm
 *   [n, 3] (the samples in the box's [-1, 1] coordinates) and target [n, 24]; face [n] int32, bary [n, 3] and points
 *   [n, 3] (unnormalised) are optional (NULL = not wanted).  Vertex indices outside [0, V) are clamped into it.
 * gs_skin_loss_forward: loss [1] = sum_i sum_j (W_ij - target_ij)^2 / n with W the activation of logits ([n, 25]
 *   GS_SKIN_HIERARCHICAL or [n, 24] GS_SKIN_SOFTMAX) and target [n, 24]; summed in a fixed order in double through
 *   `workspace` (gs_skin_loss_workspace_bytes(n): one double per block of 256 rows).
 * gs_skin_loss_backward: dL_dlogits (shaped as logits) from dL_dloss [1], a DEVICE scalar; recomputes W, keeps nothing
 *   from the forward, writes every row once.  The target gets no gradient.
 * n = 0 enqueues nothing and leaves `loss` as it is (the Python layer returns 0, not torch's nan for an empty mean).
 * Alignment: logits, dL_dlogits, target, vweights, points_norm, bary, points and the workspace need 16 bytes; the other
 * arrays their element's.  GS_E_BAD_ARG (before any HIP call): n < 0, V < 1, F < 1, an unknown kind (GS_SKIN_WEIGHTS
 * included), a NULL required pointer or a misaligned one.  GS_E_WORKSPACE: the workspace is smaller than
 * gs_skin_loss_workspace_bytes(n). ---- */
int gs_mesh_sample(int32_t n, int32_t V, int32_t F, const float* verts, const int32_t* faces, const float* cdf,
                   const float* vweights, const float* aabb_min, const float* aabb_inv_extent, const float* draws,
                   float* points_norm, float* target, int32_t* face, float* bary, float* points, void* stream);
int gs_skin_loss_workspace_bytes(int32_t n, size_t* out);
int gs_skin_loss_forward(int32_t n, int32_t kind, const float* logits, const float* target, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
int gs_skin_loss_backward(int32_t n, int32_t kind, const float* logits, const float* target, const float* dL_dloss,
                          float* dL_dlogits, void* stream);

/* ---- SMPL pose correction of `pose_correction: direct` (models/pose_correction/pose_correction.py:
 * DirectPoseOptimization.pose_correct through PoseCorrection._forward_smpl, get_transforms_02v and
 * models/pose_correction/lbs.py), batch 1, 24 joints.  The full semantics (rest joints, shape statistics, Rodrigues, the
 * kinematic chain, the star-pose transforms, the loss and every gradient) are spelled out at the top of csrc/pose.hip.
 * All arrays are fp32, row-major, contiguous device arrays; `parents` travels by value (host int32; entry 0 is ignored).
 * GsPoseArgs: v_template [V, 3], shapedirs [V, 3, NB], J_template [24, 3] = J_regressor v_template and J_shapedirs
 *   [24, 3, NB] = J_regressor shapedirs (folded once by the caller); betas [NB], root_orient [3], pose_body [63],
 *   pose_hand [6], trans [3]; rots_gt [24, 9] or NULL (no loss).
 * gs_pose_forward (two launches): rots [24, 9] (row 0 the identity), Jtrs [24, 3], bone_transforms [24, 4, 4], loss_pose
 *   (one float; required with rots_gt, else ignored), and `state` (GS_POSE_STATE_FLOATS floats) for the backward.
 *   `workspace`: gs_pose_workspace_bytes(V) bytes, 8-byte aligned (the per-block partials of the vertex pass).
 * gs_pose_backward (one launch; reads `state`, never the vertices; of GsPoseArgs it uses NB, parents, J_shapedirs,
 *   root_orient, pose_body, pose_hand and rots_gt): from dL_drots [24, 9], dL_dJtrs [24, 3], dL_dbone_transforms
 *   [24, 4, 4] (rows 3 ignored) and dL_dloss_pose (one DEVICE float), any of them NULL = zero, to dL_dbetas [NB],
 *   dL_droot_orient [3], dL_dpose_body [63], dL_dpose_hand [6], dL_dtrans [3], any of them NULL = not wanted.  Every sum
 *   has one fixed order (no atomics: bitwise reproducible).
 * GS_E_BAD_ARG (before any HIP call): a NULL args, V < 1, NB outside 1..GS_POSE_MAX_BETAS, parents[i] outside
 * 0..i-1 for some i >= 1, a NULL required pointer or a misaligned one (fp32 alignment; the workspace 8 bytes).
 * GS_E_WORKSPACE: the workspace is smaller than gs_pose_workspace_bytes(V). ---- */
#define GS_POSE_BONES 24
#define GS_POSE_MAX_BETAS 16
#define GS_POSE_STATE_FLOATS 512
typedef struct GsPoseArgs {
    int32_t V, NB;
    int32_t parents[GS_POSE_BONES];
    const float *v_template, *shapedirs, *J_template, *J_shapedirs;
    const float *betas, *root_orient, *pose_body, *pose_hand, *trans;
    const float* rots_gt;
} GsPoseArgs;
int gs_pose_workspace_bytes(int32_t V, size_t* out);
int gs_pose_forward(const GsPoseArgs* a, float* rots, float* Jtrs, float* bone_transforms, float* loss_pose, float* state,
                    void* workspace, size_t workspace_bytes, void* stream);
int gs_pose_backward(const GsPoseArgs* a, const float* state, const float* dL_drots, const float* dL_dJtrs,
                     const float* dL_dbone_transforms, const float* dL_dloss_pose, float* dL_dbetas, float* dL_droot_orient,
                     float* dL_dpose_body, float* dL_dpose_hand, float* dL_dtrans, void* stream);

/* ---- the non-rigid deformer around its MLP (models/deformer/non_rigid.py MLP / HashGridwithMLP): the hierarchical pose
 * encoder in front of it (models/network_utils.py HierarchicalPoseEncoder.forward, rel_joints = False, batch 1, 24
 * joints) and the application of the MLP's output behind it.  The full semantics, every gradient included, are spelled
 * out at the top of csrc/nonrigid.hip.  All arrays are fp32, row-major, contiguous.
 *
 * GsPoseEncArgs: d = dim_per_joint in 1..GS_POSE_ENC_MAX_DIM (m = 13 + d); the kinematic tree by value (parents[i] < i
 *   for i >= 1, entry 0 ignored); rots [24, 9], Jtrs [24, 3]; and the ADDRESSES of the 98 parameter tensors, nn.Linear
 *   layouts: W0 [d, 288], b0 [d], W1[j] [m, m], b1[j] [m], W2[j] [d, m], b2[j] [d].  The struct is handed to the kernel
 *   by value: there is no pointer table in device memory.
 * gs_pose_encoder_forward (one launch, one workgroup): out [24 d] (the out_j in joint order) and `state`
 *   (GS_POSE_ENC_STATE_FLOATS floats: in_j and h_j) for the backward.
 * gs_pose_encoder_backward (one launch, one workgroup; reads `state`, the parameters, d and parents): from dL_dout
 *   [24 d] to dL_dparams (gs_pose_encoder_grad_floats(d) floats, packed W0 | b0 | (W1_j | b1_j | W2_j | b2_j) for
 *   j = 0..23), dL_drots [24, 9] and dL_dJtrs [24, 3], any of the three NULL = not wanted.  Every sum has one fixed
 *   order: bitwise reproducible.
 *
 * gs_nonrigid_apply_forward (one launch, plus one of three workgroups with `losses`): deltas [N, D], D = 10 + F in
 *   10..GS_NONRIGID_MAX_D, xyz [N, 3], scaling [N, 3], rotation [N, 4] -> xyz_out, scaling_out, rotation_out, feature
 *   [N, F] (required when F > 0) and losses [3] = (nr_xyz, nr_scale, nr_rot) (NULL = not wanted; then no workspace is
 *   needed).  scale_offset: GS_NR_SCALE_*; rot_offset: GS_NR_ROT_*.  With GS_NR_SCALE_ZERO `scaling` and `scaling_out`
 *   may both be NULL (scaling' is scaling itself).  `deltas` is never written (the reference overwrites its column 6
 *   with 1 in GS_NR_ROT_MULT mode).  `workspace`: gs_nonrigid_workspace_bytes(N, D) bytes.
 * gs_nonrigid_apply_backward (one launch): from dL_dxyz_out, dL_dscaling_out, dL_drotation_out, dL_dfeature and the three
 *   DEVICE floats dL_dnr_xyz, dL_dnr_scale, dL_dnr_rot, any of them NULL = zero, to dL_ddeltas [N, D] (every element
 *   written, zeros included), dL_dscaling and dL_drotation, any of them NULL = not wanted.  dL/dxyz is dL_dxyz_out.
 * N == 0 does nothing.  GS_E_BAD_ARG (before any HIP call): a NULL args, d outside 1..GS_POSE_ENC_MAX_DIM, parents[i]
 * outside 0..i-1 for some i >= 1, N < 0, D outside 10..GS_NONRIGID_MAX_D, an unknown mode, a NULL required pointer or a
 * misaligned one (16 bytes for deltas, rotation, rotation_out, feature and their gradients, else fp32 alignment).
 * GS_E_WORKSPACE: the workspace is smaller than gs_nonrigid_workspace_bytes(N, D). ---- */
#define GS_POSE_ENC_JOINTS 24
#define GS_POSE_ENC_MAX_DIM 16
#define GS_POSE_ENC_STATE_FLOATS 1392
typedef struct GsPoseEncArgs {
    int32_t d;
    int32_t parents[GS_POSE_ENC_JOINTS];
    const float *rots, *Jtrs;
    const float *W0, *b0;
    const float* W1[GS_POSE_ENC_JOINTS];
    const float* b1[GS_POSE_ENC_JOINTS];
    const float* W2[GS_POSE_ENC_JOINTS];
    const float* b2[GS_POSE_ENC_JOINTS];
} GsPoseEncArgs;
int gs_pose_encoder_grad_floats(int32_t d, size_t* out);
int gs_pose_encoder_forward(const GsPoseEncArgs* a, float* out, float* state, void* stream);
int gs_pose_encoder_backward(const GsPoseEncArgs* a, const float* state, const float* dL_dout, float* dL_dparams,
                             float* dL_drots, float* dL_dJtrs, void* stream);
#define GS_NONRIGID_MAX_D 2048
#define GS_NR_SCALE_LOGIT 0
#define GS_NR_SCALE_EXP 1
#define GS_NR_SCALE_ZERO 2
#define GS_NR_ROT_ADD 0
#define GS_NR_ROT_MULT 1
int gs_nonrigid_workspace_bytes(int32_t N, int32_t D, size_t* out);
int gs_nonrigid_apply_forward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                              const float* xyz, const float* scaling, const float* rotation, float* xyz_out,
                              float* scaling_out, float* rotation_out, float* feature, float* losses, void* workspace,
                              size_t workspace_bytes, void* stream);
int gs_nonrigid_apply_backward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                               const float* scaling, const float* rotation, const float* dL_dxyz_out,
                               const float* dL_dscaling_out, const float* dL_drotation_out, const float* dL_dfeature,
                               const float* dL_dnr_xyz, const float* dL_dnr_scale, const float* dL_dnr_rot,
                               float* dL_ddeltas, float* dL_dscaling, float* dL_drotation, void* stream);

/* ---- the input of the ColorMLP texture (models/texture/texture.py ColorMLP.compose_input): the [N, D] matrix the
 * colour MLP reads, composed in one launch, and its backward in one launch (plus one small fixed-order sum for the
 * latent code).  The full semantics, every gradient included, are spelled out at the top of csrc/texture.hip.  All
 * arrays are fp32, row-major, contiguous.  The columns of `inp`:
 *   [ before[0] | .. | before[n_before-1] | sh_embed | after[0] | .. | after[n_after-1] | latent ]
 * before[b] [N, before_w[b]] and after[a] [N, after_w[a]] are copied into place; sh_embed is the (sh_degree + 1)^2 - 1
 * spherical-harmonics bases above the constant one (utils/sh_utils.py eval_sh_bases(..)[..., 1:]; none at degree 0) of
 * the unit view direction of models/texture/texture.py:90-101: d = xyz - campos; with fwd_transform, d = R^T d, R the
 * 3x3 of row n read in place at fwd_transform + n rot_stride, its rows rot_row floats apart ((N, 4, 4): 16 and 4;
 * (N, 3, 3): 9 and 3); with use_noise, d = d @ noise (row-major, by value); unit = d / (|d| + 1e-12).  latent [latent_dim]
 * is one row broadcast to every row.  D = the sum of the widths, at most GS_TEXTURE_MAX_D.  The struct is handed to the
 * kernels by value.
 * gs_texture_input_forward: a -> inp [N, D].
 * gs_texture_input_backward: from dL_dinp [N, D] to dL_dbefore[b] / dL_dafter[a] (host arrays of n_before / n_after device
 *   addresses, the array or any entry NULL = not wanted), dL_dxyz [N, 3] (sh_degree > 0 only) and dL_dlatent [latent_dim]
 *   (the column sums: per-workgroup partials in `workspace`, gs_texture_workspace_bytes(N, D, latent_dim) bytes, summed in a
 *   fixed order: bitwise reproducible), any of them NULL = not wanted and then not computed.  fwd_transform, campos and
 *   noise take no gradient.  Reads of `a`: the widths, and for dL_dxyz what the direction is made of.
 * N == 0 does nothing.  GS_E_BAD_ARG (before any HIP call): a NULL args, N < 0, sh_degree outside 0..4, n_before over
 * GS_TEXTURE_MAX_BEFORE, n_after over GS_TEXTURE_MAX_AFTER, a width below 1, latent_dim < 0, D over the cap or not the sum
 * of the widths, a NULL required pointer or a misaligned one (16 bytes for inp, the blocks and their gradients, else fp32
 * alignment), rot_row < 3 or rot_stride < 2 rot_row + 3 with a fwd_transform, dL_dxyz at sh_degree 0, dL_dlatent at
 * latent_dim 0.  GS_E_WORKSPACE: dL_dlatent with a workspace smaller than gs_texture_workspace_bytes says. ---- */
#define GS_TEXTURE_MAX_D 512
#define GS_TEXTURE_MAX_BEFORE 6
#define GS_TEXTURE_MAX_AFTER 2
typedef struct GsTextureArgs {
    int32_t N, D;
    int32_t sh_degree;
    int32_t n_before, n_after;
    int32_t before_w[GS_TEXTURE_MAX_BEFORE];
    int32_t after_w[GS_TEXTURE_MAX_AFTER];
    int32_t latent_dim;
    int32_t rot_stride, rot_row;
    int32_t use_noise;
    float noise[9];
    const float* before[GS_TEXTURE_MAX_BEFORE];
    const float* after[GS_TEXTURE_MAX_AFTER];
    const float *xyz, *campos, *fwd_transform, *latent;
} GsTextureArgs;
int gs_texture_workspace_bytes(int32_t N, int32_t D, int32_t latent_dim, size_t* out);
int gs_texture_input_forward(const GsTextureArgs* a, float* inp, void* stream);
int gs_texture_input_backward(const GsTextureArgs* a, const float* dL_dinp, float* const* dL_dbefore, float* const* dL_dafter,
                              float* dL_dxyz, float* dL_dlatent, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the dense networks (models/network_utils.py VanillaCondMLP :182-249) as one fused op on the exact-fp32 MFMA:
 * y = L_{nl-1}(leaky(.. leaky(L_0([x | cond])) ..)), n_hidden hidden layers of one width, nl = n_hidden + 1 nn.Linear
 * layers, LeakyReLU of `slope` between them and none after the last.  The full semantics, every gradient included, are
 * spelled out at the top of csrc/mlp.hip.  All arrays are fp32, row-major, contiguous.
 *
 * GsMlpArgs (handed to the kernels by value: there is no pointer table in device memory): N rows; dim_in in
 *   1..GS_MLP_MAX_IN; dim_cond in 0..GS_MLP_MAX_COND; width a multiple of 32 in 32..GS_MLP_MAX_WIDTH; n_hidden in
 *   1..GS_MLP_MAX_HIDDEN; dim_out in 1..GS_MLP_MAX_OUT; x [N, dim_in] (16-byte aligned); cond [dim_cond], ONE row shared by
 *   every row of x and never expanded (NULL at dim_cond 0); W[l], b[l] for l = 0..n_hidden: W[0] [width, dim_in + dim_cond],
 *   W[l] [width, width], W[n_hidden] [dim_out, width].  The gradient addresses dW[l], db[l] (shaped as W[l], b[l]), dx
 *   [N, dim_in] and dcond [dim_cond] are read by gs_mlp_backward only; NULL = not wanted, and then neither computed nor
 *   written.
 * gs_mlp_forward (one launch; one small launch in front of it at dim_cond > 0): y [N, dim_out]; acts [n_hidden, N, width]
 *   (16-byte aligned), the hidden post-activations gs_mlp_backward reads, NULL = not saved.  `workspace`:
 *   gs_mlp_workspace_bytes(a, 0) bytes (none at dim_cond 0).
 * gs_mlp_backward (at most three launches): from dL_dy [N, dim_out] (16-byte aligned) and acts to the wanted gradients.
 *   `workspace` (16-byte aligned): gs_mlp_workspace_bytes(a, 1) bytes -- the layers' pre-activation gradients and at most
 *   GS_MLP_MAX_PARTIALS partial parameter gradients, each over max(GS_MLP_PARTIAL_MIN_ROWS, ceil(N / GS_MLP_MAX_PARTIALS)
 *   rounded up to 32) consecutive rows and summed in index order: no atomics, bitwise reproducible, the partition a
 *   function of N alone.  A forward tile is GS_MLP_TILE_ROWS rows.
 * N == 0 does nothing.  GS_E_BAD_ARG (before any HIP call): a NULL args, N < 0, a size outside the ranges above, a NaN
 *   slope, a NULL required pointer or a misaligned one (16 bytes for x, acts, dL_dy and the backward's workspace, else fp32
 *   alignment), dcond at dim_cond 0.  GS_E_WORKSPACE: the workspace is smaller than gs_mlp_workspace_bytes says. ---- */
#define GS_MLP_MAX_WIDTH 128
#define GS_MLP_MAX_HIDDEN 6
#define GS_MLP_MAX_LAYERS 7
#define GS_MLP_MAX_IN 512
#define GS_MLP_MAX_COND 512
#define GS_MLP_MAX_OUT 64
#define GS_MLP_TILE_ROWS 128
#define GS_MLP_PARTIAL_MIN_ROWS 256
#define GS_MLP_MAX_PARTIALS 128
typedef struct GsMlpArgs {
    int32_t N, dim_in, dim_cond, width, n_hidden, dim_out;
    float slope;
    const float *x, *cond;
    const float* W[GS_MLP_MAX_LAYERS];
    const float* b[GS_MLP_MAX_LAYERS];
    float* dW[GS_MLP_MAX_LAYERS];
    float* db[GS_MLP_MAX_LAYERS];
    float *dx, *dcond;
} GsMlpArgs;
int gs_mlp_workspace_bytes(const GsMlpArgs* a, int32_t backward, size_t* out);
int gs_mlp_forward(const GsMlpArgs* a, float* y, float* acts, void* workspace, size_t workspace_bytes, void* stream);
int gs_mlp_backward(const GsMlpArgs* a, const float* acts, const float* dL_dy, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- the LPIPS-VGG perceptual loss (train.py:28,62-64,127-138 `lpips.LPIPS(net='vgg')`; utils/general_utils.py:279-291):
 * the input transform, the thirteen 3x3 convolutions of VGG16 features[0:30] with their four max-pools, and the five
 * normalise / difference / lin / spatial-mean heads, fp32 on the exact-fp32 MFMA, with a backward to the images only.  The
 * full semantics are spelled out at the top of csrc/lpips.hip (recalled from the public packages: neither was available to
 * check against).  Feature maps are channels-last (H, W, C); images are (3, H, W) with a channel stride and a row stride
 * in floats (the pixels of a row are adjacent), so a crop of a larger image is read in place.
 *
 * GsLpipsArgs: H, W in GS_LPIPS_MIN_SIZE..GS_LPIPS_MAX_SIZE; normalize != 0: the images are in [0, 1]; need_grad0 / need_grad1:
 *   whether the forward saves what the backward to in0 / in1 needs (an image without it saves nothing); in0, in1 with
 *   their strides cs* (>= 1) and rs* (>= W); `packed`: what gs_lpips_pack_weights wrote (16-byte aligned).  The parameter
 *   addresses weight[l] (Cout, Cin, 3, 3), bias[l] (Cout), lin[k] (C_k), shift (3), scale (3) -- the last two may be NULL: the
 *   defaults -- are read by gs_lpips_pack_weights only and travel to its kernel by value.
 * gs_lpips_pack_weights: the weights repacked for both directions into `packed` (gs_lpips_packed_bytes), once.
 * gs_lpips_workspace_bytes(H, W, need_grad0, need_grad1, which): which = GS_LPIPS_WS_FORWARD the forward's transient
 *   workspace, GS_LPIPS_WS_SAVED what the forward saves for the backward (0 bytes when neither image needs a gradient),
 *   GS_LPIPS_WS_BACKWARD the backward's transient workspace.
 * gs_lpips_forward: loss[1] and, unless NULL, per_tap[GS_LPIPS_TAPS] (their sum in order is the loss).
 * gs_lpips_backward: d_in0 / d_in1 (3, H, W) contiguous, NULL = not wanted (allowed only for an image whose need_grad is
 *   set); dL_dloss a device scalar, NULL = 1; `saved` as the forward with the same flags left it.
 * gs_lpips_conv: ONE layer (0..GS_LPIPS_LAYERS - 1) of the packed weights on caller-given maps.  backward == 0: out (H, W,
 *   Cout) = relu(conv(in) + bias); layer 0 reads `in` as an image through in_cs / in_rs and transforms it (`normalize`),
 *   every other layer reads (H, W, Cin) and ignores the strides.  backward != 0: out (H, W, Cin) = the backward-data
 *   convolution of `in` (H, W, Cout) masked by `mask` > 0 ((H, W, Cout), the layer's saved output); layer 0 writes the image
 *   gradient (3, H, W), times the transform's factor.  Any H, W >= 1.
 * gs_lpips_pool: backward == 0: out (H / 2, W / 2, C) = the 2x2 max-pool of in (H, W, C); != 0: out (H, W, C) = g + the
 *   gradient dp (H / 2, W / 2, C) routed to the first maximum of every window of `in`.  C a multiple of 4.
 * Every map, `packed`, `saved` and the workspaces are 16-byte aligned.  No atomics, no memsets: bitwise reproducible.
 * GS_E_BAD_ARG (before any HIP call): a NULL args or required pointer, a size outside the range, a stride below its
 *   minimum, a misaligned pointer, a gradient asked for an image whose need_grad is 0.  GS_E_WORKSPACE: a buffer smaller
 *   than gs_lpips_workspace_bytes says. ---- */
#define GS_LPIPS_LAYERS 13
#define GS_LPIPS_TAPS 5
#define GS_LPIPS_MIN_SIZE 16
#define GS_LPIPS_MAX_SIZE 2048
#define GS_LPIPS_WS_FORWARD 0
#define GS_LPIPS_WS_SAVED 1
#define GS_LPIPS_WS_BACKWARD 2
typedef struct GsLpipsArgs {
    int32_t H, W, normalize, need_grad0, need_grad1;
    int64_t cs0, rs0, cs1, rs1;
    const float *in0, *in1, *packed;
    const float* weight[GS_LPIPS_LAYERS];
    const float* bias[GS_LPIPS_LAYERS];
    const float* lin[GS_LPIPS_TAPS];
    const float *shift, *scale;
} GsLpipsArgs;
int gs_lpips_packed_bytes(size_t* out);
int gs_lpips_pack_weights(const GsLpipsArgs* a, void* packed, size_t packed_bytes, void* stream);
int gs_lpips_workspace_bytes(int32_t H, int32_t W, int32_t need_grad0, int32_t need_grad1, int32_t which, size_t* out);
int gs_lpips_forward(const GsLpipsArgs* a, float* loss, float* per_tap, void* saved, size_t saved_bytes, void* workspace,
                     size_t workspace_bytes, void* stream);
int gs_lpips_backward(const GsLpipsArgs* a, const float* dL_dloss, float* d_in0, float* d_in1, const void* saved,
                      size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gs_lpips_conv(const float* packed, int32_t layer, int32_t backward, int32_t normalize, int32_t H, int32_t W, const float* in,
                  int64_t in_cs, int64_t in_rs, const float* mask, float* out, void* stream);
int gs_lpips_pool(int32_t backward, int32_t H, int32_t W, int32_t C, const float* in, const float* g, const float* dp, float* out,
                  void* stream);

/* ---- introspection for parity tests: device pointers INTO the opaque state buffers.  `field`: one of the enums below
 * (the numbers are part of the ABI; a number past a state's range, or an image field the state does not have, is
 * GS_E_BAD_ARG). */
enum GsGeomField {
    GS_GEOM_DEPTHS = 0,      /* f32[P] */
    GS_GEOM_TILES = 1,       /* tiles touched u32[P] */
    GS_GEOM_REC = 2,         /* splat records f32[P,12]: (x, y, conicA, conicB, conicC, opacity, r, g, b, first pair u32,
                              * rect_min u32 (x | y<<16), rect_size u32 (w | h<<16)) */
    GS_GEOM_CLAMPED = 3,     /* clamped bitmask u32[P] */
    GS_GEOM_SORTED_IDX = 4,  /* depth-sorted Gaussian index u32[P] */
    GS_GEOM_COUNT = 5,       /* num_rendered u64[1] */
    GS_GEOM_FIELDS = 6
};
enum GsBinningField {
    GS_BIN_POINT_LIST = 0,   /* u32[D]: tile after tile, (depth, index) order inside a tile; tile t owns ranges[t] of it */
    GS_BIN_QLIST = 1,        /* u32[4 D]: the quadrants' compacted lists as the forward recorded them; quadrant q of tile t
                              * (n_t list entries) owns [4 ranges[t].x + q n_t, ... + n_t), filled up to GS_IMG_QCOUNT's
                              * count (at least) */
    GS_BIN_FIELDS = 2
};
enum GsImageField {
    GS_IMG_RANGES = 0,       /* u32[tiles,2] */
    GS_IMG_N_CONTRIB = 1,    /* u32[H,W] */
    GS_IMG_FINAL_T = 2,      /* f32[H,W] */
    GS_IMG_QCOUNT = 3,       /* per-quadrant compacted count up to the last contributor u32[tiles,4] */
    GS_IMG_NCON_C = 4,       /* per-pixel last contributor in compacted coordinates u32[H,W] */
    GS_IMG_ORDER = 5,        /* launch order of the tiles u32[tiles], heaviest first; bit 31 = rendered by four waves per
                              * quadrant */
    GS_IMG_FIELDS = 6
};
int gs_geom_field(void* geom, int32_t P, int32_t field, void** out);
int gs_binning_field(void* binning, int64_t num_rendered, int32_t W, int32_t H, int32_t field, void** out);
int gs_image_field(void* img, int32_t W, int32_t H, int32_t field, void** out);
/* size of the image state for a call with these arguments (W, H, long_lists); gs_image_bytes(W, H) = long_lists 0 */
int gs_image_bytes_for(const GsFwdArgs* a, size_t* out);

/* ---- per-stage timing (the reference only timed whole calls with CUDA events: render.py:46-62,
 * train.py:79-88,181-185).  When enabled (process-wide: autograd runs the backward on its own host thread), every stage launched by this library is
 * bracketed by a pair of hipEvents recorded ON THE STAGE'S OWN STREAM.  gs_profile_collect waits for
 * the recorded events, sums the elapsed milliseconds and launch counts per stage name (first `max`
 * distinct stages, names are static strings) and clears the record. ---- */
int gs_profile_reserve(int n_events); /* pre-create events so that none is created inside a timed region */
int gs_profile_enable(int on);
int gs_profile_filter(const char* stage); /* NULL or "" = every stage; else only the named stage is timed */
int gs_profile_collect(int max, const char** names, float* ms, int32_t* launches, int32_t* n_out);

/* Report counter (bench.py's `pairs_valid`; never in a timed path): from the state of a finished forward, counts[0] = the
 * (pixel, Gaussian) pairs actually composited -- alpha >= 1/255 at that pixel, before the pixel was done -- and counts[1] =
 * the pairs a per-pixel walk up to each pixel's last contributor visits (the sum of n_contrib).  `counts`: two device
 * uint64.  Against 64 x (quadrant-list entries up to each quadrant's last contributor), which is what the render kernels
 * evaluate, counts[0] says how much of their work is useful. */
int gs_pair_stats(const GsFwdArgs* a, const void* geom, size_t geom_bytes, const void* binning, size_t binning_bytes,
                  const void* img, size_t img_bytes, int64_t num_rendered, uint64_t* counts, void* stream);

/* Shader clock under load (bench.py's `roofline.binding`): runs an FMA stream on every SIMD for `iters` x 32 instructions per
 * wave (8192 iterations ~ 1 ms) and adds up, over the workgroups, ticks[0] = shader-clock cycles (s_memtime) and ticks[1] =
 * ticks of the constant 100 MHz counter (s_memrealtime) spent in it: clock = ticks[0] / ticks[1] x 100 MHz.  `ticks`: four
 * device uint64 (two results, two scratch words).  Not capture-safe. */
int gs_clock_probe(uint64_t* ticks, int32_t iters, void* stream);

/* Which XCD (accelerator die with its own L2) every workgroup of a launch of `n_blocks` workgroups of 64 threads runs on:
 * xcc[b] = HW_REG_XCC_ID of workgroup b.  The render launches' workgroup numbering (gs_tuning "xcd_map") rests on the
 * premise that the dispatcher deals workgroups round-robin over the XCDs, xcc[b] == b % 8 on an MI355X in SPX mode: only
 * then do the four quadrant waves of a tile share an XCD's L2.  A different deal costs speed, not the image -- this call is
 * how the -m gpu suite checks the premise.  `xcc`: n_blocks device uint32. */
int gs_xcc_probe(uint32_t* xcc, int32_t n_blocks, void* stream);

/* process-wide tuning switches for experiments and A/B measurements.  Without effect on the results: "xcd_map" (1: the
 * four quadrant waves of a tile on one XCD), "depth_sort" (1: bucket sort, 0: LSD radix), "nt_stores" (1: the backward's
 * row-mark fill is written with streaming stores), "fwd_marks" (1: the forward's render launch sets the backward's row
 * marks on the side, 0: every backward sets them itself), "bwd_order" (1: the backward orders the tiles by the forward's
 * per-quadrant last contributors, 0: walks them in the forward's launch order).  With an effect of fp32 rounding (which kernels render a frame of few,
 * long tile lists; flip them between frames only, "small_tiles" also changes the image state's size): "fwd4" (0: one wave per quadrant everywhere; 1 (default): four
 * waves per quadrant, four entries per step on the marked tiles; any other value is GS_E_BAD_ARG), "bwd_chunks" (1:
 * backward in chunks from the forward's checkpoints), "small_tiles" (images of up to this many tiles use both whatever GsFwdArgs.long_lists says; 2048).  "shared_qlist"
 * (1: gs_forward_shared renders from the recorded quadrant lists, 0: from the tiles' lists; same bits).  "ones_fast" (1: a
 * second render whose colours are all ones is written as 1 - T of the first; 0: composited; equal to fp32 rounding) */
int gs_tuning(const char* name, int value);
const char* gs_status_string(int code);
int gs_last_hip_error(void); /* hipError_t of the most recent GS_E_HIP on this thread */
const char* gs_last_stage(void); /* name of the stage that failed (debug mode names every kernel) */
const char* gs_build_info(void); /* "gfx950 ..." */

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_MI355_H */
