"""ctypes binding of libgsplat_mi355.so (include/gsplat_mi355.h).  There is NO fallback: if the HIP
library is missing or a call fails, this raises."""
import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSPLAT_LIB_PATH: another build of the same library (A/B runs of kernel variants: `GSPLAT_VARIANT=name python build.py`
# leaves it under variants/name/; tools/variant_cmp.sh, tools/ab_bench.sh)
LIB_PATH = os.environ.get("GSPLAT_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libgsplat_mi355.so")


class GsFwdArgs(ctypes.Structure):
    _fields_ = [
        ("P", c_int32), ("sh_degree", c_int32), ("M", c_int32), ("W", c_int32), ("H", c_int32),
        ("bg", c_void_p), ("means3D", c_void_p), ("shs", c_void_p), ("colors_precomp", c_void_p),
        ("opacities", c_void_p), ("scales", c_void_p), ("rotations", c_void_p), ("cov3D_precomp", c_void_p),
        ("viewmatrix", c_void_p), ("projmatrix", c_void_p), ("campos", c_void_p),
        ("scale_modifier", c_float), ("tanfovx", c_float), ("tanfovy", c_float),
        ("prefiltered", c_int32), ("debug", c_int32), ("tile_rect", c_int32), ("long_lists", c_int32),
        ("frame_stats", c_void_p), ("l1_target", c_void_p), ("l1_loss", c_void_p), ("l1_grad", c_void_p),
        ("forward_only", c_int32), ("antialiasing", c_int32),
    ]


class GsSecondImage(ctypes.Structure):  # include/gsplat_mi355.h: GsSecondImage
    _fields_ = [("colors", c_void_p), ("out_color", c_void_p), ("dL_dpix", c_void_p), ("img", c_void_p),
                ("img_bytes", c_size_t), ("long_lists", c_int32),
                ("dL_dcolors", c_void_p)]  # (trailing, NULL by default: the six-field positional construction stays valid)


class GsGrads(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("dL_dmeans3D", "dL_dmeans2D", "dL_dsh", "dL_dcolors", "dL_dopacity",
                                        "dL_dscales", "dL_drotations", "dL_dcov3D")]


# status codes (include/gsplat_mi355.h)
GS_OK, GS_E_BAD_ARG, GS_E_EXCLUSIVE, GS_E_TOO_LARGE, GS_E_HIP, GS_E_WORKSPACE, GS_E_CAPTURE = 0, -1, -2, -3, -4, -5, -6
GS_ADAM_MAX_TENSORS = 16
# `field` of gs_geom_field / gs_binning_field / gs_image_field (include/gsplat_mi355.h: GsGeomField, GsBinningField, GsImageField)
GS_GEOM_DEPTHS, GS_GEOM_TILES, GS_GEOM_REC, GS_GEOM_CLAMPED, GS_GEOM_SORTED_IDX, GS_GEOM_COUNT, GS_GEOM_FIELDS = range(7)
GS_BIN_POINT_LIST, GS_BIN_QLIST, GS_BIN_FIELDS = range(3)
# u64 word of the block GS_GEOM_COUNT names that says "a second render's colours are not all ones" (csrc/common.h:
# COUNT_NOT_ONES; tests/test_invdepth_host.py holds the two together)
GS_COUNT_NOT_ONES = 2
(GS_IMG_RANGES, GS_IMG_N_CONTRIB, GS_IMG_FINAL_T, GS_IMG_QCOUNT, GS_IMG_NCON_C, GS_IMG_ORDER, GS_IMG_FIELDS) = range(7)


class GsAdamTensor(ctypes.Structure):  # include/gsplat_mi355.h: GsAdamTensor
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("n", c_int64), ("lr", c_float)]


GS_OPTIM_MAX_TENSORS, GS_GRAD_NORM_BATCH, GS_ADAM_EX_BATCH, GS_ADAM_STEP_BATCH = 4096, 192, 48, 384  # include/gsplat_mi355.h


class GsGradTensor(ctypes.Structure):  # include/gsplat_mi355.h: GsGradTensor
    _fields_ = [("grad", c_void_p), ("n", c_int64)]


class GsAdamTensorEx(ctypes.Structure):  # include/gsplat_mi355.h: GsAdamTensorEx
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("n", c_int64), ("lr", c_float), ("weight_decay", c_float), ("step", c_void_p), ("lr_dev", c_void_p)]


GS_DENSIFY_MAX_TENSORS = 24  # include/gsplat_mi355.h: GS_DENSIFY_*
GS_DENSIFY_COPY, GS_DENSIFY_ZERO_IF_NEW, GS_DENSIFY_ZERO, GS_DENSIFY_CHILD_POSITION, GS_DENSIFY_CHILD_SCALING = 0, 1, 2, 3, 4
GS_DENSIFY_F_KEEP, GS_DENSIFY_F_CLONE, GS_DENSIFY_F_SPLIT, GS_DENSIFY_F_PRUNE = 1, 2, 4, 8
GS_DENSIFY_F_CHILD_PRUNE, GS_DENSIFY_F_CLONE_KEPT, GS_DENSIFY_F_CHILDREN_KEPT = 16, 32, 64


class GsDensifyPlan(ctypes.Structure):  # include/gsplat_mi355.h: GsDensifyPlan
    _fields_ = [("N", c_int32), ("scaling", c_void_p), ("opacity", c_void_p), ("grad_accum", c_void_p), ("denom", c_void_p),
                ("prune_mask", c_void_p), ("grad_threshold", c_float), ("split_scale", c_float), ("min_opacity", c_float),
                ("max_world_scale", c_float), ("max_screen_size", c_float), ("prune_size", c_int32)]


class GsDensifyTensor(ctypes.Structure):  # include/gsplat_mi355.h: GsDensifyTensor
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("width", c_int32), ("kind", c_int32)]


class GsAiapSet(ctypes.Structure):  # include/gsplat_mi355.h: GsAiapSet
    _fields_ = [("xc", c_void_p), ("xd", c_void_p), ("D", c_int32), ("loss", c_void_p), ("dL_dloss", c_void_p),
                ("dL_dxc", c_void_p), ("dL_dxd", c_void_p)]


GS_HASHGRID_MAX_LEVELS = 32  # include/gsplat_mi355.h


GS_SKIN_BONES = 24  # include/gsplat_mi355.h
GS_SKIN_HIERARCHICAL, GS_SKIN_SOFTMAX, GS_SKIN_WEIGHTS = 0, 1, 2


GS_POSE_BONES, GS_POSE_MAX_BETAS, GS_POSE_STATE_FLOATS = 24, 16, 512  # include/gsplat_mi355.h


class GsPoseArgs(ctypes.Structure):  # include/gsplat_mi355.h: GsPoseArgs
    _fields_ = [("V", c_int32), ("NB", c_int32), ("parents", c_int32 * GS_POSE_BONES)] + [
        (n, c_void_p) for n in ("v_template", "shapedirs", "J_template", "J_shapedirs", "betas", "root_orient", "pose_body",
                                "pose_hand", "trans", "rots_gt")]


GS_POSE_ENC_JOINTS, GS_POSE_ENC_MAX_DIM, GS_POSE_ENC_STATE_FLOATS = 24, 16, 1392  # include/gsplat_mi355.h
GS_NONRIGID_MAX_D = 2048
GS_NR_SCALE_LOGIT, GS_NR_SCALE_EXP, GS_NR_SCALE_ZERO = 0, 1, 2
GS_NR_ROT_ADD, GS_NR_ROT_MULT = 0, 1


class GsPoseEncArgs(ctypes.Structure):  # include/gsplat_mi355.h: GsPoseEncArgs
    _fields_ = [("d", c_int32), ("parents", c_int32 * GS_POSE_ENC_JOINTS)] + [
        (n, c_void_p) for n in ("rots", "Jtrs", "W0", "b0")] + [
        (n, c_void_p * GS_POSE_ENC_JOINTS) for n in ("W1", "b1", "W2", "b2")]


GS_TEXTURE_MAX_D, GS_TEXTURE_MAX_BEFORE, GS_TEXTURE_MAX_AFTER = 512, 6, 2  # include/gsplat_mi355.h


class GsTextureArgs(ctypes.Structure):  # include/gsplat_mi355.h: GsTextureArgs
    _fields_ = [("N", c_int32), ("D", c_int32), ("sh_degree", c_int32), ("n_before", c_int32), ("n_after", c_int32),
                ("before_w", c_int32 * GS_TEXTURE_MAX_BEFORE), ("after_w", c_int32 * GS_TEXTURE_MAX_AFTER),
                ("latent_dim", c_int32), ("rot_stride", c_int32), ("rot_row", c_int32), ("use_noise", c_int32),
                ("noise", c_float * 9), ("before", c_void_p * GS_TEXTURE_MAX_BEFORE), ("after", c_void_p * GS_TEXTURE_MAX_AFTER),
                ("xyz", c_void_p), ("campos", c_void_p), ("fwd_transform", c_void_p), ("latent", c_void_p)]


# include/gsplat_mi355.h
GS_MLP_MAX_WIDTH, GS_MLP_MAX_HIDDEN, GS_MLP_MAX_LAYERS, GS_MLP_MAX_IN, GS_MLP_MAX_COND, GS_MLP_MAX_OUT = 128, 6, 7, 512, 512, 64
GS_MLP_TILE_ROWS, GS_MLP_PARTIAL_MIN_ROWS, GS_MLP_MAX_PARTIALS = 128, 256, 128


class GsMlpArgs(ctypes.Structure):  # include/gsplat_mi355.h: GsMlpArgs
    _fields_ = [(n, c_int32) for n in ("N", "dim_in", "dim_cond", "width", "n_hidden", "dim_out")] + [
        ("slope", c_float), ("x", c_void_p), ("cond", c_void_p)] + [
        (n, c_void_p * GS_MLP_MAX_LAYERS) for n in ("W", "b", "dW", "db")] + [("dx", c_void_p), ("dcond", c_void_p)]


GS_LPIPS_LAYERS, GS_LPIPS_TAPS, GS_LPIPS_MIN_SIZE, GS_LPIPS_MAX_SIZE = 13, 5, 16, 2048  # include/gsplat_mi355.h
GS_LPIPS_WS_FORWARD, GS_LPIPS_WS_SAVED, GS_LPIPS_WS_BACKWARD = 0, 1, 2


class GsLpipsArgs(ctypes.Structure):  # include/gsplat_mi355.h: GsLpipsArgs
    _fields_ = [(n, c_int32) for n in ("H", "W", "normalize", "need_grad0", "need_grad1")] + [
        (n, c_int64) for n in ("cs0", "rs0", "cs1", "rs1")] + [(n, c_void_p) for n in ("in0", "in1", "packed")] + [
        ("weight", c_void_p * GS_LPIPS_LAYERS), ("bias", c_void_p * GS_LPIPS_LAYERS), ("lin", c_void_p * GS_LPIPS_TAPS),
        ("shift", c_void_p), ("scale", c_void_p)]


class GsHashGrid(ctypes.Structure):  # include/gsplat_mi355.h: GsHashGrid
    _fields_ = [("n_levels", c_int32), ("n_features_per_level", c_int32), ("log2_hashmap_size", c_int32),
                ("base_resolution", c_int32), ("per_level_scale", c_float)]


_fwd, _grads, _size_out = POINTER(GsFwdArgs), POINTER(GsGrads), POINTER(c_size_t)
# the forward's three states (geom, binning, image), each with its size, as gs_forward_render and every backward take them
_states = [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]
_bwd_head = [_fwd, c_void_p] + _states + [c_int64, c_void_p, c_void_p]  # a, radii, states, num_rendered, out_color, dL_dpix
_bwd_tail = [c_void_p, c_size_t, _grads, c_void_p]                        # scratch, scratch_bytes, grads, stream

# Every function of include/gsplat_mi355.h, in the header's order: name -> (restype, argtypes).  This is the one place that
# names them; load() applies it, and tests/test_cabi_host.py holds it (with the structs and constants above) against the
# header, argument for argument.
SIGNATURES = {
    # ---- state-buffer sizes
    "gs_geom_bytes": (c_int, [c_int32, _size_out]),
    "gs_image_bytes": (c_int, [c_int32, c_int32, _size_out]),
    "gs_binning_bytes": (c_int, [c_int64, c_int32, c_int32, _size_out]),
    "gs_backward_scratch_bytes": (c_int, [c_int64, c_int32, c_int32, c_int32, _size_out]),
    # ---- forward and backward
    "gs_forward_preprocess": (c_int, [_fwd, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "gs_forward_render": (c_int, [_fwd] + _states + [c_int64, c_void_p, c_void_p]),
    "gs_forward": (c_int, [_fwd, c_void_p, c_size_t, c_void_p, c_size_t, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                           c_void_p, POINTER(c_int64), c_void_p]),
    "gs_forward_shared": (c_int, [_fwd, c_void_p, c_void_p] + _states + [c_int64, c_void_p, c_void_p]),
    "gs_backward": (c_int, _bwd_head + _bwd_tail),
    "gs_opacity_image": (c_int, [_fwd, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gs_backward_with_opacity": (c_int, _bwd_head + [c_void_p] + _bwd_tail),
    "gs_backward_with_second": (c_int, _bwd_head + [POINTER(GsSecondImage)] + _bwd_tail),
    "gs_mark_visible": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # ---- distCUDA2
    "knn_workspace_bytes": (c_int, [c_int32, _size_out]),
    "knn_dist2": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # ---- pre-rasterizer per-Gaussian chains
    "gs_build_covariance": (c_int, [c_int32, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "gs_build_covariance_backward": (c_int, [c_int32, c_void_p, c_float, c_void_p, c_int32] + [c_void_p] * 4),
    "gs_sh2rgb": (c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 8),
    "gs_sh2rgb_backward": (c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 10),
    # ---- image-side losses
    "gs_l1_loss_workspace_bytes": (c_int, [c_int64, _size_out]),
    "gs_l1_loss": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_bce_loss": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_ssim_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, _size_out]),
    "gs_ssim_forward": (c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    "gs_ssim_backward": (c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 8),
    # ---- K nearest neighbours
    "knn_points": (c_int, [c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # ---- training-step bookkeeping
    "gs_densify_stats": (c_int, [c_int32] + [c_void_p] * 6),
    "gs_adam_step": (c_int, [c_int32, POINTER(GsAdamTensor), c_double, c_double, c_double, c_int64, c_void_p]),
    # ---- the converter's optimizer step
    "gs_grad_norm_workspace_bytes": (c_int, [c_int32, POINTER(GsGradTensor), _size_out]),
    "gs_grad_norm": (c_int, [c_int32, POINTER(GsGradTensor), c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_grad_scale": (c_int, [c_int32, POINTER(GsGradTensor), c_void_p, c_void_p]),
    "gs_adam_step_ex": (c_int, [c_int32, POINTER(GsAdamTensorEx), c_double, c_double, c_double, c_int64, c_void_p, c_void_p]),
    # ---- densification cycle
    "gs_densify_workspace_bytes": (c_int, [c_int32, _size_out]),
    "gs_densify_plan": (c_int, [POINTER(GsDensifyPlan), c_void_p, c_size_t, c_void_p, c_void_p]),
    "gs_densify_apply": (c_int, [c_int32, c_int32, c_void_p, c_size_t, c_int32, POINTER(GsDensifyTensor)] + [c_void_p] * 4),
    "gs_reset_opacity": (c_int, [c_int32] + [c_void_p] * 5),
    # ---- as-isometric-as-possible regularisers
    "gs_aiap_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, _size_out]),
    "gs_aiap_forward": (c_int, [c_int32, c_int32, c_void_p, c_int32, POINTER(GsAiapSet), c_void_p, c_size_t, c_void_p]),
    "gs_aiap_backward": (c_int, [c_int32, c_int32, c_void_p, c_int32, POINTER(GsAiapSet), c_void_p, c_size_t, c_void_p]),
    # ---- multiresolution hash-grid encoding
    "gs_hashgrid_levels": (c_int, [POINTER(GsHashGrid), c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_hashgrid_workspace_bytes": (c_int, [POINTER(GsHashGrid), c_int32, _size_out]),
    "gs_hashgrid_forward": (c_int, [POINTER(GsHashGrid), c_int32] + [c_void_p] * 4),
    "gs_hashgrid_backward": (c_int, [POINTER(GsHashGrid), c_int32] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    # ---- linear blend skinning
    "gs_skin_weights_forward": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "gs_skin_weights_backward": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_skinning_workspace_bytes": (c_int, [c_int32, _size_out]),
    "gs_skinning_forward": (c_int, [c_int32, c_int32] + [c_void_p] * 8),
    "gs_skinning_backward": (c_int, [c_int32, c_int32] + [c_void_p] * 11 + [c_size_t, c_void_p]),
    # ---- the skinning regulariser
    "gs_mesh_sample": (c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 13),
    "gs_skin_loss_workspace_bytes": (c_int, [c_int32, _size_out]),
    "gs_skin_loss_forward": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_skin_loss_backward": (c_int, [c_int32, c_int32] + [c_void_p] * 5),
    # ---- SMPL pose correction
    "gs_pose_workspace_bytes": (c_int, [c_int32, _size_out]),
    "gs_pose_forward": (c_int, [POINTER(GsPoseArgs)] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    "gs_pose_backward": (c_int, [POINTER(GsPoseArgs)] + [c_void_p] * 11),
    # ---- the non-rigid deformer around its MLP
    "gs_pose_encoder_grad_floats": (c_int, [c_int32, _size_out]),
    "gs_pose_encoder_forward": (c_int, [POINTER(GsPoseEncArgs), c_void_p, c_void_p, c_void_p]),
    "gs_pose_encoder_backward": (c_int, [POINTER(GsPoseEncArgs)] + [c_void_p] * 6),
    "gs_nonrigid_workspace_bytes": (c_int, [c_int32, c_int32, _size_out]),
    "gs_nonrigid_apply_forward": (c_int, [c_int32] * 4 + [c_void_p] * 10 + [c_size_t, c_void_p]),
    "gs_nonrigid_apply_backward": (c_int, [c_int32] * 4 + [c_void_p] * 14),
    # ---- the input of the ColorMLP texture
    "gs_texture_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, _size_out]),
    "gs_texture_input_forward": (c_int, [POINTER(GsTextureArgs), c_void_p, c_void_p]),
    "gs_texture_input_backward": (c_int, [POINTER(GsTextureArgs), c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    # ---- the dense networks
    "gs_mlp_workspace_bytes": (c_int, [POINTER(GsMlpArgs), c_int32, _size_out]),
    "gs_mlp_forward": (c_int, [POINTER(GsMlpArgs), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_mlp_backward": (c_int, [POINTER(GsMlpArgs), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # ---- the LPIPS-VGG perceptual loss
    "gs_lpips_packed_bytes": (c_int, [_size_out]),
    "gs_lpips_pack_weights": (c_int, [POINTER(GsLpipsArgs), c_void_p, c_size_t, c_void_p]),
    "gs_lpips_workspace_bytes": (c_int, [c_int32] * 5 + [_size_out]),
    "gs_lpips_forward": (c_int, [POINTER(GsLpipsArgs), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "gs_lpips_backward": (c_int, [POINTER(GsLpipsArgs), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                  c_void_p]),
    "gs_lpips_conv": (c_int, [c_void_p] + [c_int32] * 5 + [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "gs_lpips_pool": (c_int, [c_int32] * 4 + [c_void_p] * 5),
    # ---- introspection for parity tests
    "gs_geom_field": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_void_p)]),
    "gs_binning_field": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "gs_image_field": (c_int, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "gs_image_bytes_for": (c_int, [_fwd, _size_out]),
    # ---- per-stage timing
    "gs_profile_reserve": (c_int, [c_int]),
    "gs_profile_enable": (c_int, [c_int]),
    "gs_profile_filter": (c_int, [c_char_p]),
    "gs_profile_collect": (c_int, [c_int, POINTER(c_char_p), POINTER(c_float), POINTER(c_int32), POINTER(c_int32)]),
    # ---- report counters, probes, tuning switches, status
    "gs_pair_stats": (c_int, [_fwd] + _states + [c_int64, c_void_p, c_void_p]),
    "gs_clock_probe": (c_int, [c_void_p, c_int32, c_void_p]),
    "gs_xcc_probe": (c_int, [c_void_p, c_int32, c_void_p]),
    "gs_tuning": (c_int, [c_char_p, c_int]),
    "gs_status_string": (c_char_p, [c_int]),
    "gs_last_hip_error": (c_int, []),
    "gs_last_stage": (c_char_p, []),
    "gs_build_info": (c_char_p, []),
}
EXPORTS = list(SIGNATURES)

_lock = threading.Lock()
_lib = None


def load():
    """Loads the HIP library (torch first, so that its bundled HIP runtime is the one both share)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (libamdhip64 must come from torch's process image)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgsplat_mi355.so not found at %s: build it with "
                               "`python 3dgs-avatar-release_amd/build.py` (there is no CPU fallback)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        L = load()
        msg = L.gs_status_string(rc).decode()
        if rc == GS_E_HIP:
            msg += " %d in stage '%s'" % (L.gs_last_hip_error(), L.gs_last_stage().decode())
        raise RuntimeError("gsplat_mi355: " + msg)


tuning_listeners = []  # called after every change of a tuning switch ("small_tiles" changes the image state's size:
#                        whoever memoises the library's size queries forgets them here)


def tuning(name, value):
    """Process-wide tuning switch of the library (A/B measurements)."""
    check(load().gs_tuning(name.encode(), int(value)))
    for fn in tuning_listeners:
        fn()


def profile_enable(on, stage=None):
    """Per-stage hipEvent timing on/off; `stage` restricts it to one stage (two events per call)."""
    check(load().gs_profile_filter(stage.encode() if stage else None))
    check(load().gs_profile_enable(1 if on else 0))


def profile_reserve(n_events):
    """Pre-creates HIP events for the stage timers (event creation is slow: keep it out of timed regions)."""
    check(load().gs_profile_reserve(int(n_events)))


def profile_collect(max_stages=32):
    """{stage: (total_ms, launches)} since the last collect (waits for the recorded events)."""
    names = (c_char_p * max_stages)()
    ms = (c_float * max_stages)()
    cnt = (c_int32 * max_stages)()
    n = c_int32(0)
    check(load().gs_profile_collect(max_stages, names, ms, cnt, ctypes.byref(n)))
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(n.value)}


def xcc_probe(dev, n_blocks=4096):
    """The XCD every workgroup of a launch of `n_blocks` workgroups runs on (gs_xcc_probe), as a CPU int tensor."""
    import torch
    t = torch.zeros(int(n_blocks), dtype=torch.int32, device=dev)
    with on_device(dev):
        check(load().gs_xcc_probe(t.data_ptr(), int(n_blocks), stream_ptr(dev)))
    return t.cpu()


def clock_probe(dev, iters=8192):
    """Shader clock in Hz under a VALU-bound load (an FMA stream of ~1 ms on every SIMD), measured now on `dev`."""
    import torch
    t = torch.zeros(4, dtype=torch.int64, device=dev)
    with on_device(dev):
        check(load().gs_clock_probe(t.data_ptr(), int(iters), stream_ptr(dev)))
    c = t.cpu()
    return float(c[0]) / max(float(c[1]), 1.0) * 1.0e8


def nbytes(fn, *args):
    out = c_size_t(0)
    check(fn(*args, ctypes.byref(out)))
    return int(out.value)


def field_view(fn_name, buf, *args, nbytes):
    """The `nbytes` of a field of the state buffer `buf` (a uint8 tensor), as a view of it.  `fn_name`: gs_geom_field,
    gs_binning_field or gs_image_field; `args`: what that takes between the buffer and the result (the sizes the buffer was
    carved for, the field's id)."""
    out = c_void_p(0)
    check(getattr(load(), fn_name)(buf.data_ptr(), *args, ctypes.byref(out)))
    off = int(out.value) - buf.data_ptr()
    assert 0 <= off and off + nbytes <= buf.numel()
    return buf[off:off + nbytes]


class _OnDevice(object):
    __slots__ = ("idx", "prev")

    def __init__(self, idx):
        self.idx = idx
        self.prev = -1

    def __enter__(self):
        self.prev = _exchange_device(self.idx)

    def __exit__(self, *exc):
        _maybe_exchange_device(self.prev)
        return False


_exchange_device = _maybe_exchange_device = None


def on_device(dev):
    """`with on_device(dev):` -- torch.cuda.device(dev) without its Python-side index parsing (~5 us per use: as much as a
    kernel launch on a forward-only frame).  Falls back to torch.cuda.device where torch lacks the two C helpers."""
    global _exchange_device, _maybe_exchange_device
    import torch
    if _exchange_device is None:
        _exchange_device = getattr(torch.cuda, "_exchange_device", False)
        _maybe_exchange_device = getattr(torch.cuda, "_maybe_exchange_device", False)
    if dev.index is None or not _exchange_device or not _maybe_exchange_device:
        return torch.cuda.device(dev)
    return _OnDevice(dev.index)


_raw_stream = None


def stream_handle(dev):
    """The current HIP stream of `dev` as an integer handle (what torch.cuda.current_stream(dev).cuda_stream returns,
    without building a Stream object and parsing the device: ~5 us per call, seven calls per training step)."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream and dev.index is not None:
        return int(_raw_stream(dev.index))
    return int(torch.cuda.current_stream(dev).cuda_stream)


def stream_ptr(dev):
    return c_void_p(stream_handle(dev))


def ptr(t):
    """Device pointer of a tensor, or None (NULL = absent) for None / empty tensors."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


_float32 = None


def dev32(t, name):
    """`t` itself, after the two checks the fused modules make of a tensor argument: on the GPU, fp32.  (The caller detaches
    it or makes it contiguous, as its kernels need.)"""
    global _float32
    if _float32 is None:
        import torch
        _float32 = torch.float32
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)
    if t.dtype != _float32:
        raise TypeError("%s: fp32 tensor expected" % name)
    return t


def is_aligned(t, nbytes=16):
    """True when `t.data_ptr()` is a multiple of `nbytes` (an empty tensor counts as aligned: it is passed as NULL).  A
    contiguous view can start at any element of its storage (`img[1:]` of a (3, H, W) image with H W odd starts 4 bytes
    past a 16-byte boundary); kernels that read or write a caller's tensor as float4 need 16."""
    return t.numel() == 0 or t.data_ptr() % nbytes == 0


def contiguous_aligned(t, nbytes=16):
    """`t.contiguous()`, copied once more into fresh (allocator-aligned) storage when that view does not start on an
    `nbytes` boundary."""
    t = t.contiguous()
    return t if is_aligned(t, nbytes) else t.clone()
