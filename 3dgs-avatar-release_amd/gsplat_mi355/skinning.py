"""The rigid deformer's linear blend skinning (models/deformer/rigid.py) on the GPU through libgsplat_mi355
(csrc/skinning.hip, whose header comment carries the spec): bone weights from the skinning MLP's logits
(`hierarchical_softmax` or F.softmax), the blended bone transform T_fwd, the deformed positions and the rotation matrices
that `gs_build_covariance(is_matrix = 1)` / `gs_sh2rgb` consume, as one autograd node.  The forward is one launch; the
backward is one launch plus, when the bone transforms want a gradient, a small fixed-order reduction: no atomics (bitwise
reproducible), no host synchronisation, capture-safe.

* `hierarchical_softmax(x)` -- the reference's function, (N, 25) -> (N, 24).
* `skinning_softmax(logit)` -- SkinningField.softmax: 25 columns hierarchical, 24 F.softmax, anything else ValueError.
* `linear_blend_skinning(w, tfs, xyz, rotation, weights=False)` -> (xyz_bar, rotation_bar, T_fwd).
* `skinning_field_forward(field, gaussians, iteration, camera)` -- SkinningField.forward with the fused op
  (`SkinningField.forward = skinning_field_forward`).
Device fp32 tensors only: there is no CPU path.
"""
import torch

from . import _lib

BONES = _lib.GS_SKIN_BONES


def _dev32(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s: fp32 tensor expected" % name)
    return t.detach()


def _logit_kind(w, weights):
    if w.dim() != 2:
        raise ValueError("skinning: w must be (N, 25) or (N, 24), got %s" % (tuple(w.shape),))
    if weights:
        if w.shape[1] != BONES:
            raise ValueError("skinning: weights=True needs (N, 24) weights, got %s" % (tuple(w.shape),))
        return _lib.GS_SKIN_WEIGHTS
    if w.shape[1] == 25:
        return _lib.GS_SKIN_HIERARCHICAL
    if w.shape[1] == 24:
        return _lib.GS_SKIN_SOFTMAX
    raise ValueError("skinning: logits must have 25 (hierarchical) or 24 (softmax) columns, got %d" % w.shape[1])


class _Weights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, kind):
        x = _lib.contiguous_aligned(_dev32(logits, "logits"))
        dev, n = x.device, int(x.shape[0])
        out = torch.empty(n, BONES, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_skin_weights_forward(n, kind, _lib.ptr(x), _lib.ptr(out), _lib.stream_ptr(dev)))
        ctx.save_for_backward(x)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        dev, n = x.device, int(x.shape[0])
        g = _lib.contiguous_aligned(g.to(torch.float32))
        dx = torch.empty_like(x)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_skin_weights_backward(n, ctx.kind, _lib.ptr(x), _lib.ptr(g), _lib.ptr(dx),
                                                            _lib.stream_ptr(dev)))
        return dx, None


class _Skinning(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, tfs, xyz, rotation, kind):
        ctx.set_materialize_grads(False)
        w = _lib.contiguous_aligned(_dev32(w, "w"))
        tfs = _lib.contiguous_aligned(_dev32(tfs, "tfs"))
        xyz = _dev32(xyz, "xyz").contiguous()
        rotation = _lib.contiguous_aligned(_dev32(rotation, "rotation"))
        dev, n = w.device, int(w.shape[0])
        xyz_bar = torch.empty(n, 3, dtype=torch.float32, device=dev)
        rot_bar = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
        T_fwd = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_skinning_forward(n, kind, _lib.ptr(w), _lib.ptr(tfs), _lib.ptr(xyz), _lib.ptr(rotation),
                                                       _lib.ptr(xyz_bar), _lib.ptr(rot_bar), _lib.ptr(T_fwd),
                                                       _lib.stream_ptr(dev)))
        ctx.save_for_backward(w, tfs, xyz, rotation)
        ctx.kind = kind
        ctx.mark_non_differentiable(T_fwd)
        return xyz_bar, rot_bar, T_fwd

    @staticmethod
    def backward(ctx, g_xyz, g_rot, _g_T):
        w, tfs, xyz, rotation = ctx.saved_tensors
        need_w, need_tfs, need_xyz, need_rot = ctx.needs_input_grad[:4]
        if not (need_w or need_tfs or need_xyz or need_rot) or (g_xyz is None and g_rot is None):
            return None, None, None, None, None
        dev, n = w.device, int(w.shape[0])
        dw = torch.empty_like(w) if need_w else None
        dtfs = torch.empty(BONES, 4, 4, dtype=torch.float32, device=dev) if need_tfs else None
        dxyz = torch.empty_like(xyz) if need_xyz else None
        drot = torch.empty_like(rotation) if need_rot else None
        if n == 0:
            return dw, (dtfs.zero_() if need_tfs else None), dxyz, drot, None
        L = _lib.load()
        ws = None
        if need_tfs:  # the per-block partials of dtfs (no reduction, no workspace without it)
            ws = torch.empty(_lib.nbytes(L.gs_skinning_workspace_bytes, n), dtype=torch.uint8, device=dev)
        g_xyz = g_xyz.to(torch.float32).contiguous() if g_xyz is not None else None
        g_rot = g_rot.to(torch.float32).contiguous() if g_rot is not None else None
        with _lib.on_device(dev):
            _lib.check(L.gs_skinning_backward(n, ctx.kind, _lib.ptr(w), _lib.ptr(tfs), _lib.ptr(xyz), _lib.ptr(rotation),
                                              _lib.ptr(g_xyz), _lib.ptr(g_rot), _lib.ptr(dw), _lib.ptr(dtfs), _lib.ptr(dxyz),
                                              _lib.ptr(drot), _lib.ptr(ws), ws.numel() if ws is not None else 0,
                                              _lib.stream_ptr(dev)))
        return dw, dtfs, dxyz, drot, None


def hierarchical_softmax(x):
    """models/deformer/rigid.py hierarchical_softmax: (N, 25) logits -> (N, 24) weights along the kinematic tree."""
    if x.dim() != 2 or x.shape[1] != 25:
        raise ValueError("hierarchical_softmax: (N, 25) logits expected, got %s" % (tuple(x.shape),))
    _dev32(x, "logits")
    return _Weights.apply(x, _lib.GS_SKIN_HIERARCHICAL)


def skinning_softmax(logit):
    """SkinningField.softmax: hierarchical_softmax for 25 columns, F.softmax(dim=-1) for 24, ValueError otherwise."""
    if logit.dim() != 2 or logit.shape[-1] not in (24, 25):
        raise ValueError("skinning_softmax: (N, 25) or (N, 24) logits expected, got %s" % (tuple(logit.shape),))
    _dev32(logit, "logits")
    kind = _lib.GS_SKIN_HIERARCHICAL if logit.shape[-1] == 25 else _lib.GS_SKIN_SOFTMAX
    return _Weights.apply(logit, kind)


def linear_blend_skinning(w, tfs, xyz, rotation, weights=False):
    """(xyz_bar (N, 3), rotation_bar (N, 3, 3), T_fwd (N, 4, 4)) of the rigid deformer: W from the (N, 25) or (N, 24)
    logits `w` (or, weights=True, the (N, 24) weights themselves, as SMPLNN), T_fwd = sum_j W_j tfs_j with tfs the
    (24, 4, 4) bone transforms, xyz_bar = T_fwd[:3,:3] xyz + T_fwd[:3,3], rotation_bar = T_fwd[:3,:3]
    build_rotation(rotation).  T_fwd carries no gradient (the reference detaches it)."""
    kind = _logit_kind(w, weights)
    n = int(w.shape[0])
    if tuple(tfs.shape) != (BONES, 4, 4):
        raise ValueError("skinning: tfs must be (24, 4, 4), got %s" % (tuple(tfs.shape),))
    if tuple(xyz.shape) != (n, 3) or tuple(rotation.shape) != (n, 4):
        raise ValueError("skinning: xyz (N, 3) and rotation (N, 4) with N = %d expected, got %s and %s"
                         % (n, tuple(xyz.shape), tuple(rotation.shape)))
    for t, name in ((w, "w"), (tfs, "tfs"), (xyz, "xyz"), (rotation, "rotation")):
        _dev32(t, name)
    return _Skinning.apply(w, tfs, xyz, rotation, kind)


def skinning_field_forward(field, gaussians, iteration, camera):
    """SkinningField.forward (models/deformer/rigid.py:215-236) with the fused op.  Reads field.aabb, field.lbs_network,
    camera.bone_transforms and gaussians.get_xyz / _rotation / clone() / set_fwd_transform; sets `_xyz` and
    `rotation_precomp` on the clone.  The voxel-grid path (field.distill) is not supported."""
    if getattr(field, "distill", False):
        raise NotImplementedError("skinning_field_forward: the distill (voxel-grid) path is not supported")
    tfs = camera.bone_transforms
    xyz = gaussians.get_xyz
    xyz_norm = field.aabb.normalize(xyz, sym=True)
    logits = field.lbs_network(xyz_norm)
    xyz_bar, rotation_bar, T_fwd = linear_blend_skinning(logits, tfs, xyz, gaussians._rotation)
    deformed_gaussians = gaussians.clone()
    deformed_gaussians.set_fwd_transform(T_fwd.detach())
    deformed_gaussians._xyz = xyz_bar
    setattr(deformed_gaussians, "rotation_precomp", rotation_bar)
    return deformed_gaussians
