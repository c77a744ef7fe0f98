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

The skinning regulariser (csrc/skinloss.hip, whose header comment carries its spec) on the device as well:
* `MeshSampler(verts, faces, vertex_weights, aabb_min, aabb_max, device)` -- area-weighted surface samples of a mesh with
  their blended skinning weights, one launch per `sample(n)`.
* `skinning_mse_loss(logits, target)` -- mse_loss(softmax(logits), target, 'none').sum(-1).mean() as one autograd node:
  two launches forward, one backward, summed in a fixed order (bitwise reproducible), capture-safe.
* `skinning_loss(field, draws=None)` -- SkinningField.get_skinning_loss
  (`SkinningField.get_skinning_loss = skinning_loss`).
Device fp32 tensors only: there is no CPU path.
"""
import numpy as np
import torch

from . import _lib

BONES = _lib.GS_SKIN_BONES


def _dev32(t, name):
    return _lib.dev32(t, name).detach()


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


class _SkinLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, kind):
        x = _lib.contiguous_aligned(_dev32(logits, "logits"))
        tg = _lib.contiguous_aligned(_dev32(target, "target"))
        dev, n = x.device, int(x.shape[0])
        ctx.save_for_backward(x, tg)
        ctx.kind = kind
        if n == 0:  # nothing to launch: 0, not torch's nan for an empty mean
            return torch.zeros((), dtype=torch.float32, device=dev)
        L = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.nbytes(L.gs_skin_loss_workspace_bytes, n), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.gs_skin_loss_forward(n, kind, _lib.ptr(x), _lib.ptr(tg), loss.data_ptr(), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr(dev)))
        return loss

    @staticmethod
    def backward(ctx, g):
        x, tg = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        dev, n = x.device, int(x.shape[0])
        dx = torch.empty_like(x)
        if n == 0:
            return dx, None, None
        g = g.to(torch.float32).contiguous()  # stays on the device: the kernel reads it there
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_skin_loss_backward(n, ctx.kind, _lib.ptr(x), _lib.ptr(tg), g.data_ptr(), _lib.ptr(dx),
                                                         _lib.stream_ptr(dev)))
        return dx, None, None


def skinning_mse_loss(logits, target):
    """get_skinning_loss's tail as one autograd node: W = hierarchical_softmax(logits) for (n, 25) logits, F.softmax for
    (n, 24), anything else ValueError; the result is mse_loss(W, target, reduction='none').sum(-1).mean() as a 0-d
    tensor.  The rows are summed in a fixed order in double (bitwise reproducible); `target` (n, 24) gets no gradient.
    n = 0 gives 0 (torch's mean over no rows would give nan)."""
    if logits.dim() != 2 or logits.shape[1] not in (24, 25):
        raise ValueError("skinning_mse_loss: (n, 25) or (n, 24) logits expected, got %s" % (tuple(logits.shape),))
    if tuple(target.shape) != (int(logits.shape[0]), BONES):
        raise ValueError("skinning_mse_loss: target must be (%d, 24), got %s" % (int(logits.shape[0]), tuple(target.shape)))
    _dev32(logits, "logits")
    _dev32(target, "target")
    if target.device != logits.device:
        raise RuntimeError("skinning_mse_loss: logits and target live on different devices")
    kind = _lib.GS_SKIN_HIERARCHICAL if logits.shape[1] == 25 else _lib.GS_SKIN_SOFTMAX
    return _SkinLoss.apply(logits, target, kind)


def _np(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


class MeshSampler(object):
    """Area-weighted surface samples of a triangle mesh with their barycentrically blended per-vertex skinning weights
    (SkinningField.sample_skinning_loss: trimesh's sample_surface, igl's barycentric coordinates and the numpy blend), on
    the device.  Built once from numpy arrays or tensors: `verts` (V, 3), `faces` (F, 3), `vertex_weights` (V, 24), and the
    box `aabb_min`, `aabb_max` (3) of AABB.normalize.  The face areas and their cumulative sum are computed in float64 from
    the fp32 vertices and rounded to fp32 once.  Public buffers (device tensors): `verts`, `faces` (int32), `cdf`,
    `vertex_weights`, `aabb_min`, `aabb_inv_extent`."""

    def __init__(self, verts, faces, vertex_weights, aabb_min, aabb_max, device):
        v = _np(verts, np.float32)
        f = _np(faces, np.int64)
        w = _np(vertex_weights, np.float32)
        lo, hi = _np(aabb_min, np.float32).reshape(-1), _np(aabb_max, np.float32).reshape(-1)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
            raise ValueError("MeshSampler: verts must be (V, 3) with V >= 1, got %s" % (v.shape,))
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError("MeshSampler: faces must be (F, 3) with F >= 1, got %s" % (f.shape,))
        if w.shape != (v.shape[0], BONES):
            raise ValueError("MeshSampler: vertex_weights must be (%d, 24), got %s" % (v.shape[0], w.shape))
        if f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError("MeshSampler: faces index vertices outside [0, %d)" % v.shape[0])
        if lo.shape != (3,) or hi.shape != (3,) or not (hi > lo).all():
            raise ValueError("MeshSampler: aabb_min < aabb_max, three values each, expected")
        v64 = v.astype(np.float64)
        e1, e2 = v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]
        area = 0.5 * np.sqrt((np.cross(e1, e2) ** 2).sum(1))
        if not np.isfinite(area).all() or not area.sum() > 0:
            raise ValueError("MeshSampler: the mesh has no finite positive area")
        cdf = np.cumsum(area).astype(np.float32)
        inv = (1.0 / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32)
        self.device = torch.device(device)
        to = lambda a: torch.from_numpy(a).to(self.device)
        self.verts, self.faces, self.cdf = to(v), to(f.astype(np.int32)), to(cdf)
        self.vertex_weights, self.aabb_min, self.aabb_inv_extent = to(w), to(lo), to(inv)

    def sample(self, n, draws=None, generator=None, return_index=False):
        """(points_norm (n, 3), target (n, 24)): the samples in the box's [-1, 1] coordinates and their skinning weights;
        with return_index also (face (n) int32, bary (n, 3), points (n, 3)).  `draws` (n, 3), uniform in [0, 1): the face
        pick and the two barycentric draws of every sample; None draws them with torch.rand on the device (`generator`),
        one launch.  The distribution is trimesh's; the random stream is torch's, not numpy's: a run does not reproduce
        the reference's samples draw for draw.  An explicit `draws` pins everything."""
        n = int(n)
        if n < 0:
            raise ValueError("MeshSampler.sample: n >= 0 expected")
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("MeshSampler.sample: the mesh must live on the GPU (the fused HIP kernels have no CPU fallback)")
        if draws is None:
            draws = torch.rand((n, 3), dtype=torch.float32, device=dev, generator=generator)
        else:
            if tuple(draws.shape) != (n, 3):
                raise ValueError("MeshSampler.sample: draws must be (%d, 3), got %s" % (n, tuple(draws.shape)))
            draws = _dev32(draws, "draws").contiguous()
            if draws.device != dev:
                raise RuntimeError("MeshSampler.sample: draws live on another device than the mesh")
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        points_norm, target = new(n, 3), new(n, BONES)
        face, bary, points = (new(n, dtype=torch.int32), new(n, 3), new(n, 3)) if return_index else (None, None, None)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_mesh_sample(
                n, int(self.verts.shape[0]), int(self.faces.shape[0]), _lib.ptr(self.verts), _lib.ptr(self.faces),
                _lib.ptr(self.cdf), _lib.ptr(self.vertex_weights), _lib.ptr(self.aabb_min), _lib.ptr(self.aabb_inv_extent),
                _lib.ptr(draws), _lib.ptr(points_norm), _lib.ptr(target), _lib.ptr(face), _lib.ptr(bary), _lib.ptr(points),
                _lib.stream_ptr(dev)))
        if return_index:
            return points_norm, target, face, bary, points
        return points_norm, target


def skinning_loss(field, draws=None):
    """SkinningField.get_skinning_loss (models/deformer/rigid.py:198-212) on the device: `field.cfg.n_reg_pts` surface
    samples (or one per row of `draws`, see MeshSampler.sample), field.lbs_network on their normalised positions, and
    `skinning_mse_loss` against their sampled weights.  The sampler is built at the first call from field.smpl_verts,
    field.faces, field.skinning_weights and field.aabb (coord_min, coord_max) and kept on the module as
    `_gsplat_mesh_sampler`.  The voxel-grid path (field.distill) is not supported."""
    if getattr(field, "distill", False):
        raise NotImplementedError("skinning_loss: the distill (voxel-grid) path is not supported")
    sampler = field.__dict__.get("_gsplat_mesh_sampler")
    if sampler is None:
        aabb = field.aabb
        sampler = MeshSampler(field.smpl_verts, field.faces, field.skinning_weights, aabb.coord_min, aabb.coord_max,
                              aabb.coord_min.device)
        field.__dict__["_gsplat_mesh_sampler"] = sampler
    n = int(draws.shape[0]) if draws is not None else int(field.cfg.n_reg_pts)
    points_norm, target = sampler.sample(n, draws=draws)
    return skinning_mse_loss(field.lbs_network(points_norm), target)
