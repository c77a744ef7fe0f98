"""The non-rigid deformer around its MLP (models/deformer/non_rigid.py) on the GPU through libgsplat_mi355
(csrc/nonrigid.hip, whose header comment carries the spec): the hierarchical pose encoder in front of the MLP
(models/network_utils.py HierarchicalPoseEncoder: a batch-1 network walked joint by joint) and the application of the
MLP's (N, 10 + F) output to positions, scales and rotations with the three `nr_*` regularisers behind it.  Each is one
forward launch and one backward launch (the regularisers add one small fixed-order sum): no atomics (bitwise
reproducible), no host synchronisation, no host-to-device copy per call, capture-safe.  The MLP between them stays a torch
module (whose forward is gsplat_mi355.mlp.mlp_forward or gsplat_mi355.wide_mlp.hannw_mlp_forward).

* `pose_encode(module, rots, Jtrs)` -> (1, 24 d): the encoder's 24 per-joint outputs, before `out_layer`.
* `hierarchical_pose_encoder_forward(self, rots, Jtrs, skinning_weight=None)` -- HierarchicalPoseEncoder.forward.
* `nonrigid_apply(deltas, xyz, scaling, rotation, scale_offset="logit", rot_offset="add", compute_loss=True)`
  -> (xyz', scaling', rotation', feature or None, {nr_xyz, nr_scale, nr_rot} or {}).
* `nonrigid_forward(self, gaussians, iteration, camera, compute_loss=True)` -- HashGridwithMLP.forward and MLP.forward
  ("The non-rigid deformer").
* `hannw_forward(self, gaussians, iteration, camera, compute_loss=True)` -- HannwMLP.forward, whose MLP is a HannwCondMLP
  (gsplat_mi355.wide_mlp.hannw_mlp_forward).
One difference from the reference: with `rot_offset: mult` it writes 1 into column 6 of the MLP's output in place; the
fused op leaves `deltas` untouched (that column takes a zero gradient either way).
Device fp32 tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

JOINTS = _lib.GS_POSE_ENC_JOINTS
MAX_DIM = _lib.GS_POSE_ENC_MAX_DIM
SCALE_OFFSETS = {"logit": _lib.GS_NR_SCALE_LOGIT, "exp": _lib.GS_NR_SCALE_EXP, "zero": _lib.GS_NR_SCALE_ZERO}
ROT_OFFSETS = {"add": _lib.GS_NR_ROT_ADD, "mult": _lib.GS_NR_ROT_MULT}


def _dev32(t, name):
    return _lib.dev32(t, name).detach()


# ---- the pose encoder
def _parents(parents):
    p = [int(v) for v in (parents.detach().cpu().reshape(-1).tolist() if torch.is_tensor(parents) else list(parents))]
    if len(p) != JOINTS:
        raise ValueError("pose encoder: the tree must have %d entries, got %d" % (JOINTS, len(p)))
    p[0] = -1  # ignored
    for i in range(1, JOINTS):
        if not 0 <= p[i] < i:
            raise ValueError("pose encoder: parents[%d] = %d is not in 0..%d" % (i, p[i], i - 1))
    return tuple(p)


def grad_layout(d):
    """[(offset, shape)] of the 98 parameter gradients in the packed buffer: W0, b0, then W1_j, b1_j, W2_j, b2_j."""
    m = 13 + d
    shapes = [(d, 12 * JOINTS), (d,)] + [(m, m), (m,), (d, m), (d,)] * JOINTS
    out, off = [], 0
    for s in shapes:
        n = s[0] * (s[1] if len(s) > 1 else 1)
        out.append((off, s))
        off += n
    return out, off


def _enc_args(d, parents, rots, Jtrs, params):
    a = _lib.GsPoseEncArgs()
    a.d = d
    a.parents[:] = parents
    a.rots, a.Jtrs, a.W0, a.b0 = _lib.ptr(rots), _lib.ptr(Jtrs), params[0].data_ptr(), params[1].data_ptr()
    for j in range(JOINTS):
        a.W1[j], a.b1[j], a.W2[j], a.b2[j] = (params[2 + 4 * j + k].data_ptr() for k in range(4))
    return a


class _PoseEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rots, Jtrs, d, parents, *params):
        ctx.set_materialize_grads(False)
        rots, Jtrs = _dev32(rots, "rots").contiguous(), _dev32(Jtrs, "Jtrs").contiguous()
        params = tuple(p.detach().contiguous() for p in params)
        dev = rots.device
        out = torch.empty(1, JOINTS * d, dtype=torch.float32, device=dev)
        state = torch.empty(_lib.GS_POSE_ENC_STATE_FLOATS, dtype=torch.float32, device=dev)
        a = _enc_args(d, parents, rots, Jtrs, params)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_pose_encoder_forward(ctypes.byref(a), _lib.ptr(out), _lib.ptr(state), _lib.stream_ptr(dev)))
        ctx.save_for_backward(state, *params)
        ctx.d, ctx.parents = d, parents
        return out

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        n_in = len(need)
        if g is None or not any(need):
            return (None,) * n_in
        state, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dev, d = state.device, ctx.d
        layout, total = grad_layout(d)
        packed = torch.empty(total, dtype=torch.float32, device=dev) if any(need[4:]) else None
        drots = torch.empty(1, JOINTS, 9, dtype=torch.float32, device=dev) if need[0] else None
        dJtrs = torch.empty(1, JOINTS, 3, dtype=torch.float32, device=dev) if need[1] else None
        g = g.to(torch.float32).contiguous()
        a = _enc_args(d, ctx.parents, None, None, params)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_pose_encoder_backward(ctypes.byref(a), _lib.ptr(state), _lib.ptr(g), _lib.ptr(packed),
                                                            _lib.ptr(drots), _lib.ptr(dJtrs), _lib.stream_ptr(dev)))
        grads = [packed[off:off + torch.Size(shape).numel()].view(shape) if n else None
                 for (off, shape), n in zip(layout, need[4:])]
        return (drots, dJtrs, None, None) + tuple(grads)


def _encoder_params(module):
    d = int(module.layer_0.out_features)
    params = [module.layer_0.weight, module.layer_0.bias]
    for layer in module.layers:
        params += [layer[0].weight, layer[0].bias, layer[2].weight, layer[2].bias]
    return d, params


def pose_encode(module, rots, Jtrs):
    """The 24 per-joint outputs of a HierarchicalPoseEncoder-shaped `module` (layer_0: Linear(288, d); layers[j]:
    Sequential(Linear(13 + d, 13 + d), ReLU, Linear(13 + d, d)); ktree_parents; rel_joints False) for rots (1, 24, 9) and
    Jtrs (1, 24, 3), as one autograd node: (1, 24 d), before `out_layer`.  The parameters stay the module's own; their
    gradients are views of one packed buffer."""
    if getattr(module, "rel_joints", False):
        raise NotImplementedError("pose encoder: rel_joints=True is not supported")
    if int(getattr(module, "num_joints", JOINTS)) != JOINTS or len(module.layers) != JOINTS:
        raise NotImplementedError("pose encoder: 24 joints expected")
    if rots.shape[0] != 1 or Jtrs.shape[0] != 1:
        raise NotImplementedError("pose encoder: batch 1 expected, got %d" % rots.shape[0])
    d, params = _encoder_params(module)
    if not 1 <= d <= MAX_DIM:
        raise NotImplementedError("pose encoder: dim_per_joint must be in 1..%d, got %d" % (MAX_DIM, d))
    if rots.numel() != JOINTS * 9 or Jtrs.numel() != JOINTS * 3:
        raise ValueError("pose encoder: rots (1, 24, 9) and Jtrs (1, 24, 3) expected, got %s and %s"
                         % (tuple(rots.shape), tuple(Jtrs.shape)))
    layout, _ = grad_layout(d)
    for k, (p, (_, shape)) in enumerate(zip(params, layout)):
        if tuple(p.shape) != shape:
            raise ValueError("pose encoder: parameter %d must be %s, got %s" % (k, shape, tuple(p.shape)))
    parents = _parents(module.ktree_parents)
    for t, name in [(rots, "rots"), (Jtrs, "Jtrs")] + [(p, "parameter %d" % k) for k, p in enumerate(params)]:
        _dev32(t, name)
    return _PoseEncode.apply(rots, Jtrs, d, parents, *params)


def hierarchical_pose_encoder_forward(self, rots, Jtrs, skinning_weight=None):
    """HierarchicalPoseEncoder.forward (models/network_utils.py:151-180) with the fused op; `out_layer` (an nn.Linear
    where out_dim > 0, else the identity) stays in torch."""
    return self.out_layer(pose_encode(self, rots, Jtrs))


# ---- the delta application
class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, deltas, xyz, scaling, rotation, smode, rmode, compute_loss):
        ctx.set_materialize_grads(False)
        deltas = _lib.contiguous_aligned(_dev32(deltas, "deltas"))
        xyz = _dev32(xyz, "xyz").contiguous()
        rotation = _lib.contiguous_aligned(_dev32(rotation, "rotation"))
        zero = smode == _lib.GS_NR_SCALE_ZERO
        scaling = None if zero else _dev32(scaling, "scaling").contiguous()
        dev, n, D = deltas.device, int(deltas.shape[0]), int(deltas.shape[1])
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        xyz_o, scal_o, rot_o, feat = new(n, 3), new(0 if zero else n, 3), new(n, 4), new(n, D - 10)
        losses = new(3) if compute_loss else None
        if n == 0:
            if compute_loss:
                losses.fill_(float("nan"))  # the mean of no rows, as torch has it
        else:
            L = _lib.load()
            ws = new(_lib.nbytes(L.gs_nonrigid_workspace_bytes, n, D) // 4) if compute_loss else None
            with _lib.on_device(dev):
                _lib.check(L.gs_nonrigid_apply_forward(n, D, smode, rmode, _lib.ptr(deltas), _lib.ptr(xyz), _lib.ptr(scaling),
                                                       _lib.ptr(rotation), _lib.ptr(xyz_o), _lib.ptr(scal_o), _lib.ptr(rot_o),
                                                       _lib.ptr(feat), _lib.ptr(losses), _lib.ptr(ws),
                                                       4 * ws.numel() if ws is not None else 0, _lib.stream_ptr(dev)))
        ctx.save_for_backward(deltas, scaling if smode == _lib.GS_NR_SCALE_EXP else None,
                              rotation if rmode == _lib.GS_NR_ROT_MULT else None)
        ctx.modes = (smode, rmode)
        nr = tuple(losses[k] for k in range(3)) if compute_loss else (new(0), new(0), new(0))
        if zero:
            ctx.mark_non_differentiable(scal_o, nr[1])
        if not compute_loss:
            ctx.mark_non_differentiable(*nr)
        return (xyz_o, scal_o, rot_o, feat) + nr

    @staticmethod
    def backward(ctx, g_xyz, g_scal, g_rot, g_feat, g_nrx, g_nrs, g_nrr):
        deltas, scaling, rotation = ctx.saved_tensors
        smode, rmode = ctx.modes
        need_d, need_x, need_s, need_r = ctx.needs_input_grad[:4]
        ups = (g_xyz, g_scal, g_rot, g_feat, g_nrx, g_nrs, g_nrr)
        if not (need_d or need_x or need_s or need_r) or all(g is None for g in ups):
            return (None,) * 7
        dev, n, D = deltas.device, int(deltas.shape[0]), int(deltas.shape[1])
        cont = lambda g, a16=False: None if g is None else (_lib.contiguous_aligned(g.to(torch.float32)) if a16
                                                            else g.to(torch.float32).contiguous())
        g_xyz, g_scal, g_rot, g_feat = cont(g_xyz), cont(g_scal), cont(g_rot, True), cont(g_feat, True)
        g_nrx, g_nrs, g_nrr = cont(g_nrx), cont(g_nrs), cont(g_nrr)
        # scaling and rotation take the upstream gradient as it is unless their mode bends it
        exp, mult = smode == _lib.GS_NR_SCALE_EXP, rmode == _lib.GS_NR_ROT_MULT
        dd = torch.empty_like(deltas) if need_d else None
        ds = torch.empty(n, 3, dtype=torch.float32, device=dev) if (need_s and exp and g_scal is not None) else None
        dr = torch.empty(n, 4, dtype=torch.float32, device=dev) if (need_r and mult and g_rot is not None) else None
        if n > 0 and (dd is not None or ds is not None or dr is not None):
            with _lib.on_device(dev):
                _lib.check(_lib.load().gs_nonrigid_apply_backward(
                    n, D, smode, rmode, _lib.ptr(deltas), _lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(g_xyz), _lib.ptr(g_scal),
                    _lib.ptr(g_rot), _lib.ptr(g_feat), _lib.ptr(g_nrx), _lib.ptr(g_nrs), _lib.ptr(g_nrr), _lib.ptr(dd),
                    _lib.ptr(ds), _lib.ptr(dr), _lib.stream_ptr(dev)))
        if need_s and not exp:
            ds = g_scal
        if need_r and not mult:
            dr = g_rot
        return dd, (g_xyz if need_x else None), (ds if need_s else None), (dr if need_r else None), None, None, None


def nonrigid_apply(deltas, xyz, scaling, rotation, scale_offset="logit", rot_offset="add", compute_loss=True):
    """(xyz', scaling', rotation', feature, losses) of the non-rigid deformer's tail: deltas (N, 10 + F) split into a
    position offset (added), a scale offset (`logit`: added; `exp`: log(max(exp(scaling) + offset, 1e-6)); `zero`:
    ignored, scaling' is `scaling` itself), a rotation offset (`add`: added; `mult`: (1, deltas[7:10]) Hamilton-multiplied
    onto `rotation`) and F feature columns (a contiguous (N, F) tensor; None when F = 0).  losses = {nr_xyz, nr_scale,
    nr_rot} (means of the L2 / L1 / L1 norms of the offsets), or {} without compute_loss.  One autograd node."""
    if scale_offset not in SCALE_OFFSETS or rot_offset not in ROT_OFFSETS:
        raise ValueError("nonrigid_apply: scale_offset in %s and rot_offset in %s expected, got %r and %r"
                         % (sorted(SCALE_OFFSETS), sorted(ROT_OFFSETS), scale_offset, rot_offset))
    if deltas.dim() != 2 or not 10 <= deltas.shape[1] <= _lib.GS_NONRIGID_MAX_D:
        raise ValueError("nonrigid_apply: deltas must be (N, 10 + F) with at most %d columns, got %s"
                         % (_lib.GS_NONRIGID_MAX_D, tuple(deltas.shape)))
    n = int(deltas.shape[0])
    if tuple(xyz.shape) != (n, 3) or tuple(scaling.shape) != (n, 3) or tuple(rotation.shape) != (n, 4):
        raise ValueError("nonrigid_apply: xyz (N, 3), scaling (N, 3) and rotation (N, 4) with N = %d expected, got %s, %s and %s"
                         % (n, tuple(xyz.shape), tuple(scaling.shape), tuple(rotation.shape)))
    for t, name in ((deltas, "deltas"), (xyz, "xyz"), (scaling, "scaling"), (rotation, "rotation")):
        _dev32(t, name)
    smode, rmode = SCALE_OFFSETS[scale_offset], ROT_OFFSETS[rot_offset]
    zero = smode == _lib.GS_NR_SCALE_ZERO
    xyz_o, scal_o, rot_o, feat, nrx, nrs, nrr = _Apply.apply(deltas, xyz, None if zero else scaling, rotation, smode, rmode,
                                                             bool(compute_loss))
    losses = {"nr_xyz": nrx, "nr_scale": nrs, "nr_rot": nrr} if compute_loss else {}
    return xyz_o, (scaling if zero else scal_o), rot_o, (feat if deltas.shape[1] > 10 else None), losses


def nonrigid_forward(self, gaussians, iteration, camera, compute_loss=True):
    """HashGridwithMLP.forward (models/deformer/non_rigid.py:226-300) and MLP.forward (:55-131) with the fused pose
    encoder and the fused delta application; `self.hashgrid` is used when the module has one.  Reads self.cfg, delay,
    feature_dim, latent_dim (with frame_dict and latent), pose_encoder, aabb, mlp; camera.rots / Jtrs / frame_id;
    gaussians.get_xyz / _xyz / _scaling / _rotation / clone().  The latent row's index is a slice of a device tensor
    cached on the module: no host-to-device copy per step."""
    if iteration < self.delay:
        deformed_gaussians = gaussians.clone()
        if self.feature_dim > 0:
            xyz = gaussians.get_xyz
            setattr(deformed_gaussians, "non_rigid_feature", torch.zeros(xyz.shape[0], self.feature_dim, device=xyz.device))
        return deformed_gaussians, {}
    pose_feat = hierarchical_pose_encoder_forward(self.pose_encoder, camera.rots, camera.Jtrs)
    if self.latent_dim > 0:
        row = self.frame_dict.get(camera.frame_id, len(self.frame_dict) - 1)  # an unknown frame takes the last code
        rows = self.__dict__.get("_gsplat_latent_rows")
        if rows is None or rows.device != pose_feat.device:
            rows = self.__dict__["_gsplat_latent_rows"] = torch.arange(self.latent.num_embeddings, dtype=torch.long,
                                                                       device=pose_feat.device)
        latent_code = self.latent(rows[row:row + 1]).expand(pose_feat.shape[0], -1)
        pose_feat = torch.cat([pose_feat, latent_code], dim=1)
    xyz_norm = self.aabb.normalize(gaussians.get_xyz, sym=True)
    hashgrid = getattr(self, "hashgrid", None)
    deltas = self.mlp(hashgrid(xyz_norm) if hashgrid is not None else xyz_norm, cond=pose_feat)
    xyz, scaling, rotation, feature, loss_reg = nonrigid_apply(
        deltas, gaussians._xyz, gaussians._scaling, gaussians._rotation, scale_offset=self.cfg.get('scale_offset', 'logit'),
        rot_offset=self.cfg.get('rot_offset', 'add'), compute_loss=compute_loss)
    deformed_gaussians = gaussians.clone()
    deformed_gaussians._xyz, deformed_gaussians._scaling, deformed_gaussians._rotation = xyz, scaling, rotation
    if self.feature_dim > 0:
        setattr(deformed_gaussians, "non_rigid_feature", feature)
    return deformed_gaussians, loss_reg


def hannw_forward(self, gaussians, iteration, camera, compute_loss=True):
    """HannwMLP.forward (models/deformer/non_rigid.py:146-201) with the fused pose encoder, `self.mlp(xyz_norm, iteration,
    cond=pose_feat)` (a HannwCondMLP: wide_mlp.hannw_mlp_forward) and the fused delta application (no feature columns).
    Before `cfg.mlp.embedder.kick_in_iter` the deltas are multiplied by zeros, as the reference does: the MLP's parameters
    then take ZERO gradients, not None ones, which is what keeps Adam's step count the reference's."""
    pose_feat = hierarchical_pose_encoder_forward(self.pose_encoder, camera.rots, camera.Jtrs)
    xyz_norm = self.aabb.normalize(gaussians.get_xyz, sym=True)
    deltas = self.mlp(xyz_norm, iteration, cond=pose_feat)
    if iteration < self.cfg.mlp.embedder.kick_in_iter:
        deltas = deltas * torch.zeros_like(deltas)
    xyz, scaling, rotation, _, loss_reg = nonrigid_apply(
        deltas, gaussians._xyz, gaussians._scaling, gaussians._rotation, scale_offset=self.cfg.get('scale_offset', 'logit'),
        rot_offset=self.cfg.get('rot_offset', 'add'), compute_loss=compute_loss)
    deformed_gaussians = gaussians.clone()
    deformed_gaussians._xyz, deformed_gaussians._scaling, deformed_gaussians._rotation = xyz, scaling, rotation
    return deformed_gaussians, loss_reg
