"""The SMPL forward of `pose_correction: direct` (models/pose_correction/pose_correction.py, models/pose_correction/lbs.py)
on the GPU through libgsplat_mi355 (csrc/pose.hip, whose header comment carries the spec): Rodrigues for the 24 joints,
the kinematic chain, the A-pose -> star-pose transforms, the normalised rest joints and the `pose` loss as one autograd
node.  The forward is two launches (the statistics of the shaped template over the vertices, then everything else in one
workgroup), the backward one: no atomics (bitwise reproducible), no host synchronisation, no host-to-device copy,
capture-safe.  `verts_posed`, `v_posed`, `Jtrs_posed` and the pose blend shapes are not computed: training never reads
them (`export()` keeps the reference's torch path).

* `PoseModel(v_template, shapedirs, J_regressor, parents)` -- the body model's constants; folds the joint regressor
  into `J_template` (24, 3) and `J_shapedirs` (24, 3, NB) once, in float64 on the host.
* `smpl_pose_forward(model, betas, root_orient, pose_body, pose_hand, trans, rots_gt=None)`
  -> (rots (1, 24, 9), Jtrs (1, 24, 3), bone_transforms (24, 4, 4), loss_pose or None).
* `pose_correct(module, camera, iteration)` -- DirectPoseOptimization.pose_correct with the fused op
  (`DirectPoseOptimization.pose_correct = pose_correct`).
Device fp32 tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

BONES = _lib.GS_POSE_BONES
MAX_BETAS = _lib.GS_POSE_MAX_BETAS


def _dev32(t, name):
    return _lib.dev32(t, name).detach()


def _parents(parents):
    p = [int(v) for v in (parents.detach().cpu().reshape(-1).tolist() if torch.is_tensor(parents) else list(parents))]
    if len(p) != BONES:
        raise ValueError("pose: parents must have %d entries, got %d" % (BONES, len(p)))
    p[0] = -1  # ignored (SMPL's kintree_table stores -1 or 2^32 - 1 there)
    for i in range(1, BONES):
        if not 0 <= p[i] < i:
            raise ValueError("pose: parents[%d] = %d is not in 0..%d" % (i, p[i], i - 1))
    return p


class PoseModel(object):
    """The constants of the body model: v_template (V, 3) or (1, V, 3), shapedirs (V, 3, NB), J_regressor (24, V), device
    fp32, and the kinematic tree `parents` (24 integers, parents[i] < i; entry 0 is ignored).  The rest joints are linear
    in betas: J_template = J_regressor v_template and J_shapedirs = J_regressor shapedirs are computed here, once, in
    float64 on the host and kept on the device in fp32; the regressor is not read again."""

    def __init__(self, v_template, shapedirs, J_regressor, parents):
        if v_template.dim() == 3 and v_template.shape[0] == 1:
            v_template = v_template[0]
        if v_template.dim() != 2 or v_template.shape[1] != 3 or v_template.shape[0] < 1:
            raise ValueError("pose: v_template must be (V, 3) with V >= 1, got %s" % (tuple(v_template.shape),))
        V = int(v_template.shape[0])
        if shapedirs.dim() != 3 or tuple(shapedirs.shape[:2]) != (V, 3) or not 1 <= shapedirs.shape[2] <= MAX_BETAS:
            raise ValueError("pose: shapedirs must be (%d, 3, NB) with NB in 1..%d, got %s" % (V, MAX_BETAS, tuple(shapedirs.shape)))
        if tuple(J_regressor.shape) != (BONES, V):
            raise ValueError("pose: J_regressor must be (24, %d), got %s" % (V, tuple(J_regressor.shape)))
        self.parents = _parents(parents)
        self.v_template = _dev32(v_template, "v_template").contiguous()
        self.shapedirs = _dev32(shapedirs, "shapedirs").contiguous()
        Jr = _dev32(J_regressor, "J_regressor").double().cpu()
        dev = self.v_template.device
        self.J_template = (Jr @ self.v_template.double().cpu()).to(torch.float32).to(dev)
        self.J_shapedirs = torch.einsum("jv,vkl->jkl", Jr, self.shapedirs.double().cpu()).to(torch.float32).contiguous().to(dev)
        self.V, self.NB, self.device = V, int(shapedirs.shape[2]), dev
        self.workspace_bytes = _lib.nbytes(_lib.load().gs_pose_workspace_bytes, V)

    def args(self, betas, root_orient, pose_body, pose_hand, trans, rots_gt):
        a = _lib.GsPoseArgs()
        a.V, a.NB = self.V, self.NB
        a.parents[:] = self.parents
        for name, t in (("v_template", self.v_template), ("shapedirs", self.shapedirs), ("J_template", self.J_template),
                        ("J_shapedirs", self.J_shapedirs), ("betas", betas), ("root_orient", root_orient),
                        ("pose_body", pose_body), ("pose_hand", pose_hand), ("trans", trans), ("rots_gt", rots_gt)):
            setattr(a, name, _lib.ptr(t))
        return a


class _Pose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, betas, root_orient, pose_body, pose_hand, trans, rots_gt):
        ctx.set_materialize_grads(False)
        betas, root_orient, pose_body, pose_hand, trans = (
            _dev32(t, n).contiguous() for t, n in ((betas, "betas"), (root_orient, "root_orient"), (pose_body, "pose_body"),
                                                   (pose_hand, "pose_hand"), (trans, "trans")))
        if rots_gt is not None:
            rots_gt = _dev32(rots_gt, "rots_gt").contiguous()
        dev = model.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        rots, Jtrs, bone, loss, state = new(1, BONES, 9), new(1, BONES, 3), new(BONES, 4, 4), new(()), new(_lib.GS_POSE_STATE_FLOATS)
        ws = torch.empty(model.workspace_bytes, dtype=torch.uint8, device=dev)
        a = model.args(betas, root_orient, pose_body, pose_hand, trans, rots_gt)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_pose_forward(ctypes.byref(a), _lib.ptr(rots), _lib.ptr(Jtrs), _lib.ptr(bone),
                                                   loss.data_ptr(), _lib.ptr(state), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr(dev)))
        ctx.save_for_backward(betas, root_orient, pose_body, pose_hand, trans, rots_gt, state)
        ctx.model = model
        if rots_gt is None:
            ctx.mark_non_differentiable(loss)
        return rots, Jtrs, bone, loss

    @staticmethod
    def backward(ctx, g_rots, g_Jtrs, g_bone, g_loss):
        betas, root_orient, pose_body, pose_hand, trans, rots_gt, state = ctx.saved_tensors
        need = ctx.needs_input_grad[1:6]
        if not any(need) or (g_rots is None and g_Jtrs is None and g_bone is None and g_loss is None):
            return (None,) * 7
        model = ctx.model
        dev = model.device
        grads = [torch.empty_like(t) if n else None for t, n in zip((betas, root_orient, pose_body, pose_hand, trans), need)]
        ups = [g.to(torch.float32).contiguous() if g is not None else None for g in (g_rots, g_Jtrs, g_bone, g_loss)]
        a = model.args(betas, root_orient, pose_body, pose_hand, trans, rots_gt)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_pose_backward(ctypes.byref(a), _lib.ptr(state), *[_lib.ptr(g) for g in ups],
                                                    *[_lib.ptr(g) for g in grads], _lib.stream_ptr(dev)))
        return (None,) + tuple(grads) + (None,)


def smpl_pose_forward(model, betas, root_orient, pose_body, pose_hand, trans, rots_gt=None):
    """(rots (1, 24, 9), Jtrs (1, 24, 3), bone_transforms (24, 4, 4), loss_pose) of PoseCorrection._forward_smpl and the
    `pose` loss of DirectPoseOptimization.pose_correct, as one autograd node.  betas (1, NB), root_orient (1, 3),
    pose_body (1, 63), pose_hand (1, 6) and trans (1, 3) take gradients; rots_gt ((1, 24, 9) or (24, 9), the dataset's
    camera.rots) takes none, and without it loss_pose is None."""
    if not isinstance(model, PoseModel):
        raise TypeError("pose: a PoseModel expected, got %s" % type(model).__name__)
    named = ((betas, "betas", (1, model.NB)), (root_orient, "root_orient", (1, 3)), (pose_body, "pose_body", (1, 63)),
             (pose_hand, "pose_hand", (1, 6)), (trans, "trans", (1, 3)))
    for t, name, shape in named:
        if tuple(t.shape) != shape:
            raise ValueError("pose: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
    if rots_gt is not None and tuple(rots_gt.shape) not in ((1, BONES, 9), (BONES, 9)):
        raise ValueError("pose: rots_gt must be (1, 24, 9), got %s" % (tuple(rots_gt.shape),))
    for t, name, _ in named + (((rots_gt, "rots_gt", None),) if rots_gt is not None else ()):
        _dev32(t, name)
    rots, Jtrs, bone, loss = _Pose.apply(model, betas, root_orient, pose_body, pose_hand, trans, rots_gt)
    return rots, Jtrs, bone, (loss if rots_gt is not None else None)


def pose_correct(self, camera, iteration):
    """DirectPoseOptimization.pose_correct (models/pose_correction/pose_correction.py:225-252) with the fused op.  Reads
    self.cfg, frame_dict, betas, the four embeddings (root_orients, pose_bodys, pose_hands, trans) and the buffers
    v_template, shapedirs, J_regressor and kintree_table; camera.frame_id, camera.rots, camera.copy() and update().  The
    PoseModel and a device-resident index tensor (sliced by the frame's row: no host-to-device copy per step) are built on
    first use and cached on the module."""
    if iteration < self.cfg.get('delay', 0):
        return camera, {}
    frame = camera.frame_id
    if frame not in self.frame_dict:  # (PoseCorrection.forward returns before it gets here)
        return camera, {}
    dev = self.betas.device
    cache = self.__dict__.get("_gsplat_pose_cache")
    if cache is None or cache[0].device != dev:
        model = PoseModel(self.v_template, self.shapedirs, self.J_regressor, self.kintree_table[0])
        rows = torch.arange(self.root_orients.num_embeddings, dtype=torch.long, device=dev)
        cache = self.__dict__["_gsplat_pose_cache"] = (model, rows)
    model, rows = cache
    row = self.frame_dict[frame]
    idx = rows[row:row + 1]

    rots, Jtrs, bone_transforms, loss_pose = smpl_pose_forward(model, self.betas, self.root_orients(idx), self.pose_bodys(idx),
                                                               self.pose_hands(idx), self.trans(idx), rots_gt=camera.rots)
    updated_camera = camera.copy()
    updated_camera.update(rots=rots, Jtrs=Jtrs, bone_transforms=bone_transforms)
    return updated_camera, {'pose': loss_pose}
