"""Generates tests/golden/pose.npz by EXECUTING the reference's own pose-correction code on the CPU (only possible where
the reference tree exists; the tests only read the .npz).

Taken from the syntax trees and executed, nothing else: lbs, vertices2joints, blend_shapes, batch_rodrigues,
transform_mat and batch_rigid_transform (models/pose_correction/lbs.py), get_transforms_02v,
PoseCorrection._forward_smpl and DirectPoseOptimization.pose_correct (models/pose_correction/pose_correction.py; scipy
builds the two z rotations, as there).  Stand-ins: the module is a plain object with the reference's attribute names, its
four embeddings are three-row leaf tables looked up at row 1, the camera is a minimal object with copy() / update().
SMPL's data files are not available, so the body models are synthetic and seeded (tests/pose_ref.py synthetic_model: a
few hundred vertices, regressor rows non-negative and summing to 1, the SMPL tree); posedirs and lbs_weights, which
none of the stored results depends on, are random.  Each case runs in fp32 (the reference's precision) and in fp64:
there the default dtype is float64, the `torch` the reference sees answers `torch.float32` with the default dtype and
Tensor.float() is the identity, so nothing is rounded to fp32.

Stored per case: the inputs ("<case>/{v_template,shapedirs,J_regressor,parents,betas,root_orient,pose_body,pose_hand,
trans,rots_gt}"), the seeded upstream gradients ("<case>/{g_rots,g_Jtrs,g_bone,g_loss}"), and, as
"<case>/<name>_{f32,f64res}", the four outputs (rots, Jtrs, bone_transforms, loss_pose) and the five autograd gradients
(dbetas, droot_orient, dpose_body, dpose_hand, dtrans) of sum(g_rots rots) + sum(g_Jtrs Jtrs) + sum(g_bone
bone_transforms) + g_loss loss_pose.  An fp64 result is stored as its float32 residual from the fp32 one
(tests/pose_ref.py load_fixture adds them back) when that gives it back to 1e-14 of its largest magnitude, and whole
otherwise.  "bar/<name>": the fp32 reference's own error against its fp64 run, as a fraction of the tensor's largest
magnitude, the largest over the cases (printed per case).
  a  a generic pose, angles up to ~1 rad, NB = 10, V = 300
  b  pose_hand exactly zero (ZJU-MoCap), body row 4 exactly zero, body row 9 of magnitude 1e-6
  c  rows near pi ("c/near_pi": along an axis, so one coordinate is within 1e-3 of +-pi, and in general directions) and
     one near 3 pi ("c/near_3pi")
  d  NB = 6, V = 257, every shaped coordinate positive
  e  V = 333, every shaped coordinate negative

Run:  python tests/golden/make_pose_golden.py
"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _CpuTorch, _exec_nodes, _load_functions, _method  # noqa: E402
import pose_ref  # noqa: E402

LBS = "models/pose_correction/lbs.py"
PC = "models/pose_correction/pose_correction.py"
OUTS, GRADS = pose_ref.OUTS, pose_ref.GRADS


class _Torch(_CpuTorch):
    """make_golden.py's stand-in, whose `float32` is the default dtype (the reference's explicit dtype arguments then do
    not round in the fp64 run)."""

    @property
    def float32(self):
        return torch.get_default_dtype()


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Camera(_Obj):
    def copy(self):
        return _Camera(**self.__dict__)

    def update(self, **kw):
        self.__dict__.update(kw)


@contextlib.contextmanager
def _precision(dt):
    if dt == torch.float32:
        yield
        return
    prev, float_ = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(torch.float64)
    torch.Tensor.float = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.set_default_dtype(prev)
        torch.Tensor.float = float_


def _reference():
    T = _Torch()
    ns = _load_functions(LBS, ["lbs", "vertices2joints", "blend_shapes", "batch_rodrigues", "transform_mat",
                               "batch_rigid_transform"], dict(torch=T, F=F))
    ns02 = _load_functions(PC, ["get_transforms_02v"], dict(torch=T, F=F, np=np))
    scope = dict(torch=T, F=F, np=np, lbs=ns["lbs"], get_transforms_02v=ns02["get_transforms_02v"], Tuple=tuple, Dict=dict)
    fns = {}
    for cls, name in (("PoseCorrection", "_forward_smpl"), ("DirectPoseOptimization", "pose_correct")):
        node, path = _method(PC, cls, name)
        node.returns = None  # (the annotation names typing.Tuple; it is not evaluated)
        fns[name] = _exec_nodes([node], path, scope)[name]
    return fns


def _run_case(fns, model, inp, ups, rng):
    V = model["v_template"].shape[0]
    posedirs = rng.normal(scale=0.01, size=(207, V * 3)).astype(np.float32)
    lbs_weights = rng.dirichlet(np.full(24, 0.3), size=V).astype(np.float32)
    kintree = np.stack([model["parents"], np.arange(24, dtype=np.int32)]).astype(np.int32)
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
            leaves = {"betas": t(inp["betas"]).requires_grad_(True)}
            tables = {}
            for name in ("root_orient", "pose_body", "pose_hand", "trans"):
                tab = torch.zeros(3, inp[name].shape[1], dtype=dt)
                tab[1] = t(inp[name])[0]
                tables[name] = tab.requires_grad_(True)
            this = _Obj(cfg=dict(delay=100), frame_dict={7: 0, 11: 1, 13: 2}, betas=leaves["betas"],
                        root_orients=lambda i: tables["root_orient"][i], pose_bodys=lambda i: tables["pose_body"][i],
                        pose_hands=lambda i: tables["pose_hand"][i], trans=lambda i: tables["trans"][i],
                        v_template=t(model["v_template"]).unsqueeze(0), shapedirs=t(model["shapedirs"]),
                        posedirs=t(posedirs), J_regressor=t(model["J_regressor"]), lbs_weights=t(lbs_weights),
                        kintree_table=torch.from_numpy(kintree))
            this._forward_smpl = lambda *a: fns["_forward_smpl"](this, *a)
            camera = _Camera(frame_id=11, rots=t(inp["rots_gt"]), Jtrs=None, bone_transforms=None)
            same, nothing = fns["pose_correct"](this, camera, 99)  # below `delay`: the camera itself and {}
            assert same is camera and nothing == {}
            cam, losses = fns["pose_correct"](this, camera, 100)
            res = dict(rots=cam.rots, Jtrs=cam.Jtrs, bone_transforms=cam.bone_transforms, loss_pose=losses["pose"])
            assert all(v.dtype == dt for v in res.values()), [v.dtype for v in res.values()]
            assert tuple(cam.rots.shape) == (1, 24, 9) and tuple(cam.Jtrs.shape) == (1, 24, 3)
            loss = ((res["rots"] * t(ups["g_rots"])).sum() + (res["Jtrs"] * t(ups["g_Jtrs"])).sum()
                    + (res["bone_transforms"] * t(ups["g_bone"])).sum() + res["loss_pose"] * float(ups["g_loss"]))
            wrt = [leaves["betas"]] + [tables[n] for n in ("root_orient", "pose_body", "pose_hand", "trans")]
            grads = torch.autograd.grad(loss, wrt)
            for g in grads[1:]:  # only the row looked up sees a gradient
                assert not g[0].any() and not g[2].any()
            grads = [grads[0]] + [g[1:2] for g in grads[1:]]
        for name in OUTS:
            out["%s_%s" % (name, tag)] = res[name].detach().numpy()
        for name, g in zip(GRADS, grads):
            out["%s_%s" % (name, tag)] = g.numpy()
    return out


def _pose(rng, scale):
    aa = rng.normal(size=(24, 3))
    aa = aa / np.linalg.norm(aa, axis=1, keepdims=True) * rng.uniform(0.05, scale, size=(24, 1))
    return aa


def main():
    fns = _reference()
    rng = np.random.default_rng(2025)
    out, bars = {}, {}

    def case(key, model, aa, NB, extra=None):
        aa = aa.astype(np.float32)
        inp = dict(betas=rng.normal(scale=1.0, size=(1, NB)).clip(-3, 3).astype(np.float32), root_orient=aa[:1].reshape(1, 3),
                   pose_body=aa[1:22].reshape(1, 63), pose_hand=aa[22:].reshape(1, 6),
                   trans=rng.normal(scale=0.5, size=(1, 3)).astype(np.float32))
        gt = np.stack([pose_ref.rodrigues(r) for r in aa.astype(np.float64) + rng.normal(scale=0.05, size=(24, 3))])
        inp["rots_gt"] = gt.reshape(1, 24, 9).astype(np.float32)
        ups = dict(g_rots=rng.normal(size=(1, 24, 9)).astype(np.float32), g_Jtrs=rng.normal(size=(1, 24, 3)).astype(np.float32),
                   g_bone=rng.normal(size=(24, 4, 4)).astype(np.float32), g_loss=np.float32(rng.uniform(0.5, 2.0) * 10.0))
        res = _run_case(fns, model, inp, ups, rng)
        for d in (model, inp, ups, res, extra or {}):
            out.update({"%s/%s" % (key, k): v for k, v in d.items()})
        for name in OUTS + GRADS:
            f32, f64 = res[name + "_f32"].astype(np.float64), res[name + "_f64"]
            err = float(np.abs(f32 - f64).max() / np.abs(f64).max())
            bars[name] = max(bars.get(name, 0.0), err)
            print("%s %-16s fp32 reference vs fp64: %.3g of the largest magnitude" % (key, name, err))

    case("a", pose_ref.synthetic_model(300, 10, seed=1), _pose(rng, 1.0), 10)
    aa = _pose(rng, 1.0)
    aa[22:] = 0.0
    aa[1 + 4] = 0.0
    aa[1 + 9] *= 1e-6 / np.linalg.norm(aa[1 + 9])
    case("b", pose_ref.synthetic_model(300, 10, seed=2), aa, 10)
    aa = _pose(rng, 1.0)
    near_pi, near_3pi = np.array([2, 5, 8, 12, 16, 19]), np.array([21])
    for k, j in enumerate(near_pi):
        if k < 3:  # along an axis: one coordinate near +-pi
            v = rng.normal(scale=1e-4, size=3)
            v[k] = (np.pi - rng.uniform(1e-5, 5e-4)) * (-1.0 if k == 1 else 1.0)
            aa[j] = v
        else:
            aa[j] *= (np.pi + rng.uniform(-5e-4, 5e-4)) / np.linalg.norm(aa[j])
    aa[near_3pi[0]] *= (3 * np.pi - 3e-4) / np.linalg.norm(aa[near_3pi[0]])
    case("c", pose_ref.synthetic_model(300, 10, seed=3), aa, 10, dict(near_pi=near_pi, near_3pi=near_3pi))
    case("d", pose_ref.synthetic_model(257, 6, seed=4, sign=1), _pose(rng, 1.0), 6)
    case("e", pose_ref.synthetic_model(333, 10, seed=5, sign=-1), _pose(rng, 1.0), 10)

    for name, v in bars.items():
        out["bar/" + name] = np.float64(v)
        print("bar/%-16s %.3g%s" % (name, v, "  (beyond 2.5e-6: the test's bar becomes four times this)" if v > 2.5e-6 else ""))
    for k in [k for k in out if k.endswith("_f64")]:
        f32 = out[k[:-4] + "_f32"].astype(np.float64)
        res = (out[k] - f32).astype(np.float32)
        if np.abs(f32 + res - out[k]).max() <= 1e-14 * np.abs(out[k]).max():  # (else kept whole)
            out[k + "res"] = res
            del out[k]
    path = os.path.join(HERE, "pose.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
