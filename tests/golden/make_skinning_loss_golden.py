"""Generates tests/golden/skinning_loss.npz by EXECUTING the reference's own skinning-regulariser code on the CPU (only
possible where the reference tree exists; the tests only read the .npz).

Taken from the syntax trees and executed, nothing else: SkinningField.get_skinning_loss and SkinningField.softmax with
hierarchical_softmax (models/deformer/rigid.py) and AABB.normalize (utils/dataset_utils.py), with make_golden.py's `torch`
stand-in that allocates its "cuda" tensors on the CPU.  Stand-ins: sample_skinning_loss returns given points and weights
(the reference samples them with trimesh and igl, which are not installed here), lbs_network records the normalised points
it is given and returns a logits leaf, the aabb is a minimal object with coord_min and coord_max.  Each case runs in fp32
(the reference's precision) and in fp64 (make_skinning_golden.py's `_precision`).  Stored: inputs, the normalised points,
the loss and its autograd gradient with respect to the logits; nothing of the reference's text.

Keys: "<case>/{logits,target,points}" (fp32 inputs; the fp64 runs use the same values), "aabb_min", "aabb_max",
"<case>/{loss,dlogits,pnorm}_{f32,f64res}" (fp64 results as float32 residuals where that loses nothing, as in
skinning.npz; tests/skinning_ref.py load_fixture adds them back).
  a  hierarchical (25 logits), 96 rows
  b  softmax over 24 logits, 64 rows
  c  hierarchical with saturated logits (|x| 20-1000: 1 - s rounds to 0 in fp32), 48 rows
  d  hierarchical, n = 1024 (the default n_reg_pts)

Run:  python tests/golden/make_skinning_loss_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _CpuTorch, _exec_nodes, _load_functions, _method  # noqa: E402
from make_skinning_golden import _Obj, _precision  # noqa: E402

RIGID = "models/deformer/rigid.py"
CASES = (("a", 25, 96, False), ("b", 24, 64, False), ("c", 25, 48, True), ("d", 25, 1024, False))
AABB_MIN, AABB_MAX = np.array([-1.1, -1.3, -0.4], np.float32), np.array([1.1, 0.9, 0.5], np.float32)


def _reference():
    T = _CpuTorch()
    ns = _load_functions(RIGID, ["hierarchical_softmax"], dict(torch=T, F=F))
    scope = dict(torch=T, F=F, hierarchical_softmax=ns["hierarchical_softmax"])
    fns = {}
    for rel, cls, name in ((RIGID, "SkinningField", "softmax"), (RIGID, "SkinningField", "get_skinning_loss"),
                           ("utils/dataset_utils.py", "AABB", "normalize")):
        node, path = _method(rel, cls, name)
        fns[name] = _exec_nodes([node], path, scope)[name]
    return fns


def _run_case(fns, logits, target, points):
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            leaf = torch.from_numpy(logits).to(dt).requires_grad_(True)
            seen = {}

            def lbs_network(x, leaf=leaf, seen=seen):
                seen["pnorm"] = x
                return leaf

            aabb = _Obj(coord_min=torch.from_numpy(AABB_MIN).to(dt), coord_max=torch.from_numpy(AABB_MAX).to(dt))
            aabb.normalize = lambda x, sym=False, a=aabb: fns["normalize"](a, x, sym=sym)
            this = _Obj(distill=False, aabb=aabb, lbs_network=lbs_network)
            this.sample_skinning_loss = lambda: (torch.from_numpy(points).to(dt), torch.from_numpy(target).to(dt))
            this.softmax = lambda logit, t=this: fns["softmax"](t, logit)
            loss = fns["get_skinning_loss"](this)
            assert loss.dtype == dt and loss.dim() == 0 and seen["pnorm"].dtype == dt, (loss.dtype, loss.shape)
            (dx,) = torch.autograd.grad(loss, [leaf])
        out["loss_" + tag] = loss.detach().numpy()
        out["dlogits_" + tag] = dx.numpy()
        out["pnorm_" + tag] = seen["pnorm"].detach().numpy()
    return out


def main():
    fns = _reference()
    rng = np.random.default_rng(2025)
    short = lambda a: (np.round(a * 64) / 64).astype(np.float32)  # (short mantissas: they compress)
    out = {"aabb_min": AABB_MIN, "aabb_max": AABB_MAX}
    for key, width, n, saturated in CASES:
        if saturated:
            logits = (rng.uniform(20.0, 1000.0, size=(n, width)) * rng.choice([-1.0, 1.0], size=(n, width))).astype(np.float32)
        else:
            logits = short(rng.normal(scale=2.0, size=(n, width)))
        # weights as a mesh gives them: blends of three sparse rows
        rows = rng.dirichlet(np.full(24, 0.1), size=(n, 3))
        bary = rng.dirichlet(np.ones(3), size=n)
        target = (rows * bary[:, :, None]).sum(1).astype(np.float32)
        points = short(rng.uniform(AABB_MIN, AABB_MAX, size=(n, 3)))
        res = _run_case(fns, logits, target, points)
        out.update({"%s/%s" % (key, k): v for k, v in dict(logits=logits, target=target, points=points).items()})
        out.update({"%s/%s" % (key, k): v for k, v in res.items()})
    for k in [k for k in out if k.endswith("_f64")]:
        f32 = out[k[:-4] + "_f32"].astype(np.float64)
        res = (out[k] - f32).astype(np.float32)
        if np.abs(f32 + res - out[k]).max() <= 1e-14 * np.abs(out[k]).max():  # (else kept whole)
            out[k + "res"] = res
            del out[k]
    path = os.path.join(HERE, "skinning_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
