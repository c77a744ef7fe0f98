"""Generates tests/golden/skinning.npz by EXECUTING the reference's own rigid-deformer code on the CPU (only possible
where the reference tree exists; the tests only read the .npz).

Taken from the syntax trees and executed, nothing else: hierarchical_softmax, SkinningField.softmax /
get_forward_transform / forward and SMPLNN.forward (models/deformer/rigid.py), build_rotation (utils/general_utils.py,
with make_golden.py's `torch` stand-in that allocates its "cuda" tensors on the CPU).  Stand-ins: lbs_network returns a
logits leaf, query_weights a weights leaf, the aabb and the Gaussians are minimal objects.  Each case runs in fp32 (the
reference's precision) and in fp64: there the default dtype is float64 and Tensor.float() (the reference's casts) is the
identity, so nothing is rounded to fp32.  Stored: inputs, x_bar, R_bar, T_fwd and the autograd gradients of the
logits / weights, tfs, xyz and quaternions for seeded upstream gradients g and G; nothing of the reference's text.

Keys: "<case>/{w,tfs,xyz,rot,g,G}" (fp32 inputs; the fp64 runs use the same values), "<case>/kind",
"<case>/{xbar,Rbar,T,dw,dtfs,dxyz,drot}_{f32,f64res}"; case f: "f/{x,gW}", "f/{W,dx}_{f32,f64res}".  An fp64 result is
stored as its float32 residual from the fp32 one (`_f64res` = float32(f64 - f32); tests/skinning_ref.py load_fixture
adds them back) when that gives it back to 1e-14 of its largest magnitude, and whole otherwise: this halves the file.
  a  hierarchical (25 logits), a body-like cloud, SMPL-like rigid tfs, unnormalised quaternions of norm 0.5-2
  b  softmax over 24 logits
  c  given weights (SMPLNN), one-hot and blended rows
  d  hierarchical with saturated logits (|x| 20-1000: 1 - s rounds to 0 in fp32)
  e  hierarchical with a general tfs whose rows 3 are not (0, 0, 0, 1)
  f  hierarchical_softmax alone, 1024 rows, with a given dL/dW

Run:  python tests/golden/make_skinning_golden.py
"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _CpuTorch, _exec_nodes, _load_functions, _method  # noqa: E402

RIGID = "models/deformer/rigid.py"
N_A, N_B, N_C, N_D, N_E, N_F = 96, 64, 64, 48, 48, 1024


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _AABB(object):  # only its output's shape matters: lbs_network ignores its input
    def normalize(self, x, sym=False):
        return 2 * x - 1.0 if sym else x


class _Gaussians(object):
    def __init__(self, xyz, rotation):
        self._xyz, self._rotation = xyz, rotation

    @property
    def get_xyz(self):
        return self._xyz

    def clone(self):
        return _Gaussians(self._xyz, self._rotation)

    def set_fwd_transform(self, T):
        self.fwd_transform = T


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
    T = _CpuTorch()
    ns = _load_functions("utils/general_utils.py", ["build_rotation"], dict(torch=T))
    ns.update(_load_functions(RIGID, ["hierarchical_softmax"], dict(torch=T, F=F)))
    scope = dict(torch=T, F=F, build_rotation=ns["build_rotation"], hierarchical_softmax=ns["hierarchical_softmax"])
    fns = {}
    for cls, name in (("SkinningField", "softmax"), ("SkinningField", "get_forward_transform"), ("SkinningField", "forward"),
                      ("SMPLNN", "forward")):
        node, path = _method(RIGID, cls, name)
        fns[(cls, name)] = _exec_nodes([node], path, scope)[name]
    return ns["hierarchical_softmax"], fns


def _rodrigues(aa):
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    k = aa / np.maximum(th, 1e-12)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    K = K - np.swapaxes(K, -1, -2)
    s, c = np.sin(th)[..., None], np.cos(th)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def _smpl_tfs(rng, general=False):
    """24 rigid bone transforms (rotations up to ~1 rad, translations ~0.3), or general 4x4 matrices."""
    tfs = np.zeros((24, 4, 4))
    tfs[:, :3, :3] = _rodrigues(rng.normal(scale=0.5, size=(24, 3)))
    tfs[:, :3, 3] = rng.normal(scale=0.3, size=(24, 3))
    tfs[:, 3, 3] = 1.0
    if general:
        tfs += rng.normal(scale=0.2, size=(24, 4, 4))
    return tfs.astype(np.float32)


def _body(n, rng):
    """Points around a 1.7-unit body: torso, head, limbs."""
    parts = np.array([[0, 1.3, 0, 0.16], [0, 1.62, 0, 0.1], [-0.1, 0.5, 0, 0.07], [0.1, 0.5, 0, 0.07],
                      [-0.5, 1.45, 0, 0.05], [0.5, 1.45, 0, 0.05]])
    k = rng.integers(len(parts), size=n)
    x = parts[k, :3] + parts[k, 3:] * rng.normal(size=(n, 3)) + rng.normal(scale=0.1, size=(n, 3))
    return x.astype(np.float32)


def _quats(n, rng):
    q = rng.normal(size=(n, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))
    return q.astype(np.float32)


def _run_case(ref, kind, w, tfs, xyz, rot, g, G):
    hs, fns = ref
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (w, tfs, xyz, rot)]
            gs = _Gaussians(leaves[2], leaves[3])
            camera = _Obj(bone_transforms=leaves[1])
            if kind == "weights":
                this = _Obj(query_weights=lambda x, W=leaves[0]: W)
                deformed = fns[("SMPLNN", "forward")](this, gs, 0, camera)
            else:
                this = _Obj(distill=False, aabb=_AABB(), lbs_network=lambda x, W=leaves[0]: W)
                this.softmax = lambda logit, t=this: fns[("SkinningField", "softmax")](t, logit)
                this.get_forward_transform = lambda x, tf, t=this: fns[("SkinningField", "get_forward_transform")](t, x, tf)
                deformed = fns[("SkinningField", "forward")](this, gs, 0, camera)
            xb, Rb, T = deformed._xyz, deformed.rotation_precomp, deformed.fwd_transform
            assert xb.dtype == dt and Rb.dtype == dt and T.dtype == dt, (xb.dtype, Rb.dtype, T.dtype)
            loss = (xb * torch.from_numpy(g).to(dt)).sum() + (Rb * torch.from_numpy(G).to(dt)).sum()
            grads = torch.autograd.grad(loss, leaves)
        for name, v in (("xbar", xb), ("Rbar", Rb), ("T", T)) + tuple(zip(("dw", "dtfs", "dxyz", "drot"), grads)):
            out["%s_%s" % (name, tag)] = v.detach().numpy()
    return out


def main():
    ref = _reference()
    rng = np.random.default_rng(2024)
    out = {}

    def case(key, kind, n, w, tfs):
        xyz, rot = _body(n, rng), _quats(n, rng)
        g = rng.normal(size=(n, 3)).astype(np.float32)
        G = rng.normal(size=(n, 3, 3)).astype(np.float32)
        res = _run_case(ref, kind, w, tfs, xyz, rot, g, G)
        out.update({"%s/%s" % (key, k): v for k, v in dict(w=w, tfs=tfs, xyz=xyz, rot=rot, g=g, G=G).items()})
        out["%s/kind" % key] = np.array(kind)
        out.update({"%s/%s" % (key, k): v for k, v in res.items()})

    case("a", "hierarchical", N_A, rng.normal(scale=2.0, size=(N_A, 25)).astype(np.float32), _smpl_tfs(rng))
    case("b", "softmax", N_B, rng.normal(scale=2.0, size=(N_B, 24)).astype(np.float32), _smpl_tfs(rng))
    w = rng.dirichlet(np.full(24, 0.3), size=N_C)
    hot = rng.random(N_C) < 0.5
    w[hot] = np.eye(24)[rng.integers(24, size=int(hot.sum()))]
    case("c", "weights", N_C, w.astype(np.float32), _smpl_tfs(rng))
    x = rng.uniform(20.0, 1000.0, size=(N_D, 25)) * rng.choice([-1.0, 1.0], size=(N_D, 25))
    case("d", "hierarchical", N_D, x.astype(np.float32), _smpl_tfs(rng))
    case("e", "hierarchical", N_E, rng.normal(scale=2.0, size=(N_E, 25)).astype(np.float32), _smpl_tfs(rng, general=True))

    hs = ref[0]
    x = (np.round(rng.normal(scale=3.0, size=(N_F, 25)) * 64) / 64).astype(np.float32)  # (short mantissas: they compress)
    gW = (np.round(rng.normal(size=(N_F, 24)) * 64) / 64).astype(np.float32)
    out["f/x"], out["f/gW"] = x, gW
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            W = hs(xt)
            assert W.dtype == dt
            (dx,) = torch.autograd.grad((W * torch.from_numpy(gW).to(dt)).sum(), [xt])
        out["f/W_%s" % tag], out["f/dx_%s" % tag] = W.detach().numpy(), dx.numpy()

    for k in [k for k in out if k.endswith("_f64")]:
        f32 = out[k[:-4] + "_f32"].astype(np.float64)
        res = (out[k] - f32).astype(np.float32)
        if np.abs(f32 + res - out[k]).max() <= 1e-14 * np.abs(out[k]).max():  # (else kept whole)
            out[k + "res"] = res
            del out[k]
    path = os.path.join(HERE, "skinning.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
