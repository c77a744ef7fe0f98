"""Generates tests/golden/texture.npz by EXECUTING the reference's own texture-input code on the CPU (only possible where
the reference tree exists; the tests only read the .npz).

Taken from the syntax trees and executed, nothing else: the method ColorMLP.compose_input (models/texture/texture.py) and
the function eval_sh_bases with the constants C0..C4 (utils/sh_utils.py).  Stand-ins: a cfg object with `.get`, minimal
Gaussians (get_features is the reference's cat of _features_dc and _features_rest), an aabb that normalises as
utils/dataset_utils.py's does, an nn.Embedding, a camera, and an `augm_rots` that returns the case's stored matrix (the
reference transposes it and multiplies from the right).  Each case runs in fp32 (the reference's precision) and in fp64
(default dtype float64, the same parameter and input values).  Stored per case "<case>/": the inputs (texture_ref.INPUTS,
`latent_row` = the embedding row the frame selects, `noise` already transposed), `inp_{f32,f64res}` and the autograd
gradients of every leaf (texture_ref.GRADS) for the seeded upstream gradient `g`; nothing of the reference's text.  An
fp64 result is stored as its float32 residual from the fp32 one (tests/texture_ref.py load_fixture adds them back) when
that gives it back to 1e-14 of its largest magnitude, and whole otherwise.

Cases (texture_ref.CASES), N = 40 rows, points in [-1, 1]^3, the camera 0.3 or 3 from the origin: degrees 1, 3 and 4 at
the default widths 32 / 16 / 16; degree 3 without cano_view_dir; degree 3 with use_xyz; degree 0 with latent_dim 0; a
frame the module does not know (the last latent row).

The generator asserts, for every stored result, that the reference's own fp32 value lies within 1e-6 of the tensor's
largest magnitude of its fp64 value: a tenth of the bar the GPU tests hold the kernels to.

Run:  python tests/golden/make_texture_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import texture_ref as tr  # noqa: E402
from make_golden import REF, _CpuTorch, _exec_nodes, _method  # noqa: E402
from make_skinning_golden import _Obj, _precision  # noqa: E402

N = 40
FRAME_IDS = (10, 11, 12, 13, 14)
REF_BAR = 1e-6


class _Torch64(_CpuTorch):
    """In the fp64 run the reference's `torch.tensor(.., dtype=torch.float32)` of the noise matrix gives float64."""

    def tensor(self, *a, **kw):
        if kw.get("dtype") == torch.float32:
            kw = dict(kw, dtype=torch.float64)
        return _CpuTorch.tensor(self, *a, **kw)


def _sh_bases(T):
    path = os.path.join(REF, "utils/sh_utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body
            if (isinstance(n, ast.Assign) and all(isinstance(t, ast.Name) and t.id in ("C0", "C1", "C2", "C3", "C4") for t in n.targets))
            or (isinstance(n, ast.FunctionDef) and n.name == "eval_sh_bases")]
    assert len(keep) == 6, [getattr(n, "name", None) for n in keep]
    return _exec_nodes(keep, path, dict(torch=T, np=np))["eval_sh_bases"]


class _Cfg(dict):
    pass  # (`.get` is all compose_input asks of it)


class _AABB(object):  # utils/dataset_utils.py AABB.normalize
    def __init__(self, lo, hi):
        self.coord_min, self.coord_max = lo, hi

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1. if sym else x


class _Gaussians(object):
    def __init__(self, dc, rest, xyz, T_fwd, feature):
        self._features_dc, self._features_rest, self._xyz, self.fwd_transform, self.non_rigid_feature = dc, rest, xyz, T_fwd, feature

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):  # scene/gaussian_model.py:145-148
        return torch.cat((self._features_dc, self._features_rest), dim=1)


def _inputs(case, seed):
    c = tr.CASES[case]
    r = tr.random_inputs(N, (1, tr.FEATURE_DIM - 1), (tr.NON_RIGID_DIM,), 0, seed, dist=c["dist"])
    rng = np.random.default_rng(seed + 1)
    D = tr.FEATURE_DIM + 3 * c["use_xyz"] + tr.n_sh(c["sh_degree"]) + tr.NON_RIGID_DIM + c["latent_dim"]
    frame = FRAME_IDS[2] if c["known_frame"] else 999
    return dict(features_dc=r["before"][0].reshape(N, 1, 1), features_rest=r["before"][1].reshape(N, tr.FEATURE_DIM - 1, 1),
                xyz=r["xyz"], campos=r["campos"], T_fwd=r["fwd_transform"], noise=r["noise"], non_rigid_feature=r["after"][0],
                latent_weight=rng.normal(size=(len(FRAME_IDS), max(c["latent_dim"], 1))).astype(np.float32),
                aabb=np.array([[-1.25, -1.5, -1.125], [1.5, 1.25, 1.75]], dtype=np.float32),
                g=rng.normal(size=(N, D)).astype(np.float32), frame_id=np.array(frame),
                latent_row=np.array(FRAME_IDS.index(frame) if c["known_frame"] else len(FRAME_IDS) - 1))


def _run(case, inp):
    c = tr.CASES[case]
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            T = _CpuTorch() if dt == torch.float32 else _Torch64()
            bases = _sh_bases(T)
            node, path = _method("models/texture/texture.py", "ColorMLP", "compose_input")
            # the stored matrix is the transposed one: the stand-in hands its transpose to the reference's .transpose(0, 1)
            augm = lambda *a: inp["noise"].astype(np.float64).T
            compose = _exec_nodes([node], path, dict(torch=T, augm_rots=augm))["compose_input"]
            t = lambda k: torch.from_numpy(inp[k]).to(dt)
            leaves = [t(k).requires_grad_(True) for k in ("features_dc", "features_rest", "xyz", "non_rigid_feature")]
            latent = torch.nn.Embedding(len(FRAME_IDS), max(c["latent_dim"], 1))
            with torch.no_grad():
                latent.weight.copy_(t("latent_weight"))
            assert latent.weight.dtype == dt
            deg = c["sh_degree"]
            this = _Obj(cfg=_Cfg(view_noise=45.0), metadata={"aabb": _AABB(t("aabb")[0], t("aabb")[1])}, use_xyz=bool(c["use_xyz"]),
                        use_cov=False, use_normal=False, sh_degree=deg, cano_view_dir=bool(c["cano"]), non_rigid_dim=tr.NON_RIGID_DIM,
                        latent_dim=c["latent_dim"], frame_dict={f: k for k, f in enumerate(FRAME_IDS)}, latent=latent,
                        training=bool(c["train"]), sh_embed=lambda d: bases(deg, d)[..., 1:])
            gs = _Gaussians(leaves[0], leaves[1], leaves[2], t("T_fwd"), leaves[3])
            camera = _Obj(camera_center=t("campos"), frame_id=int(inp["frame_id"]))
            y = compose(this, gs, camera)
            assert y.dtype == dt and tuple(y.shape) == inp["g"].shape, (y.dtype, y.shape)
            grads = torch.autograd.grad((y * t("g")).sum(), leaves + [latent.weight], allow_unused=True)
            grads = [g if g is not None else torch.zeros_like(l) for g, l in zip(grads, leaves + [latent.weight])]
        out["inp_" + tag] = y.detach().numpy()
        for name, g in zip(tr.GRADS, grads):
            out["%s_%s" % (name, tag)] = g.numpy()
    return out


def main():
    out = {}
    for k, case in enumerate(tr.CASES):
        inp = _inputs(case, 700 + k)
        res = _run(case, inp)
        worst = 0.0
        for name in ("inp",) + tr.GRADS:
            f32, f64 = res[name + "_f32"].astype(np.float64), res[name + "_f64"]
            scale = np.abs(f64).max()
            err = np.abs(f32 - f64).max() / scale if scale else np.abs(f32).max()
            assert err <= REF_BAR, (case, name, err)
            worst = max(worst, err)
        print("%s: D=%d, the reference's fp32 within %.3g of its fp64" % (case, inp["g"].shape[1], worst))
        out.update({"%s/%s" % (case, n): v for n, v in inp.items()})
        out.update({"%s/%s" % (case, n): v for n, v in res.items()})
    for k in [k for k in out if k.endswith("_f64")]:
        f32 = out[k[:-4] + "_f32"].astype(np.float64)
        res = (out[k] - f32).astype(np.float32)
        if np.abs(f32 + res - out[k]).max() <= 1e-14 * max(np.abs(out[k]).max(), 1e-300):  # (else kept whole)
            out[k + "res"] = res
            del out[k]
    path = os.path.join(HERE, "texture.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
