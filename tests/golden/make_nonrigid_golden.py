"""Generates tests/golden/nonrigid.npz by EXECUTING the reference's own non-rigid deformer code on the CPU (only possible
where the reference tree exists; the tests only read the .npz).

Taken from the syntax trees and executed, nothing else: the class HierarchicalPoseEncoder (models/network_utils.py), the
methods HashGridwithMLP.forward and MLP.forward (models/deformer/non_rigid.py) and quaternion_multiply
(utils/general_utils.py; `tf.quaternion_multiply` is bound to it: pytorch3d computes the same product and is not needed).
Stand-ins: a cfg object with `.get`, an MLP that returns a `deltas` leaf (times one: the reference writes into its
output in place), identity hash grid and pose encoder, minimal Gaussians and aabb.  Each case runs in fp32 (the
reference's precision) and in fp64 (default dtype float64, the same parameter and input values).  Stored: inputs,
outputs and the autograd gradients for seeded upstream gradients; nothing of the reference's text.  An fp64 result is
stored as its float32 residual from the fp32 one (tests/nonrigid_ref.py load_fixture adds them back) when that gives it
back to 1e-14 of its largest magnitude, and whole otherwise.

Encoder cases, keys "<case>/{d,params,rots,Jtrs,g}" and "<case>/{out,drots,dJtrs,dparams}_{f32,f64res}", "<case>/pre_f64"
(the 24 x (13 + d) pre-activations); parameters and their gradients packed W0 | b0 | (W1_j | b1_j | W2_j | b2_j):
  a  d = 1          b  d = 6          c  d = 16
  z  d = 6, joint 7 placed on its parent and the root at the origin (two zero-length bones)
  k  d = 6, every hidden unit of joints 5 and 16 dead (their first biases at -10)
Apply cases "<scale_offset>_<rot_offset>_F<F>", all six mode pairs at F = 0 and 16, N = 40 rows (row 3: a zero offset row;
`exp`: every seventh row on the clamp's side), keys "<case>/{deltas,xyz,scaling,rotation,g_xyz,g_scal,g_rot,g_feat,g_nr}"
and "<case>/{xyz_o,scal_o,rot_o,nr,ddeltas,dxyz,dscaling,drotation}_{f32,f64res}"; both forwards are run and must agree.

The generator asserts what lets the reference alone decide every threshold the same way in both precisions: every ReLU
pre-activation of the fp64 run is further than 1e-4 from 0 (the dead ones below -1); in `exp` cases exp(scaling) + offset
is at least 0.1 exp(scaling) or at most 0.

Run:  python tests/golden/make_nonrigid_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import nonrigid_ref as nr  # noqa: E402
from make_golden import REF, _CpuTorch, _exec_nodes, _load_functions, _method  # noqa: E402
from make_skinning_golden import _Obj, _precision  # noqa: E402

NON_RIGID = "models/deformer/non_rigid.py"
N_APPLY = 40


def _encoder_class():
    path = os.path.join(REF, "models/network_utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HierarchicalPoseEncoder"]
    assert len(node) == 1
    return _exec_nodes(node, path, dict(torch=torch, nn=torch.nn, np=np))["HierarchicalPoseEncoder"]


def _run_encoder(Enc, d, params, rots, Jtrs, g):
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            mod = Enc(dim_per_joint=d)
            assert np.array_equal(mod.ktree_parents, nr.SMPL_PARENTS) and not mod.rel_joints
            own = [mod.layer_0.weight, mod.layer_0.bias]
            for layer in mod.layers:
                own += [layer[0].weight, layer[0].bias, layer[2].weight, layer[2].bias]
            assert len(own) == 98 == len(list(mod.parameters()))
            with torch.no_grad():
                for p, v in zip(own, params):
                    assert p.dtype == dt and tuple(p.shape) == v.shape
                    p.copy_(torch.from_numpy(v).to(dt))
            pre = [None] * 24
            for j, layer in enumerate(mod.layers):
                layer[0].register_forward_hook(lambda m, i, o, j=j: pre.__setitem__(j, o.detach()[0]))
            r = torch.from_numpy(rots).to(dt).requires_grad_(True)
            J = torch.from_numpy(Jtrs).to(dt).requires_grad_(True)
            y = mod(r, J)
            assert y.dtype == dt and tuple(y.shape) == (1, 24 * d)
            grads = torch.autograd.grad((y * torch.from_numpy(g).to(dt)).sum(), [r, J] + own)
        out["out_" + tag], out["drots_" + tag], out["dJtrs_" + tag] = y.detach().numpy(), grads[0].numpy(), grads[1].numpy()
        out["dparams_" + tag] = nr.pack([x.numpy() for x in grads[2:]])
        if tag == "f64":
            out["pre_f64"] = torch.stack(pre).numpy()
    return out


class _Cfg(dict):
    pass  # (`.get` is all the forwards ask of it)


class _Gaussians(object):
    def __init__(self, xyz, scaling, rotation):
        self._xyz, self._scaling, self._rotation = xyz, scaling, rotation

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    def clone(self):
        return _Gaussians(self._xyz, self._scaling, self._rotation)


class _AABB(object):
    def normalize(self, x, sym=False):
        return 2 * x - 1.0 if sym else x


def _apply_forwards():
    T = _CpuTorch()
    qm = _load_functions("utils/general_utils.py", ["quaternion_multiply"], dict(torch=T))["quaternion_multiply"]
    scope = dict(torch=T, tf=_Obj(quaternion_multiply=qm), quaternion_multiply=qm)
    fns = []
    for cls in ("HashGridwithMLP", "MLP"):
        node, path = _method(NON_RIGID, cls, "forward")
        fns.append(_exec_nodes([node], path, scope)["forward"])
    return fns


def _run_apply(fns, so, ro, F, inp, ups):
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        per_fn = []
        for fn in fns:
            with _precision(dt):
                leaves = [torch.from_numpy(inp[k]).to(dt).requires_grad_(True) for k in ("deltas", "xyz", "scaling", "rotation")]
                this = _Obj(cfg=_Cfg(scale_offset=so, rot_offset=ro), delay=0, latent_dim=0, feature_dim=F, aabb=_AABB(),
                            pose_encoder=lambda rots, Jtrs: rots, hashgrid=lambda x: x,
                            mlp=lambda x, cond=None, D=leaves[0]: D * 1.0)
                camera = _Obj(rots=torch.zeros(1, 4, dtype=dt), Jtrs=None, frame_id=0)
                deformed, losses = fn(this, _Gaussians(*leaves[1:]), 10, camera, compute_loss=True)
                outs = [deformed._xyz, deformed._scaling, deformed._rotation,
                        torch.stack([losses["nr_xyz"], losses["nr_scale"], losses["nr_rot"]])]
                assert all(o.dtype == dt for o in outs)
                gs = [torch.from_numpy(ups[k]).to(dt) for k in ("g_xyz", "g_scal", "g_rot", "g_nr")]
                loss = sum((o * g).sum() for o, g in zip(outs, gs))
                if F > 0:
                    feat = deformed.non_rigid_feature
                    assert torch.equal(feat, leaves[0][:, 10:])  # (the in-place write touches column 6 alone)
                    loss = loss + (feat * torch.from_numpy(ups["g_feat"]).to(dt)).sum()
                else:
                    assert not hasattr(deformed, "non_rigid_feature")
                grads = torch.autograd.grad(loss, leaves, allow_unused=True)
                grads = [g if g is not None else torch.zeros_like(l) for g, l in zip(grads, leaves)]
            per_fn.append([o.detach().numpy() for o in outs] + [g.numpy() for g in grads])
        for a, b in zip(*per_fn):
            assert np.array_equal(a, b)
        for name, v in zip(nr.APPLY_OUTS + nr.APPLY_GRADS, per_fn[0]):
            out["%s_%s" % (name, tag)] = v
    return out


def main():
    out = {}
    Enc = _encoder_class()
    for case, d, seed in (("a", 1, 11), ("b", 6, 12), ("c", 16, 13), ("z", 6, 14), ("k", 6, 15)):
        dead = (5, 16) if case == "k" else ()
        g = np.random.default_rng(seed + 200).normal(size=(1, 24 * d)).astype(np.float32)
        while True:  # the first seed whose pre-activations (by the restatement) keep clear of 0; the reference is asserted below
            params = nr.random_params(d, seed)
            rots, Jtrs = nr.random_pose(seed + 100)
            if case == "z":
                Jtrs[0, 7] = Jtrs[0, nr.SMPL_PARENTS[7]]
                Jtrs[0, 0] = 0.0
            for j in dead:
                params[2 + 4 * j + 1][:] = -10.0
            pre = nr.encoder_forward_backward(nr.pack(params), d, rots, Jtrs, nr.SMPL_PARENTS, g)["pre"]
            if np.abs(pre).min() > 2e-4:
                break
            seed += 1000
        res = _run_encoder(Enc, d, params, rots, Jtrs, g)
        pre = res["pre_f64"]
        live = np.delete(pre, dead, axis=0)
        assert np.abs(live).min() > 1e-4, (case, np.abs(live).min())
        assert (live > 0).any(axis=1).all()  # (no joint dead by accident)
        if dead:
            assert pre[list(dead)].max() < -1.0, pre[list(dead)].max()
        out.update({"%s/%s" % (case, k): v for k, v in dict(d=np.array(d), params=nr.pack(params), rots=rots, Jtrs=Jtrs, g=g).items()})
        out.update({"%s/%s" % (case, k): v for k, v in res.items()})
        print("encoder %s: d=%d, smallest live |pre-activation| %.3g" % (case, d, np.abs(live).min()))

    fns = _apply_forwards()
    for k, case in enumerate(nr.APPLY_CASES):
        so, ro, F = case.split("_")
        F = int(F[1:])
        inp, ups = nr.apply_inputs(N_APPLY, 10 + F, seed=300 + k, scale_offset=so)
        inp["deltas"][3, :10] = 0.0
        if so == "exp":
            e = np.exp(inp["scaling"].astype(np.float64))
            arg = e + inp["deltas"][:, 3:6].astype(np.float64)
            assert ((arg >= 0.1 * e) | (arg <= 0)).all() and (arg <= 0).sum() >= 9 and (arg >= 0.1 * e).sum() >= 60
        res = _run_apply(fns, so, ro, F, inp, ups)
        out.update({"%s/%s" % (case, n): v for n, v in list(inp.items()) + list(ups.items()) if v.size})
        out.update({"%s/%s" % (case, n): v for n, v in res.items()})

    for k in [k for k in out if k.endswith("_f64") and not k.endswith("pre_f64")]:
        f32 = out[k[:-4] + "_f32"].astype(np.float64)
        res = (out[k] - f32).astype(np.float32)
        if np.abs(f32 + res - out[k]).max() <= 1e-14 * max(np.abs(out[k]).max(), 1e-300):  # (else kept whole)
            out[k + "res"] = res
            del out[k]
    path = os.path.join(HERE, "nonrigid.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
