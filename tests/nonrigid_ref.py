"""A restatement of csrc/nonrigid.hip's spec (the non-rigid deformer's pose encoder and delta application), written from
the spec in torch and run in float64 on the CPU; gradients by autograd.  tests/test_nonrigid_host.py pins it to the
reference's own fp64 results (tests/golden/nonrigid.npz); the GPU tests compare the kernels with it at the sizes the
fixture does not cover.  `PoseEncoder` is a HierarchicalPoseEncoder-shaped module (the attribute names of the
reference's) whose forward is the restatement in its parameters' dtype."""
import numpy as np
import torch

SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], dtype=np.int32)
SCALE_OFFSETS = ("logit", "exp", "zero")
ROT_OFFSETS = ("add", "mult")
ENC_CASES = ("a", "b", "c", "z", "k")
APPLY_CASES = tuple("%s_%s_F%d" % (s, r, F) for s in SCALE_OFFSETS for r in ROT_OFFSETS for F in (0, 16))
APPLY_OUTS = ("xyz_o", "scal_o", "rot_o", "nr")
APPLY_GRADS = ("ddeltas", "dxyz", "dscaling", "drotation")
APPLY_UPS = ("g_xyz", "g_scal", "g_rot", "g_feat", "g_nr")


def load_fixture(path):
    """tests/golden/nonrigid.npz as a dict, with every "<name>_f64" rebuilt from "<name>_f32" + "<name>_f64res"."""
    d = np.load(path)
    out = {k: d[k] for k in d.files}
    for k in [k for k in out if k.endswith("_f64res")]:
        out[k[:-3]] = out[k[:-7] + "_f32"].astype(np.float64) + out.pop(k).astype(np.float64)
    return out


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---- the pose encoder
def param_shapes(d):
    """The 98 parameter shapes in the packed order: W0, b0, then W1_j, b1_j, W2_j, b2_j for j = 0..23."""
    m = 13 + d
    return [(d, 288), (d,)] + [(m, m), (m,), (d, m), (d,)] * 24


def unpack(packed, d):
    out, off = [], 0
    for s in param_shapes(d):
        n = int(np.prod(s))
        out.append(packed[off:off + n].reshape(s))
        off += n
    assert off == packed.shape[0], (off, packed.shape)
    return out


def pack(params):
    return np.concatenate([np.asarray(p).reshape(-1) for p in params])


def random_params(d, seed):
    """98 fp32 arrays, uniform in +-1/sqrt(fan_in) as nn.Linear draws them, on a grid of 1/1024 (they compress)."""
    rng = np.random.default_rng(seed)
    out, fan_in = [], 1
    for s in param_shapes(d):
        if len(s) == 2:  # (a bias draws with its weight's fan-in)
            fan_in = s[1]
        out.append((np.round(rng.uniform(-1, 1, size=s) / np.sqrt(fan_in) * 1024) / 1024).astype(np.float32))
    return out


def rodrigues(aa):
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    k = aa / np.maximum(th, 1e-12)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    K = K - np.swapaxes(K, -1, -2)
    s, c = np.sin(th)[..., None], np.cos(th)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def random_pose(seed):
    """(rots (1, 24, 9), Jtrs (1, 24, 3)) fp32: rotations of up to ~1 rad, joints in the normalised cube."""
    rng = np.random.default_rng(seed)
    rots = rodrigues(rng.normal(scale=0.5, size=(24, 3))).reshape(1, 24, 9).astype(np.float32)
    Jtrs = rng.uniform(-0.8, 0.8, size=(1, 24, 3)).astype(np.float32)
    return rots, Jtrs


def encoder(params, rots, Jtrs, parents, pre=None):
    """(1, 24 d) from the 98 parameters (torch tensors), rots (1, 24, 9) and Jtrs (1, 24, 3); `pre` collects the 24
    pre-activations."""
    x = torch.cat([rots.reshape(-1), Jtrs.reshape(-1)])
    g = params[0] @ x + params[1]
    out = [None] * 24
    for j in range(24):
        W1, b1, W2, b2 = params[2 + 4 * j:6 + 4 * j]
        Jtr = Jtrs[0, j]
        if j == 0:
            bone, up = torch.linalg.vector_norm(Jtr).reshape(1), g
        else:
            p = int(parents[j])
            bone, up = torch.linalg.vector_norm(Jtr - Jtrs[0, p]).reshape(1), out[p]
        a = W1 @ torch.cat([rots[0, j], Jtr, bone, up]) + b1
        if pre is not None:
            pre.append(a.detach())
        out[j] = W2 @ torch.relu(a) + b2
    return torch.cat(out).reshape(1, -1)


def encoder_forward_backward(packed, d, rots, Jtrs, parents, g):
    """float64 numpy {"out", "drots", "dJtrs", "dparams" (packed), "pre" (24, 13 + d)}."""
    params = [_t(p).requires_grad_(True) for p in unpack(np.asarray(packed), d)]
    r, J = _t(rots).requires_grad_(True), _t(Jtrs).requires_grad_(True)
    pre = []
    out = encoder(params, r, J, parents, pre)
    grads = torch.autograd.grad((out * _t(g)).sum(), [r, J] + params)
    return {"out": out.detach().numpy(), "drots": grads[0].numpy(), "dJtrs": grads[1].numpy(),
            "dparams": pack([x.numpy() for x in grads[2:]]), "pre": torch.stack(pre).numpy()}


class PoseEncoder(torch.nn.Module):
    """HierarchicalPoseEncoder's shape and attribute names; forward = `encoder` above in the parameters' dtype."""

    def __init__(self, dim_per_joint=6, out_dim=-1, rel_joints=False, parents=SMPL_PARENTS, seed=0, dtype=torch.float32):
        super().__init__()
        nn, d = torch.nn, dim_per_joint
        self.num_joints, self.rel_joints, self.ktree_parents = 24, rel_joints, np.asarray(parents, dtype=np.int32)
        self.layer_0 = nn.Linear(288, d)
        self.layers = nn.ModuleList([nn.Sequential(nn.Linear(13 + d, 13 + d), nn.ReLU(), nn.Linear(13 + d, d)) for _ in range(24)])
        self.out_layer = nn.Linear(24 * d, out_dim) if out_dim > 0 else nn.Identity()
        self.n_output_dims = out_dim if out_dim > 0 else 24 * d
        with torch.no_grad():
            for p, v in zip(self.encoder_parameters(), random_params(d, seed)):
                p.copy_(torch.from_numpy(v))
            if out_dim > 0:
                rng = np.random.default_rng(seed + 1)
                self.out_layer.weight.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, size=(out_dim, 24 * d))))
                self.out_layer.bias.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, size=out_dim)))
        self.to(dtype)

    def encoder_parameters(self):
        out = [self.layer_0.weight, self.layer_0.bias]
        for layer in self.layers:
            out += [layer[0].weight, layer[0].bias, layer[2].weight, layer[2].bias]
        return out

    def forward(self, rots, Jtrs, skinning_weight=None):
        return self.out_layer(encoder(self.encoder_parameters(), rots, Jtrs, self.ktree_parents))


# ---- the delta application
def quaternion_multiply(r, s):
    """The Hamilton product, real part first."""
    r0, r1, r2, r3 = r.unbind(-1)
    s0, s1, s2, s3 = s.unbind(-1)
    return torch.stack([r0 * s0 - r1 * s1 - r2 * s2 - r3 * s3, r0 * s1 + r1 * s0 - r2 * s3 + r3 * s2,
                        r0 * s2 + r1 * s3 + r2 * s0 - r3 * s1, r0 * s3 - r1 * s2 + r2 * s1 + r3 * s0], dim=-1)


def apply(deltas, xyz, scaling, rotation, scale_offset, rot_offset):
    """(xyz', scaling', rotation', feature, nr (3)) in the dtype of the inputs; `deltas` is not written."""
    dx, ds, dr = deltas[:, :3], deltas[:, 3:6], deltas[:, 6:10]
    xyz_o = xyz + dx
    if scale_offset == "logit":
        scal_o = scaling + ds
    elif scale_offset == "exp":
        scal_o = torch.log(torch.clamp_min(torch.exp(scaling) + ds, 1e-6))
    else:
        assert scale_offset == "zero"
        ds, scal_o = torch.zeros_like(ds), scaling
    if rot_offset == "add":
        rot_o = rotation + dr
    else:
        assert rot_offset == "mult"
        rot_o = quaternion_multiply(torch.cat([torch.ones_like(dr[:, :1]), dr[:, 1:]], dim=1), rotation)
        dr = dr[:, 1:]
    n = max(deltas.shape[0], 1)
    nr = torch.stack([torch.linalg.vector_norm(dx, dim=1).sum() / n, ds.abs().sum() / n, dr.abs().sum() / n])
    return xyz_o, scal_o, rot_o, deltas[:, 10:], nr


def apply_forward_backward(deltas, xyz, scaling, rotation, scale_offset, rot_offset, g_xyz=None, g_scal=None, g_rot=None,
                           g_feat=None, g_nr=None):
    """float64 numpy {"xyz_o", "scal_o", "rot_o", "feat", "nr", "ddeltas", "dxyz", "dscaling", "drotation"} for the
    upstream gradients given (None = zero; g_nr: three weights of the regularisers)."""
    leaves = [_t(a).requires_grad_(True) for a in (deltas, xyz, scaling, rotation)]
    outs = apply(*leaves, scale_offset, rot_offset)
    res = {k: v.detach().numpy() for k, v in zip(("xyz_o", "scal_o", "rot_o", "feat", "nr"), outs)}
    loss = None
    for o, g in zip(outs, (g_xyz, g_scal, g_rot, g_feat, g_nr)):
        if g is not None and o.numel():
            term = (o * _t(g)).sum()
            loss = term if loss is None else loss + term
    if loss is not None and loss.requires_grad:
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    else:
        grads = [None] * 4
    for name, gr, leaf in zip(APPLY_GRADS, grads, leaves):
        res[name] = (gr if gr is not None else torch.zeros_like(leaf)).numpy()
    return res


def apply_inputs(n, D, seed, scale_offset="logit"):
    """Seeded fp32 inputs and upstream gradients for n rows.  For `exp` the scale offsets keep exp(scaling) + offset at
    0.1 exp(scaling) or more, except every seventh row, where it is negative (the clamp's side)."""
    rng = np.random.default_rng(seed)
    deltas = rng.normal(scale=0.3, size=(n, D)).astype(np.float32)
    scaling = rng.normal(loc=-4.0, scale=0.5, size=(n, 3)).astype(np.float32)
    if scale_offset == "exp":
        u = rng.uniform(-0.8, 2.0, size=(n, 3))
        u[::7] = -rng.uniform(1.5, 3.0, size=u[::7].shape)
        deltas[:, 3:6] = (np.exp(scaling.astype(np.float64)) * u).astype(np.float32)
    q = rng.normal(size=(n, 4))
    rotation = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    ups = dict(g_xyz=rng.normal(size=(n, 3)).astype(np.float32), g_scal=rng.normal(size=(n, 3)).astype(np.float32),
               g_rot=rng.normal(size=(n, 4)).astype(np.float32), g_feat=rng.normal(size=(n, D - 10)).astype(np.float32),
               g_nr=rng.uniform(0.5, 2.0, size=3).astype(np.float32) * n)
    return dict(deltas=deltas, xyz=xyz, scaling=scaling, rotation=rotation), ups
