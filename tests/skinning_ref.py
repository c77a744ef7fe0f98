"""A float64 restatement of csrc/skinning.hip's spec (the rigid deformer's linear blend skinning), written from the spec
in torch on the CPU; gradients by autograd.  tests/test_skinning_host.py pins it to the reference's own fp64 results
(tests/golden/skinning.npz); the GPU tests compare the kernels with it at sizes the fixture does not cover."""
import numpy as np
import torch

KINDS = ("hierarchical", "softmax", "weights")
# (parent, child) splits of the hierarchy before and after step 5; the child's logit is the gate
SPLITS_A = ((1, 4), (2, 5), (3, 6), (4, 7), (5, 8), (6, 9), (7, 10), (8, 11))
SPLITS_B = ((12, 15), (13, 16), (14, 17), (16, 18), (17, 19), (18, 20), (19, 21), (20, 22), (21, 23))


def weights(x, kind):
    """(N, 24) bone weights of the logits / weights x."""
    if kind == "weights":
        return x
    if kind == "softmax":
        return torch.softmax(x, dim=-1)
    s = torch.sigmoid(x)
    p = [None] * 24
    sm = torch.softmax(x[:, 1:4], dim=-1)
    for i in range(3):
        p[1 + i] = s[:, 0] * sm[:, i]
    p[0] = 1 - s[:, 0]

    def split(a, c):
        v = p[a]
        p[c] = v * s[:, c]
        p[a] = v * (1 - s[:, c])

    for a, c in SPLITS_A:
        split(a, c)
    sm = torch.softmax(x[:, 12:15], dim=-1)
    e = p[9] * s[:, 24]
    for i in range(3):
        p[12 + i] = e * sm[:, i]
    p[9] = p[9] * (1 - s[:, 24])
    for a, c in SPLITS_B:
        split(a, c)
    return torch.stack(p, dim=1)


def rotation_matrix(r):
    """build_rotation: q = r / |r| (no epsilon), (w, x, y, z) -> R."""
    q = r / torch.sqrt((r * r).sum(1, keepdim=True))
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def skinning(w, tfs, xyz, rot, kind):
    """(x_bar (N, 3), R_bar (N, 3, 3), T (N, 4, 4)) in the dtype of the inputs."""
    W = weights(w, kind)
    T = (W @ tfs.reshape(24, 16)).reshape(-1, 4, 4)
    x_bar = torch.einsum("nij,nj->ni", T[:, :3, :3], xyz) + T[:, :3, 3]
    R_bar = T[:, :3, :3] @ rotation_matrix(rot)
    return x_bar, R_bar, T


def load_fixture(path):
    """tests/golden/skinning.npz as a dict, with every "<name>_f64" rebuilt from "<name>_f32" + "<name>_f64res"."""
    d = np.load(path)
    out = {k: d[k] for k in d.files}
    for k in [k for k in out if k.endswith("_f64res")]:
        out[k[:-3]] = out[k[:-7] + "_f32"].astype(np.float64) + out.pop(k).astype(np.float64)
    return out


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def forward_backward(w, tfs, xyz, rot, kind, g=None, G=None):
    """float64 numpy results: {"xbar", "Rbar", "T", "dw", "dtfs", "dxyz", "drot"} for upstream gradients g (N, 3) and
    G (N, 3, 3) (None = zero)."""
    leaves = [_t(a).requires_grad_(True) for a in (w, tfs, xyz, rot)]
    xb, Rb, T = skinning(*leaves, kind)
    loss = 0.0
    if g is not None:
        loss = loss + (xb * _t(g)).sum()
    if G is not None:
        loss = loss + (Rb * _t(G)).sum()
    out = {"xbar": xb.detach().numpy(), "Rbar": Rb.detach().numpy(), "T": T.detach().numpy()}
    if g is None and G is None:
        return out
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    for name, gr, leaf in zip(("dw", "dtfs", "dxyz", "drot"), grads, leaves):
        out[name] = (gr if gr is not None else torch.zeros_like(leaf)).numpy()
    return out


def weights_forward_backward(x, kind, gW):
    """float64 (W, dL/dx) of the activation alone for the upstream gradient gW (N, 24)."""
    xt = _t(x).requires_grad_(True)
    W = weights(xt, kind)
    (dx,) = torch.autograd.grad((W * _t(gW)).sum(), [xt])
    return W.detach().numpy(), dx.numpy()
