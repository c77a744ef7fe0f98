"""A float64 restatement of csrc/skinloss.hip's spec (the rigid deformer's skinning regulariser: surface samples of the
canonical mesh, their blended skinning weights, the box normalisation and the loss), written from the spec in numpy and
torch on the CPU; gradients by autograd.  tests/test_skinning_loss_host.py pins the loss half to the reference's own fp64
results (tests/golden/skinning_loss.npz).  The sampling half cannot be pinned to trimesh or igl (neither is installed
where this suite runs), so `sample` also computes every sample's barycentric coordinates geometrically, from the
sub-triangle areas of the sampled point, and the tests require them to agree with (1 - a - b, a, b).

Two decisions of the spec are made in fp32, exactly as the kernel makes them, because they are discontinuous: the face
pick (pick = u0 * cdf[F-1], one fp32 multiply, searched in the fp32 cdf) and the fold test a + b > 1 (the fp32 sum).
Everything else is float64.  Also here: the small meshes the tests sample."""
import numpy as np
import torch

import skinning_ref

load_fixture = skinning_ref.load_fixture


def face_areas(verts, faces):
    """float64 triangle areas of the fp32 vertices."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((n * n).sum(1))


def sample(verts, faces, cdf, vweights, aabb_min, aabb_max, draws):
    """dict of float64 arrays (face: int64): face, a, b, bary, bary_geo, points, points_norm, target for the fp32 `cdf`
    (the sampler's own) and the fp32 `draws` (n, 3)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    w = np.asarray(vweights, np.float32).astype(np.float64)
    cdf = np.asarray(cdf)
    u = np.asarray(draws)
    assert cdf.dtype == np.float32 and u.dtype == np.float32
    pick = u[:, 0] * cdf[-1]  # fp32 x fp32: one fp32 multiply
    assert pick.dtype == np.float32
    face = np.minimum(np.searchsorted(cdf, pick, side="left"), len(cdf) - 1).astype(np.int64)
    fold = (u[:, 1] + u[:, 2]) > np.float32(1.0)  # the fp32 sum
    a, b = u[:, 1].astype(np.float64), u[:, 2].astype(np.float64)
    a, b = np.where(fold, np.abs(a - 1.0), a), np.where(fold, np.abs(b - 1.0), b)
    v0, v1, v2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    p = v0 + a[:, None] * (v1 - v0) + b[:, None] * (v2 - v0)
    bary = np.stack([1.0 - a - b, a, b], 1)
    # the same coordinates from the point alone: signed sub-triangle areas over the triangle's, along its normal
    nrm = np.cross(v1 - v0, v2 - v0)
    nn = (nrm * nrm).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        geo = np.stack([(np.cross(v1 - p, v2 - p) * nrm).sum(1) / nn, (np.cross(v2 - p, v0 - p) * nrm).sum(1) / nn,
                        (np.cross(v0 - p, v1 - p) * nrm).sum(1) / nn], 1)
    target = (bary[:, :, None] * w[f[face]]).sum(1)
    lo, hi = np.asarray(aabb_min, np.float64), np.asarray(aabb_max, np.float64)
    return dict(face=face, a=a, b=b, bary=bary, bary_geo=geo, points=p, points_norm=2.0 * (p - lo) / (hi - lo) - 1.0,
                target=target)


def loss_torch(logits, target):
    """The loss of (n, 25) or (n, 24) logits against (n, 24) targets, in the dtype of the (torch) inputs."""
    kind = {25: "hierarchical", 24: "softmax"}[int(logits.shape[1])]
    return ((skinning_ref.weights(logits, kind) - target) ** 2).sum(-1).mean()


def loss_and_grad(logits, target, g=1.0):
    """float64 (loss, d(g loss)/dlogits) of the fp32 or fp64 arrays."""
    x = torch.from_numpy(np.asarray(logits, np.float64)).requires_grad_(True)
    loss = loss_torch(x, torch.from_numpy(np.asarray(target, np.float64)))
    (dx,) = torch.autograd.grad(loss * g, [x])
    return float(loss.detach()), dx.numpy()


# ---- meshes (vertices within the unit cube, fp32)
def _weights(rng, V):
    return rng.dirichlet(np.full(24, 0.3), size=V).astype(np.float32)


def triangle(seed=0):
    rng = np.random.default_rng(seed)
    v = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.9]], np.float32)
    return v, np.array([[0, 1, 2]], np.int64), _weights(rng, 3)


def tetrahedron_with_degenerate_face(seed=1):
    """Four faces of a tetrahedron and, in the middle of the list (index 2), a face of zero area (a repeated vertex)."""
    rng = np.random.default_rng(seed)
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 1, 2], [0, 3, 2], [1, 2, 3]], np.int64)
    return v, f, _weights(rng, 4)


def sphere(n_lat=17, n_lon=31, seed=2):
    """A latitude-longitude sphere of diameter 1 centred in the unit cube: 2 n_lon (n_lat - 1) faces (992 by default:
    not a power of two), no degenerate face."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones_like(ph))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * 0.5 + 0.5
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    south = 1 + (n_lat - 1) * n_lon
    f = []
    for j in range(n_lon):
        f.append([0, idx(0, j), idx(0, j + 1)])
        f.append([south, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
        for i in range(n_lat - 2):
            f.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            f.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    return v.astype(np.float32), np.array(f, np.int64), _weights(rng, len(v))


def two_triangles(seed=3):
    """Two separate right triangles with legs (1/4, 1/4) and (1/4, 3/4): areas 1 : 3."""
    rng = np.random.default_rng(seed)
    v = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.25, 0.0], [0.5, 0.0, 0.5], [0.5, 0.75, 0.5], [0.75, 0.0, 0.5]],
                 np.float32)
    return v, np.array([[0, 1, 2], [3, 5, 4]], np.int64), _weights(rng, 6)
