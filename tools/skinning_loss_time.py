"""Times the rigid deformer's skinning regulariser (SkinningField.get_skinning_loss: n_reg_pts = 1024 surface samples of
the canonical mesh, their blended skinning weights, the skinning MLP, hierarchical_softmax and the summed squared error)
on a synthetic mesh of SMPL's size (V = 6890, F = 13 776): gsplat_mi355.skinning.skinning_loss (csrc/skinloss.hip: sampling
on the device, the loss as one autograd node) against a restatement of the reference's chain written for this tool --
the host sampling in numpy from its definition (the cumulative sum of the face areas, a searchsorted and two random draws
as trimesh's sample_surface does them, the barycentric coordinates of the sampled points from dot products, the gather
and blend of three rows of the weight table per point; trimesh and igl themselves are not installed where this tool was
written), the two host-to-device copies, AABB.normalize, and the torch operator sequence of hierarchical_softmax
(tools/skinning_time.py's) and of mse_loss(., 'none').sum(-1).mean().  Both sides run the same MLP (the fused one).
Forward alone, and forward + backward to the MLP's parameters.  Per call: wall time from the call to a finished stream and
the device time between two events around it; median of 15 [smallest .. largest] after 3 warm-up calls.  No threshold.

Usage:  python tools/skinning_loss_time.py [--n 1024] [--runs 15]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "3dgs-avatar-release_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsplat_mi355 import mlp, skinning  # noqa: E402
from skinning_time import torch_weights  # noqa: E402

DEV = torch.device("cuda:0")
V, F = 6890, 13776


class AABB(object):
    def __init__(self, cmax, cmin):
        self.coord_max, self.coord_min = cmax, cmin

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1.0 if sym else x


class SkinningMLP(torch.nn.Module):
    """What VanillaCondMLP leaves on the module for the skinning network: 3 -> 128 x 4 -> 25, LeakyReLU."""

    def __init__(self):
        super().__init__()
        self.config = dict(multires=0, skip_in=[], cond_in=[], n_neurons=128, n_hidden_layers=4)
        self.num_layers, self.embed_fn = 6, None
        dims = [3, 128, 128, 128, 128, 25]
        for l in range(5):
            setattr(self, "lin%d" % l, torch.nn.Linear(dims[l], dims[l + 1]))
        self.activation = torch.nn.LeakyReLU()

    def forward(self, coords, cond=None):
        return mlp.mlp_forward(self, coords, cond=cond)


def synthetic_mesh(rng):
    """A closed strip of triangles over V body-sized random vertices, F faces, Dirichlet skinning weights."""
    verts = (rng.normal(size=(V, 3)) * np.array([0.35, 0.55, 0.12])).astype(np.float32)
    k = np.arange(F)
    faces = np.stack([k % V, (k + 1) % V, (k + 2 + k // V) % V], 1).astype(np.int64)
    weights = rng.dirichlet(np.full(24, 0.1), size=V).astype(np.float32)
    return verts, faces, weights


class HostChain(object):
    """The reference's chain, restated: the sampling on the host, two copies, torch operators on the device."""

    def __init__(self, field, seed):
        self.field, self.rng = field, np.random.default_rng(seed)
        v, f = field.smpl_verts, field.faces
        self.origins, self.vectors = v[f[:, 0]], np.stack([v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]], 1)
        self.areas = 0.5 * np.linalg.norm(np.cross(self.vectors[:, 0].astype(np.float64), self.vectors[:, 1]), axis=1)

    def sample(self, n):
        field = self.field
        cum = np.cumsum(self.areas)
        face_idx = np.searchsorted(cum, self.rng.random(n) * cum[-1])
        lengths = self.rng.random((n, 2, 1))
        fold = lengths.sum(axis=1).reshape(-1) > 1.0
        lengths[fold] -= 1.0
        lengths = np.abs(lengths)
        points = ((self.vectors[face_idx] * lengths).sum(axis=1) + self.origins[face_idx]).astype(np.float32)
        ids = field.faces[face_idx]
        a, b, c = field.smpl_verts[ids[:, 0]], field.smpl_verts[ids[:, 1]], field.smpl_verts[ids[:, 2]]
        v0, v1, v2 = b - a, c - a, points - a  # barycentric coordinates of the points, from dot products
        d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
        d20, d21 = (v2 * v0).sum(1), (v2 * v1).sum(1)
        den = d00 * d11 - d01 * d01
        bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        bary = np.stack([1.0 - bv - bw, bv, bw], 1)
        pts_W = (field.skinning_weights[ids] * bary[..., None]).sum(axis=1).astype(np.float32)
        return torch.from_numpy(points).cuda(), torch.from_numpy(pts_W).cuda()

    def loss(self):
        field = self.field
        pts, sampled = self.sample(field.cfg.n_reg_pts)
        pred = torch_weights(field.lbs_network(field.aabb.normalize(pts, sym=True)))
        return torch.nn.functional.mse_loss(pred, sampled, reduction="none").sum(-1).mean()


def timed(fn, runs):
    """((median, min, max) wall ms, (median, min, max) device ms) per call."""
    wall, device = [], []
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(3 + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        if it >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
            device.append(start.elapsed_time(stop))
    stats = lambda s: (sorted(s)[len(s) // 2], min(s), max(s))
    return stats(wall), stats(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    field = type("Field", (), {})()
    field.smpl_verts, field.faces, field.skinning_weights = synthetic_mesh(rng)
    lo, hi = field.smpl_verts.min(0) - 0.05, field.smpl_verts.max(0) + 0.05
    field.aabb = AABB(torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV))
    field.lbs_network, field.distill = SkinningMLP().to(DEV), False
    field.cfg = type("Cfg", (), {"n_reg_pts": args.n})()
    params = list(field.lbs_network.parameters())
    host = HostChain(field, seed=1)
    with torch.no_grad():
        print("n=%d V=%d F=%d: loss fused %.6f, host chain %.6f (other samples of the same surface)"
              % (args.n, V, F, float(skinning.skinning_loss(field)), float(host.loss())), flush=True)
    fmt = lambda s: "%.3f [%.3f .. %.3f]" % s
    for name, loss in (("fused", lambda: skinning.skinning_loss(field)), ("host chain", host.loss)):
        def fwd():
            with torch.no_grad():
                loss()

        def fwd_bwd():
            torch.autograd.grad(loss(), params)

        for what, fn in (("forward", fwd), ("forward + backward", fwd_bwd)):
            wall, device = timed(fn, args.runs)
            print("%-10s %-18s wall %s ms, device %s ms" % (name, what, fmt(wall), fmt(device)), flush=True)


if __name__ == "__main__":
    main()
