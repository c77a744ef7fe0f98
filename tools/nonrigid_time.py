"""Times the two fused parts of the non-rigid deformer: gsplat_mi355.nonrigid (csrc/nonrigid.hip) against torch
formulations written for this tool with the reference's operator sequences.
  * the pose encoder at dim_per_joint = 6: one nn.Linear over the 288 inputs, then per joint in a Python loop a norm, a
    cat, Linear -> ReLU -> Linear, each joint waiting for its parent's output, and a final cat;
  * the delta application at 200k rows and F = 0, 16, 64 (`logit` scales, `mult` rotations): four slices of the MLP's
    output, the in-place 1 in column 6, the quaternion product from unbound columns and a stack, three norm-and-mean
    regularisers; backward through autograd (every slice materialises a zero (N, 10 + F) tensor).
Forward alone (no_grad) and forward + backward.  After a warm-up, `--iters` calls are enqueued between two
synchronisations and their mean is one sample; the median of `--runs` samples is reported.

Usage:  python tools/nonrigid_time.py [--iters 50] [--runs 15] [--rows 200000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

from gsplat_mi355 import nonrigid  # noqa: E402

DEV = torch.device("cuda:0")
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


class TorchEncoder(torch.nn.Module):
    def __init__(self, d=6):
        super().__init__()
        nn = torch.nn
        self.num_joints, self.rel_joints, self.ktree_parents = 24, False, PARENTS
        self.layer_0 = nn.Linear(288, d)
        self.layers = nn.ModuleList([nn.Sequential(nn.Linear(13 + d, 13 + d), nn.ReLU(), nn.Linear(13 + d, d)) for _ in range(24)])
        self.out_layer = nn.Identity()

    def forward(self, rots, Jtrs):
        b = rots.size(0)
        feat = self.layer_0(torch.cat([rots.view(b, -1), Jtrs.view(b, -1)], dim=-1))
        out = [None] * 24
        for j in range(24):
            rot, Jtr, p = rots[:, j, :], Jtrs[:, j, :], PARENTS[j]
            if p < 0:
                x = torch.cat([rot, Jtr, torch.norm(Jtr, dim=-1, keepdim=True), feat], dim=-1)
            else:
                x = torch.cat([rot, Jtr, torch.norm(Jtr - Jtrs[:, p, :], dim=-1, keepdim=True), out[p]], dim=-1)
            out[j] = self.layers[j](x)
        return self.out_layer(torch.cat(out, dim=-1))


def torch_apply(mlp_out, xyz, scaling, rotation):
    deltas = mlp_out * 1.0  # (the MLP's output is not a leaf: the chain writes into it)
    d_xyz, d_scale, d_rot = deltas[:, :3], deltas[:, 3:6], deltas[:, 6:10]
    feature = deltas[:, 10:]
    xyz_o = xyz + d_xyz
    scal_o = scaling + d_scale
    q1 = d_rot
    q1[:, 0] = 1.
    d_rot = d_rot[:, 1:]
    r0, r1, r2, r3 = q1.unbind(-1)
    s0, s1, s2, s3 = rotation.unbind(-1)
    rot_o = torch.stack([r0 * s0 - r1 * s1 - r2 * s2 - r3 * s3, r0 * s1 + r1 * s0 - r2 * s3 + r3 * s2,
                         r0 * s2 + r1 * s3 + r2 * s0 - r3 * s1, r0 * s3 - r1 * s2 + r2 * s1 + r3 * s0], dim=-1)
    losses = (torch.norm(d_xyz, p=2, dim=1).mean(), torch.norm(d_scale, p=1, dim=1).mean(), torch.norm(d_rot, p=1, dim=1).mean())
    return xyz_o, scal_o, rot_o, feature, losses


def timed(fn, iters, runs):
    for _ in range(5):
        fn()
    samples = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) / iters)
    samples.sort()
    return samples[len(samples) // 2] * 1e3


def report(what, res):
    h, t = res["hip"], res["torch"]
    print("%s  forward: hip %.4f ms, torch %.4f ms, %.1fx | forward + backward: hip %.4f ms, torch %.4f ms, %.1fx"
          % (what, h[0], t[0], t[0] / h[0], h[1], t[1], t[1] / h[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--rows", type=int, default=200000)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)

    torch.manual_seed(0)
    enc = TorchEncoder(6).to(DEV)
    rots, Jtrs = rand(1, 24, 9).requires_grad_(True), rand(1, 24, 3).requires_grad_(True)
    g = rand(1, 144)
    leaves = [rots, Jtrs] + list(enc.parameters())
    res = {}
    for impl, fn in (("hip", lambda: nonrigid.pose_encode(enc, rots, Jtrs)), ("torch", lambda: enc(rots, Jtrs))):
        def fwd():
            with torch.no_grad():
                fn()

        def fwd_bwd():
            torch.autograd.grad((fn() * g).sum(), leaves)
        res[impl] = (timed(fwd, args.iters, args.runs), timed(fwd_bwd, args.iters, args.runs))
    report("pose encoder d=6", res)

    n = args.rows
    for F in (0, 16, 64):
        deltas = (0.1 * rand(n, 10 + F)).requires_grad_(True)
        xyz, scaling, rotation = rand(n, 3).requires_grad_(True), rand(n, 3).requires_grad_(True), rand(n, 4).requires_grad_(True)
        gx, gs, gr, gf = rand(n, 3), rand(n, 3), rand(n, 4), rand(n, F)
        leaves = [deltas, xyz, scaling, rotation]
        hip = lambda: nonrigid.nonrigid_apply(deltas, xyz, scaling, rotation, scale_offset="logit", rot_offset="mult")
        res = {}
        for impl, fn in (("hip", lambda: (lambda o: o[:4] + (tuple(o[4][k] for k in ("nr_xyz", "nr_scale", "nr_rot")),))(hip())),
                         ("torch", lambda: torch_apply(deltas, xyz, scaling, rotation))):
            def fwd():
                with torch.no_grad():
                    fn()

            def fwd_bwd():
                x, s, q, feat, losses = fn()
                total = (x * gx).sum() + (s * gs).sum() + (q * gr).sum() + losses[0] + losses[1] + losses[2]
                if F:
                    total = total + (feat * gf).sum()
                torch.autograd.grad(total, leaves)
            res[impl] = (timed(fwd, args.iters, args.runs), timed(fwd_bwd, args.iters, args.runs))
        report("apply N=%d F=%d logit/mult" % (n, F), res)


if __name__ == "__main__":
    main()
