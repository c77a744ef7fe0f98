"""Times the rigid deformer's skinning (hierarchical weights from 25 logits, blend of the 24 bone transforms, positions
and rotation matrices) at 1024, 50k, 200k and 500k Gaussians: gsplat_mi355.skinning.linear_blend_skinning
(csrc/skinning.hip) against a torch formulation written for this tool with the reference's operator sequence (sigmoid,
indexed-assignment hierarchy, a GEMM for T_fwd, homogeneous bmm, build_rotation by element assignment, bmm).  Forward
alone, and forward + backward with and without a gradient to the bone transforms (the learnable ones of pose_correction:
direct).  Wall time from the call to a finished stream, median of 15 after 3 warm-up runs.

Usage:  python tools/skinning_time.py [--sizes 1024,50000,200000,500000] [--runs 15]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gsplat_mi355 import skinning  # noqa: E402

DEV = torch.device("cuda:0")
STEPS = ((None, [1, 2, 3], 0), ([1, 2, 3], [4, 5, 6], 4), ([4, 5, 6], [7, 8, 9], 7), ([7, 8], [10, 11], 10), None,
         ([12], [15], 15), ([13, 14], [16, 17], 16), ([16, 17], [18, 19], 18), ([18, 19], [20, 21], 20),
         ([20, 21], [22, 23], 22))


def torch_weights(x):
    """The kinematic-tree softmax with one indexed assignment per statement, as a training loop runs it in torch."""
    s = torch.sigmoid(x)
    p = torch.ones(x.shape[0], 24, device=x.device)
    p[:, [1, 2, 3]] = s[:, [0]] * F.softmax(x[:, [1, 2, 3]], dim=-1)
    p[:, [0]] = 1 - s[:, [0]]
    for k, step in enumerate(STEPS[1:], start=1):
        if step is None:  # step 5
            p[:, [12, 13, 14]] = p[:, [9]] * s[:, [24]] * F.softmax(x[:, [12, 13, 14]], dim=-1)
            p[:, [9]] = p[:, [9]] * (1 - s[:, [24]])
            continue
        par, ch, g0 = step
        gate = list(range(g0, g0 + len(ch)))
        p[:, ch] = p[:, par] * s[:, gate]
        p[:, par] = p[:, par] * (1 - s[:, gate])
    return p


def torch_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def torch_skinning(logits, tfs, xyz, rot):
    n = xyz.shape[0]
    T = torch.matmul(torch_weights(logits), tfs.view(-1, 16)).view(-1, 4, 4)
    homo = torch.cat([xyz, torch.ones(n, 1, device=xyz.device)], dim=-1).view(n, 4, 1)
    x_bar = torch.matmul(T, homo)[:, :3, 0]
    R_bar = torch.matmul(T[:, :3, :3], torch_rotation(rot))
    return x_bar, R_bar, T.detach()


def timed(fn, runs):
    ts = []
    for it in range(3 + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= 3:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,50000,200000,500000")
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    for n in (int(s) for s in args.sizes.split(",")):
        logits = (2 * torch.randn(n, 25, device=DEV, generator=gen)).requires_grad_(True)
        tfs = (torch.eye(4, device=DEV) + 0.2 * torch.randn(24, 4, 4, device=DEV, generator=gen)).requires_grad_(True)
        xyz = torch.randn(n, 3, device=DEV, generator=gen).requires_grad_(True)
        rot = torch.randn(n, 4, device=DEV, generator=gen).requires_grad_(True)
        g, G = torch.randn(n, 3, device=DEV, generator=gen), torch.randn(n, 3, 3, device=DEV, generator=gen)
        res = {}
        for impl, fn in (("hip", skinning.linear_blend_skinning), ("torch", torch_skinning)):
            def fwd():
                with torch.no_grad():
                    fn(logits, tfs, xyz, rot)

            def fwd_bwd(with_tfs):
                tfs.requires_grad_(with_tfs)
                xb, Rb, _ = fn(logits, tfs, xyz, rot)
                torch.autograd.grad((xb * g).sum() + (Rb * G).sum(), [logits, xyz, rot] + ([tfs] if with_tfs else []))
            res[impl] = (timed(fwd, args.runs), timed(lambda: fwd_bwd(True), args.runs), timed(lambda: fwd_bwd(False), args.runs))
        h, t = res["hip"], res["torch"]
        print("N=%d  forward: hip %.3f ms, torch %.3f ms, %.1fx | fwd+bwd (dtfs): hip %.3f ms, torch %.3f ms, %.1fx | "
              "fwd+bwd (no dtfs): hip %.3f ms, torch %.3f ms, %.1fx"
              % (n, h[0], t[0], t[0] / h[0], h[1], t[1], t[1] / h[1], h[2], t[2], t[2] / h[2]), flush=True)


if __name__ == "__main__":
    main()
