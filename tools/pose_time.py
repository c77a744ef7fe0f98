"""Times the SMPL forward of `pose_correction: direct` at V = 6890, NB = 10 (a seeded synthetic body model of SMPL's
sizes): gsplat_mi355.pose.smpl_pose_forward (csrc/pose.hip) against a torch formulation written for this tool with the
reference's operator sequence: two einsums over the vertices, Rodrigues for 24 joints, the pose blend shapes, a Python
loop of 23 dependent 4x4 products, the blended vertex transforms and posed vertices (the reference computes them every
step although training does not read them), the star-pose transforms from two rotations built on the host and copied to
the device every step, torch.inverse of 24 matrices, the joint normalisation and the pose loss.  Forward alone and
forward + backward (to betas and the four pose rows).  After a warm-up, `--iters` calls are enqueued between two
synchronisations and their mean is one sample; the median of `--runs` samples is reported.

Usage:  python tools/pose_time.py [--iters 50] [--runs 15]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gsplat_mi355 import pose  # noqa: E402

DEV = torch.device("cuda:0")
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
V, NB = 6890, 10


def torch_rodrigues(aa):
    angle = torch.norm(aa + 1e-8, dim=1, keepdim=True)
    n = aa / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = torch.split(n, 1, dim=1)
    zeros = torch.zeros((aa.shape[0], 1), device=aa.device)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    return torch.eye(3, device=aa.device)[None] + sin * K + (1 - cos) * torch.bmm(K, K)


def torch_rigid(R, t):
    return torch.cat([F.pad(R, [0, 0, 0, 1]), F.pad(t, [0, 0, 0, 1], value=1)], dim=2)


def torch_star(J):
    """The A-pose -> star-pose transforms: the z rotations are built on the host and copied over, every call."""
    c = float(np.cos(np.pi / 4))
    T = torch.eye(4, device=J.device).reshape(1, 4, 4).repeat(24, 1, 1)
    for chain, s in (([1, 4, 7, 10], c), ([2, 5, 8, 11], -c)):
        rot = torch.tensor(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), dtype=torch.float32, device=J.device)
        ts = []
        for k, j in enumerate(chain):
            t = J[j]
            if k > 0:
                t = torch.matmul(rot, t - J[chain[k - 1]]) + ts[k - 1]
            ts.append(t)
        ts = torch.stack(ts, dim=0) - torch.matmul(J[chain], rot.transpose(0, 1))
        Rs = F.pad(torch.stack([rot] * 4, dim=0), (0, 0, 0, 1))
        T[chain] = torch.cat([Rs, F.pad(ts, (0, 1), value=1.0).unsqueeze(-1)], dim=-1)
    return T


def torch_pose(m, betas, root_orient, pose_body, pose_hand, trans, rots_gt):
    pose_all = torch.cat([root_orient, pose_body, pose_hand], dim=-1)
    v_shaped = m["v_template"][None] + torch.einsum("bl,mkl->bmk", [betas, m["shapedirs"]])
    J = torch.einsum("bik,ji->bjk", [v_shaped, m["J_regressor"]])
    R = torch_rodrigues(pose_all.view(-1, 3)).view(1, -1, 3, 3)
    feature = (R[:, 1:] - torch.eye(3, device=DEV)).view(1, -1)
    v_posed = torch.matmul(feature, m["posedirs"]).view(1, -1, 3) + v_shaped
    joints = J.unsqueeze(-1)
    rel = joints.clone()
    rel[:, 1:] -= joints[:, PARENTS[1:]]
    mats = torch_rigid(R.view(-1, 3, 3), rel.reshape(-1, 3, 1)).view(-1, 24, 4, 4)
    chain = [mats[:, 0]]
    for i in range(1, 24):
        chain.append(torch.matmul(chain[PARENTS[i]], mats[:, i]))
    G = torch.stack(chain, dim=1)
    init = torch.matmul(G, torch.cat([joints, torch.zeros(1, 24, 1, 1, device=DEV)], dim=2))
    A = G - F.pad(init, [3, 0, 0, 0, 0, 0, 0, 0])
    T = torch.matmul(m["lbs_weights"][None], A.view(1, 24, 16)).view(1, -1, 4, 4)
    homo = torch.cat([v_posed, torch.ones(1, v_posed.shape[1], 1, device=DEV)], dim=2)
    verts = torch.matmul(T, homo.unsqueeze(-1))[:, :, :3, 0] + trans[None]
    rots = torch.cat([torch.eye(3, device=DEV).reshape(1, 1, 3, 3), R[:, 1:]], dim=1).reshape(1, -1, 9).contiguous()
    bone = torch.matmul(A.squeeze(0), torch.inverse(torch_star(J.squeeze(0))))
    bone[:, :3, 3] = bone[:, :3, 3] + trans
    v_shaped = v_shaped.detach()
    center = torch.mean(v_shaped, dim=1)
    centered = v_shaped - center
    cmax, cmin = centered.max(), centered.min()
    Jtrs = J - center
    Jtrs = (Jtrs - cmin + (cmax - cmin) * 0.05) / (cmax - cmin) / 1.1
    Jtrs -= 0.5
    Jtrs *= 2.
    return rots, Jtrs.contiguous(), bone, ((rots_gt - rots) ** 2).mean(), verts


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    m = dict(v_template=rand(V, 3) * torch.tensor([0.3, 0.5, 0.15], device=DEV), shapedirs=0.01 * rand(V, 3, NB),
             J_regressor=torch.softmax(4 * rand(24, V), dim=1), posedirs=0.01 * rand(207, 3 * V),
             lbs_weights=torch.softmax(4 * rand(V, 24), dim=1))
    model = pose.PoseModel(m["v_template"], m["shapedirs"], m["J_regressor"], PARENTS)
    leaves = [(s * rand(1, n)).requires_grad_(True) for n, s in ((NB, 1.0), (3, 0.5), (63, 0.5), (6, 0.5), (3, 0.5))]
    rots_gt = torch_rodrigues(0.5 * rand(24, 3)).reshape(1, 24, 9)
    g = [rand(1, 24, 9), rand(1, 24, 3), rand(24, 4, 4)]
    res = {}
    for impl, fn in (("hip", lambda *a: pose.smpl_pose_forward(model, *a[:5], rots_gt=a[5])), ("torch", lambda *a: torch_pose(m, *a))):
        def fwd():
            with torch.no_grad():
                fn(*leaves, rots_gt)

        def fwd_bwd():
            out = fn(*leaves, rots_gt)
            torch.autograd.grad((out[0] * g[0]).sum() + (out[1] * g[1]).sum() + (out[2] * g[2]).sum() + out[3], leaves)
        res[impl] = (timed(fwd, args.iters, args.runs), timed(fwd_bwd, args.iters, args.runs))
    h, t = res["hip"], res["torch"]
    print("V=%d NB=%d  forward: hip %.4f ms, torch %.4f ms, %.1fx | forward + backward: hip %.4f ms, torch %.4f ms, %.1fx"
          % (V, NB, h[0], t[0], t[0] / h[0], h[1], t[1], t[1] / h[1]), flush=True)


if __name__ == "__main__":
    main()
