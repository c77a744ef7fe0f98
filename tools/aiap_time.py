"""Times the AIAP regularisers, forward and backward of both losses (positions and covariances sharing one K = 5
neighbour list, as full_aiap_loss runs them every training step) at 50k, 200k and 500k Gaussians: gsplat_mi355.aiap
(one fused autograd node) against a torch formulation of the same losses written for this tool (the reference's cdist
form: gathers, batched cdist, l1_loss, autograd), both excluding and including the knn_points search (the same GPU
K-NN for both).  Wall time from the call to a finished stream, median of 15 after 3 warm-up runs.

Usage:  python tools/aiap_time.py [--sizes 50000,200000,500000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gsplat_mi355 import aiap  # noqa: E402
from gsplat_mi355.knn import knn_points  # noqa: E402

DEV = torch.device("cuda:0")
K = 5


def make_state(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    xyz = r(n, 3)
    cov = r(n, 6) * 1e-3
    return [xyz, xyz + 0.05 * r(n, 3), cov, cov * (1.0 + 0.1 * r(n, 6))]


def torch_aiap(xc, xd, idx):
    dc = torch.cdist(xc.unsqueeze(1), xc[idx])[:, 0, 1:]
    dd = torch.cdist(xd.unsqueeze(1), xd[idx])[:, 0, 1:]
    return F.l1_loss(dc, dd)


def fused_pair(t, idx):
    return aiap._AiapFunction.apply(idx, t[0], t[1], t[2], t[3])


def torch_pair(t, idx):
    return torch_aiap(t[0], t[1], idx), torch_aiap(t[2], t[3], idx)


def step(fn, state, with_knn, idx_fixed):
    t = [x.detach().clone().requires_grad_(True) for x in state]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if with_knn:
        idx = knn_points(t[0].detach()[None], t[0].detach()[None], K=K)[1][0]
    else:
        idx = idx_fixed
    l_xyz, l_cov = fn(t, idx)
    (1.0 * l_xyz + 100.0 * l_cov).backward()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000,200000,500000")
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    for n in (int(s) for s in args.sizes.split(",")):
        state = make_state(n)
        idx = knn_points(state[0][None], state[0][None], K=K)[1][0]
        res = {}
        for name, fn in (("fused", fused_pair), ("torch", torch_pair)):
            for with_knn in (False, True):
                ts = []
                for it in range(3 + args.runs):
                    t = step(fn, state, with_knn, idx)
                    if it >= 3:
                        ts.append(t)
                ts.sort()
                res[(name, with_knn)] = ts[len(ts) // 2] * 1e3
        print("N=%d K=%d  fwd+bwd of both losses: fused %.3f ms, torch %.3f ms, %.1fx | with knn_points: fused %.3f ms, "
              "torch %.3f ms, %.1fx" % (n, K, res[("fused", False)], res[("torch", False)],
                                        res[("torch", False)] / res[("fused", False)], res[("fused", True)],
                                        res[("torch", True)], res[("torch", True)] / res[("fused", True)]), flush=True)


if __name__ == "__main__":
    main()
