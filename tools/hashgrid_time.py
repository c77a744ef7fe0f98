"""Times the hash-grid encoding with the reference's config (16 levels, 2 features, 2^16 rows, base 16, max resolution
2048), forward alone and forward + backward (gradients of the table and of the points), at 50k, 200k and 500k points:
tinycudann.Encoding (gsplat_mi355.hashgrid, csrc/hashgrid.hip) against a torch formulation of the same encoding written
for this tool (corner gathers, autograd; its table gradient is autograd's accumulating scatter, with atomics).  Two clouds: uniform in the
unit box, and scenes.synthetic_cloud(layout="body") normalised by its padded AABB, as AABB.normalize(sym=True) and
HashGrid's (x + 1) / 2 do.  Wall time from the call to a finished stream, median of 15 after 3 warm-up runs.

Usage:  python tools/hashgrid_time.py [--sizes 50000,200000,500000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402
from gsplat_mi355 import hashgrid, scenes  # noqa: E402

DEV = torch.device("cuda:0")
CFG = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 16, "base_resolution": 16,
       "per_level_scale": float(np.exp(np.log(2048 / 16) / 15))}
PRIMES = (1, 2654435761, 805459861)


class TorchHashGrid:
    """The same encoding as torch operators (int64 index arithmetic, masked to 32 bits)."""

    def __init__(self, cfg):
        self.off, self.scale, self.res, _ = hashgrid.levels(hashgrid.parse_config(3, cfg))
        self.F = cfg["n_features_per_level"]

    def __call__(self, x, params):
        th = params.view(-1, self.F)
        outs = []
        M = 0xFFFFFFFF
        for l in range(len(self.scale)):
            size = self.off[l + 1] - self.off[l]
            pos = x * self.scale[l] + 0.5
            fl = torch.floor(pos)
            t = pos - fl
            c = fl.long() & M
            acc = 0
            for k in range(8):
                b = [(k >> d) & 1 for d in range(3)]
                v = [(c[:, d] + b[d]) & M for d in range(3)]
                if self.res[l] ** 3 <= size:
                    idx = (v[0] + v[1] * self.res[l] + v[2] * self.res[l] ** 2) & M
                else:
                    idx = (v[0] * PRIMES[0]) ^ ((v[1] * PRIMES[1]) & M) ^ ((v[2] * PRIMES[2]) & M)
                w = 1
                for d in range(3):
                    w = w * (t[:, d] if b[d] else 1 - t[:, d])
                acc = acc + w[:, None] * th[self.off[l] + idx % size]
            outs.append(acc)
        return torch.cat(outs, 1)


def clouds(n):
    g = torch.Generator().manual_seed(0)
    box = torch.rand(n, 3, generator=g)
    xyz = scenes._body_points(n, torch.Generator().manual_seed(0))  # synthetic_cloud(layout="body")'s positions
    lo, hi = xyz.min(0).values, xyz.max(0).values
    pad = 0.05 * (hi - lo)
    lo, hi = lo - pad, hi + pad
    body = ((xyz - lo) / (hi - lo) * 2 - 1 + 1) * 0.5
    return {"box": box.to(DEV), "body": body.float().to(DEV)}


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
    ap.add_argument("--sizes", default="50000,200000,500000")
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    enc = tcnn.Encoding(3, CFG).to(DEV)
    ref = TorchHashGrid(CFG)
    for n in (int(s) for s in args.sizes.split(",")):
        for name, x0 in clouds(n).items():
            x = x0.clone().requires_grad_(True)
            g = torch.randn(n, 32, device=DEV)
            res = {}
            for impl, fn in (("hip", lambda: enc(x)), ("torch", lambda: ref(x, enc.params))):
                def fwd():
                    with torch.no_grad():
                        fn()

                def fwd_bwd():
                    x.grad = None
                    enc.params.grad = None
                    fn().backward(g)
                res[impl] = (timed(fwd, args.runs), timed(fwd_bwd, args.runs))
            print("N=%d %-4s  forward: hip %.3f ms, torch %.3f ms, %.1fx | forward+backward: hip %.3f ms, torch %.3f ms, "
                  "%.1fx" % (n, name, res["hip"][0], res["torch"][0], res["torch"][0] / res["hip"][0], res["hip"][1],
                             res["torch"][1], res["torch"][1] / res["hip"][1]), flush=True)


if __name__ == "__main__":
    main()
