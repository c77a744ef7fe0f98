"""Times one densification cycle (densify_and_prune with its Adam-state surgery) at 50k, 200k and 500k Gaussians, SH degree
3, a few per cent cloned, split and pruned: gsplat_mi355.densify (classify + scan + map, one count readback, one apply
launch) against a boolean-mask torch formulation of the same semantics written for this tool (masks, nonzero gathers,
torch.cat, a final masked prune over 18 tensors).  Wall time from the call to a finished stream, median of 15.

Usage:  python tools/densify_time.py [--sizes 50000,200000,500000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

from gsplat_mi355 import densify  # noqa: E402
from gsplat_mi355.optim import FusedAdam  # noqa: E402

GROUPS = densify.GROUPS
DEV = torch.device("cuda:0")
KW = dict(grad_threshold=0.0002, percent_dense=0.01, extent=1.0, min_opacity=0.05, max_screen_size=20)


def make_state(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    params = {"xyz": r(n, 3), "f_dc": r(n, 1, 3), "f_rest": r(n, 15, 3), "opacity": r(n, 1) * 0.9 + 0.5,
              "scaling": r(n, 3) * 0.25 - 4.6, "rotation": r(n, 4)}
    # ~6 % over the gradient threshold (about half clone, half split); ~3 % under the opacity threshold
    accum = torch.exp(r(n, 1) * 0.7 + torch.log(torch.tensor(0.0002 / 3.0)))
    stats = {"xyz_gradient_accum": accum * 3.0, "denom": torch.full((n, 1), 3.0, device=DEV),
             "max_radii2D": torch.zeros(n, device=DEV)}
    moments = {k: (r(*params[k].shape) * 1e-3, r(*params[k].shape).abs() * 1e-6) for k in GROUPS}
    return params, stats, moments


def fused_cycle(params, stats, moments, noise):
    ps = {k: torch.nn.Parameter(v) for k, v in params.items()}
    opt = FusedAdam([{"params": [ps[k]], "lr": 1e-3, "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
    for k in GROUPS:
        opt.state[ps[k]] = {"step": torch.tensor(10.0), "exp_avg": moments[k][0], "exp_avg_sq": moments[k][1]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    new, _ = densify.densify_and_prune(ps, opt, stats, noise=noise, **KW)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, new["xyz"].shape[0]


def _rot(q):
    q = q / torch.sqrt((q * q).sum(1, keepdim=True))
    r, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_cycle(params, stats, moments, noise):
    """The same cycle as boolean-mask torch code: each masked index is a nonzero() with a host sync."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ext = KW["extent"]
    g = stats["xyz_gradient_accum"] / stats["denom"]
    g[g.isnan()] = 0.0
    scale = torch.exp(params["scaling"])
    smax = scale.max(1).values
    sel = g.squeeze(1) >= KW["grad_threshold"]
    clone = sel & (smax <= KW["percent_dense"] * ext)
    split = sel & (smax > KW["percent_dense"] * ext)
    keep = ~split
    std = scale[split].repeat(2, 1)
    z = noise[split].transpose(0, 1).reshape(-1, 3)
    child = {k: v[split].repeat(2, *([1] * (v.dim() - 1))) for k, v in params.items()}
    child["xyz"] = torch.bmm(_rot(params["rotation"][split]).repeat(2, 1, 1), (std * z).unsqueeze(-1)).squeeze(-1) + child["xyz"]
    child["scaling"] = torch.log(std / 1.6)
    cat = {k: torch.cat((v[keep], v[clone], child[k])) for k, v in params.items()}
    n_new = clone.sum() + child["xyz"].shape[0]
    mom = {k: tuple(torch.cat((m[keep], torch.zeros((int(n_new),) + tuple(m.shape[1:]), device=DEV))) for m in moments[k])
           for k in GROUPS}
    prune = (torch.sigmoid(cat["opacity"]) < KW["min_opacity"]).squeeze(1)
    prune |= torch.exp(cat["scaling"]).max(1).values > 0.1 * ext
    live = ~prune
    out = {k: torch.nn.Parameter(v[live]) for k, v in cat.items()}
    out_m = {k: (a[live], b[live]) for k, (a, b) in mom.items()}
    n = out["xyz"].shape[0]
    st = (torch.zeros(n, 1, device=DEV), torch.zeros(n, 1, device=DEV), torch.zeros(n, device=DEV))
    torch.cuda.synchronize()
    del out_m, st
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000,200000,500000")
    args = ap.parse_args()
    for n in (int(s) for s in args.sizes.split(",")):
        params, stats, moments = make_state(n)
        noise = torch.randn(n, 2, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        res = {}
        for name, fn in (("fused", fused_cycle), ("torch", torch_cycle)):
            ts, nn_ = [], None
            for it in range(18):
                t, nn_ = fn(params, stats, moments, noise)
                if it >= 3:
                    ts.append(t)
            ts.sort()
            res[name] = (ts[len(ts) // 2] * 1e3, nn_)
        f = res["fused"][0]
        print("N=%d -> N'=%d (torch %d): fused %.3f ms, torch %.3f ms, %.1fx" % (n, res["fused"][1], res["torch"][1], f,
                                                                                  res["torch"][0], res["torch"][0] / f))


if __name__ == "__main__":
    main()
