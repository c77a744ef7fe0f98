"""Times the fused input of the ColorMLP texture: gsplat_mi355.texture.color_mlp_input (csrc/texture.hip) against a torch
formulation written for this tool with the reference's operator sequence, at the default config's widths (32 features,
the 15 bases of degree 3, 16 non-rigid features, 16 latent values: D = 79), canonical view direction and view noise on:
  a cat of the two feature tensors and a squeeze; the camera centre repeated; the batched 3x3 product with the transposed
  rotations; the noise matrix built on the host and copied to the device, and its product; a norm and a division; the
  bases as an empty (N, 16) tensor filled by one indexed assignment per basis, sliced; three cats, each of the whole
  matrix so far; the latent row looked up through an index built on the host and copied to the device, expanded.
The fused call gets its noise matrix by value and its latent row through a cached device index, as texture_forward does.
Forward alone (no_grad) and forward + backward through (inp * g).sum().  After a warm-up, `--iters` calls are enqueued
between two synchronisations and their mean is one sample; the median of `--runs` samples is reported.

Usage:  python tools/texture_time.py [--iters 50] [--runs 15] [--rows 50000 200000]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsplat_mi355 import texture  # noqa: E402

DEV = torch.device("cuda:0")
PI = math.pi
K0, K1 = math.sqrt(1 / (4 * PI)), math.sqrt(3 / (4 * PI))
K2 = [math.sqrt(15 / (4 * PI)) * c for c in (1, -1, 1 / (2 * math.sqrt(3)), -1, 0.5)]
K3 = [-math.sqrt(35 / (32 * PI)), math.sqrt(105 / (4 * PI)), -math.sqrt(21 / (32 * PI)), math.sqrt(7 / (16 * PI)),
      -math.sqrt(21 / (32 * PI)), math.sqrt(105 / (16 * PI)), -math.sqrt(35 / (32 * PI))]


def torch_bases3(dirs):
    """The 16 bases of degree 3: an empty tensor and one indexed assignment per basis."""
    out = torch.empty((*dirs.shape[:-1], 16), dtype=dirs.dtype, device=dirs.device)
    out[..., 0] = K0
    x, y, z = dirs.unbind(-1)
    out[..., 1] = -K1 * y
    out[..., 2] = K1 * z
    out[..., 3] = -K1 * x
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    out[..., 4] = K2[0] * xy
    out[..., 5] = K2[1] * yz
    out[..., 6] = K2[2] * (2.0 * zz - xx - yy)
    out[..., 7] = K2[3] * xz
    out[..., 8] = K2[4] * (xx - yy)
    out[..., 9] = K3[0] * y * (3 * xx - yy)
    out[..., 10] = K3[1] * xy * z
    out[..., 11] = K3[2] * y * (4 * zz - xx - yy)
    out[..., 12] = K3[3] * z * (2 * zz - 3 * xx - 3 * yy)
    out[..., 13] = K3[4] * x * (4 * zz - xx - yy)
    out[..., 14] = K3[5] * z * (xx - yy)
    out[..., 15] = K3[6] * x * (xx - 3 * yy)
    return out


def torch_compose(dc, rest, xyz, campos, T_fwd, noise_host, feature, latent, row):
    features = torch.cat((dc, rest), dim=1).squeeze(-1)
    n = features.shape[0]
    d = xyz - campos.repeat(n, 1)
    R_bwd = T_fwd[:, :3, :3].transpose(1, 2)
    d = torch.matmul(R_bwd, d.unsqueeze(-1)).squeeze(-1)
    noise = torch.tensor(noise_host, dtype=torch.float32, device=d.device).transpose(0, 1)
    d = torch.matmul(d, noise)
    unit = d / (d.norm(dim=1, keepdim=True) + 1e-12)
    features = torch.cat([features, torch_bases3(unit)[..., 1:]], dim=1)
    features = torch.cat([features, feature], dim=1)
    idx = torch.Tensor([row]).long().to(features.device)
    code = latent(idx).expand(features.shape[0], -1)
    return torch.cat([features, code], dim=1)


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
    ap.add_argument("--rows", type=int, nargs="+", default=[50000, 200000])
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    rng = np.random.default_rng(0)
    a = rng.normal(scale=0.5, size=3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    noise_host = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)  # as augm_rots returns it: float64, on the host
    noise_t = torch.as_tensor(noise_host, dtype=torch.float32).transpose(0, 1)
    torch.manual_seed(0)
    latent = torch.nn.Embedding(8, 16).to(DEV)
    rows = torch.arange(8, dtype=torch.long, device=DEV)
    campos = torch.tensor([0.5, -1.0, 2.5], device=DEV)
    for n in args.rows:
        dc, rest = rand(n, 1, 1).requires_grad_(True), rand(n, 31, 1).requires_grad_(True)
        xyz, feature = rand(n, 3).requires_grad_(True), rand(n, 16).requires_grad_(True)
        q = torch.nn.functional.normalize(rand(n, 4), dim=1)
        r, x, y, z = q.unbind(1)
        T_fwd = torch.zeros(n, 4, 4, device=DEV)
        T_fwd[:, :3, :3] = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                                        1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                                        1 - 2 * (x * x + y * y)], dim=1).reshape(n, 3, 3)
        T_fwd[:, :3, 3], T_fwd[:, 3, 3] = rand(n, 3), 1.0
        g = rand(n, 79)
        leaves = [dc, rest, xyz, feature, latent.weight]
        impls = (("hip", lambda: texture.color_mlp_input([dc, rest], xyz, campos, 3, fwd_transform=T_fwd, view_noise=noise_t,
                                                         after=[feature], latent=latent(rows[3:4]))),
                 ("torch", lambda: torch_compose(dc, rest, xyz, campos, T_fwd, noise_host, feature, latent, 3)))
        with torch.no_grad():
            a, b = impls[0][1](), impls[1][1]()
            print("N=%d: largest difference between the two inputs %.3g" % (n, float((a - b).abs().max())), flush=True)
        res = {}
        for impl, fn in impls:
            def fwd():
                with torch.no_grad():
                    fn()

            def fwd_bwd():
                torch.autograd.grad((fn() * g).sum(), leaves)
            res[impl] = (timed(fwd, args.iters, args.runs), timed(fwd_bwd, args.iters, args.runs))
        h, t = res["hip"], res["torch"]
        print("texture input N=%d D=79  forward: hip %.4f ms, torch %.4f ms, %.1fx | forward + backward: hip %.4f ms, torch %.4f ms, %.1fx"
              % (n, h[0], t[0], t[0] / h[0], h[1], t[1], t[1] / h[1]), flush=True)


if __name__ == "__main__":
    main()
