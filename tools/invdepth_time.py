"""Times the rasterizer's inverse-depth image (GaussianRasterizer.forward(..., with_invdepth=True)): forward + backward of

  (A) the colour image alone;
  (B) colour and inverse depth from one call (`with_invdepth=True`): a shared-geometry second render inside the node, ONE
      render backward for both images, the second image's colour gradient from csrc/second_colors.hip;
  (C) what a caller had to write without the option: a second rasterizer call with colors_precomp = 1/z requiring a
      gradient -- the forward is shared, but each call runs a backward of its own;

at the headline workload (200k Gaussians / 1024 x 1024 / SH degree 3) or `--workload avatar` (the body-shaped cloud at
512 x 512), with the benchmark's cloud and orbit camera.  The loss is a fixed random gradient image per output.

After a warm-up, `--iters` steps are enqueued between two synchronisations; one sample is their mean, taken twice over
the same steps: wall time on the host, and device time between two events on the stream.  Reported: the median of
`--runs` samples and, in brackets, their smallest and largest; B against C with whether the two ranges are disjoint (the
new kernel earns its place only if they are, B below C).

Usage:  python tools/invdepth_time.py [--workload config3|avatar] [--iters 5] [--runs 15] [--legs ABC]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
from gsplat_mi355.camera import orbit_camera  # noqa: E402
from gsplat_mi355.scenes import synthetic_cloud  # noqa: E402

DEV = torch.device("cuda:0")
WORKLOADS = {"config3": (200000, 1024, 1024, "box"), "avatar": (200000, 512, 512, "body")}  # (bench.py: WORKLOADS)


def timed(fn, iters, runs):
    """((median, min, max) wall ms, (median, min, max) device ms) per call."""
    for _ in range(3):
        fn()
    wall, device = [], []
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / iters * 1e3)
        device.append(start.elapsed_time(stop) / iters)
    stats = lambda s: (sorted(s)[len(s) // 2], min(s), max(s))
    return stats(wall), stats(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3", choices=sorted(WORKLOADS))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--legs", default="ABC", help="which of A, B, C to time (A alone also runs on a tree without the option)")
    args = ap.parse_args()
    N, W, H, layout = WORKLOADS[args.workload]
    cloud = synthetic_cloud(N, sh_degree=3, seed=0, device=DEV, layout=layout)
    cam = orbit_camera(0, W, H, device=DEV)
    settings = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(3, device=DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False)
    rast = dgr.GaussianRasterizer(settings)
    leaves = dict(means3D=cloud.xyz, opacities=cloud.opacity, scales=cloud.scales, rotations=cloud.rotations, shs=cloud.shs)
    for t in leaves.values():
        t.requires_grad_(True)
    leaves["means2D"] = torch.zeros(N, 3, device=DEV, requires_grad=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    gC = torch.randn(3, H, W, device=DEV, generator=gen)
    gD = torch.randn(1, H, W, device=DEV, generator=gen)
    V = cam.world_view_transform
    zero = torch.zeros((), device=DEV)
    params = list(leaves.values())
    geometry = {k: v for k, v in leaves.items() if k != "shs"}

    def colour_only():
        color, _ = rast(**leaves)
        return torch.autograd.grad((color * gC).sum(), params, allow_unused=True)

    def one_call():
        color, _, inv = rast(with_invdepth=True, **leaves)
        return torch.autograd.grad((color * gC).sum() + (inv * gD).sum(), params, allow_unused=True)

    def two_calls():
        color, radii = rast(**leaves)
        z = leaves["means3D"] @ V[:3, 2] + V[3, 2]
        inv = torch.where(radii > 0, 1.0 / z, zero)
        img2, _ = rast(colors_precomp=inv.unsqueeze(1).expand(N, 3), **geometry)
        return torch.autograd.grad((color * gC).sum() + (img2[:1] * gD).sum(), params, allow_unused=True)

    if "B" in args.legs:
        with torch.no_grad():
            inv = rast(with_invdepth=True, **leaves)[2]
        print("invdepth %s: %d Gaussians, %d x %d; image mean %.6g, max %.6g"
              % (args.workload, N, W, H, float(inv.mean()), float(inv.max())), flush=True)
    fmt = lambda s: "%.3f [%.3f .. %.3f]" % s
    res = {}
    for name, fn in (("A colour only", colour_only), ("B with_invdepth", one_call), ("C two calls", two_calls)):
        if name[0] not in args.legs:
            continue
        dgr.release_shared_geometry()
        res[name] = timed(fn, args.iters, args.runs)
        for j, clock in enumerate(("wall", "device")):
            print("invdepth %s forward + backward, %s ms: %s %s" % (args.workload, clock, name, fmt(res[name][j])), flush=True)
    for j, clock in enumerate(("wall", "device") if set("ABC") <= set(args.legs) else ()):
        b, c = res["B with_invdepth"][j], res["C two calls"][j]
        verdict = "B below C, ranges disjoint" if b[2] < c[1] else ("C below B, ranges disjoint" if c[2] < b[1] else "the ranges overlap")
        print("invdepth %s, %s: B %.3f ms against C %.3f ms, %.2fx (%s); B - A = %.3f ms"
              % (args.workload, clock, b[0], c[0], c[0] / b[0], verdict, b[0] - res["A colour only"][j][0]), flush=True)


if __name__ == "__main__":
    main()
