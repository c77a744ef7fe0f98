"""Times the LPIPS-VGG perceptual loss: lpips.LPIPS(net='vgg') of this tree (csrc/lpips.hip) against the same network
as torch modules on the same device (F.conv2d through the vendor library, F.max_pool2d, the head written out), with the
same seeded random weights.  One call = what a training step does: the forward on two images (the rendered crop, which
needs a gradient, and the ground-truth crop, which does not) and the backward to the first, at the crops 256 x 160,
400 x 250 and 512 x 512.

After a warm-up, `--iters` calls are enqueued between two synchronisations; one sample is their mean, taken twice over the
same calls: wall time on the host, and device time between two events on the stream.  Reported: the median of `--runs`
samples and, in brackets, their smallest and largest; the achieved TFLOP/s of the fused path (611 712 FLOP per crop pixel
per image forward, twice that for a backward-data pass less its first layer's share: 3 x that per call, against the
155 TFLOP/s fp32 matrix rate).  Separately, for both implementations, the time of the FIRST call at a shape the process
has never seen (`--first`, a list of W x H): what a training run pays on each new crop size.

Usage:  python tools/lpips_time.py [--iters 5] [--runs 15] [--crops 256x160 400x250 512x512] [--first 399x250 400x251]  (W x H)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lpips  # noqa: E402
from gsplat_mi355 import lpips as gl  # noqa: E402

DEV = torch.device("cuda:0")
FLOP_PER_PIXEL = 611712  # one image forward


class TorchLPIPS(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.w = [sd[k + ".weight"].to(DEV) for k in gl.trunk_keys()]
        self.b = [sd[k + ".bias"].to(DEV) for k in gl.trunk_keys()]
        self.lin = [sd["lin%d.model.1.weight" % k].to(DEV) for k in range(5)]
        self.shift, self.scale = sd["scaling_layer.shift"].to(DEV), sd["scaling_layer.scale"].to(DEV)

    def taps(self, x):
        h, out = (2 * x[None] - 1 - self.shift) / self.scale, []
        for l in range(13):
            if l in (2, 4, 7, 10):
                h = F.max_pool2d(h, 2, 2)
            h = F.relu(F.conv2d(h, self.w[l], self.b[l], padding=1))
            if l in gl.TAP_LAYERS:
                out.append(h)
        return out

    def forward(self, a, b):
        unit = lambda f: f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)
        return sum(F.conv2d((unit(x) - unit(y)) ** 2, lin).mean() for x, y, lin in zip(self.taps(a), self.taps(b), self.lin))


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


def first_call(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shape(text):
    w, h = text.lower().split("x")
    return int(h), int(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--crops", type=shape, nargs="+", default=[shape("256x160"), shape("400x250"), shape("512x512")])
    ap.add_argument("--first", type=shape, nargs="*", default=[shape("399x250"), shape("400x251"), shape("397x247")])
    args = ap.parse_args()
    sd = gl.random_state_dict(0)
    hip = lpips.LPIPS(net="vgg", pretrained=False, verbose=False).to(DEV)
    ref = TorchLPIPS(sd)
    gen = torch.Generator(device=DEV).manual_seed(0)
    fmt = lambda s: "%.3f [%.3f .. %.3f]" % s

    def calls(h, w):
        a = torch.rand(3, h, w, device=DEV, generator=gen).requires_grad_(True)
        b = (a.detach() + 0.1 * torch.randn(3, h, w, device=DEV, generator=gen)).clamp(0, 1)
        return (("hip", lambda: torch.autograd.grad(hip(a, b, normalize=True).mean(), a)),
                ("torch", lambda: torch.autograd.grad(ref(a, b), a))), a, b

    for h, w in args.crops:
        impls, a, b = calls(h, w)
        with torch.no_grad():
            x, y = float(hip(a, b, normalize=True).mean()), float(ref(a, b))
        print("lpips %dx%d: loss hip %.8g, torch %.8g" % (w, h, x, y), flush=True)
        res = {name: timed(fn, args.iters, args.runs) for name, fn in impls}
        for j, clock in enumerate(("wall", "device")):
            p, t = res["hip"][j], res["torch"][j]
            clear = p[2] < t[1] or t[2] < p[1]
            print("lpips %dx%d forward x2 + backward x1, %s ms: hip %s, torch %s, %.2fx%s"
                  % (w, h, clock, fmt(p), fmt(t), t[0] / p[0], "" if clear else "  (the ranges overlap)"), flush=True)
        tf = 3.0 * FLOP_PER_PIXEL * h * w / (res["hip"][1][0] * 1e-3) / 1e12
        print("lpips %dx%d: %.1f TFLOP/s on the fused path (%.0f %% of 155)" % (w, h, tf, tf / 155 * 100), flush=True)
    for h, w in args.first:
        impls, a, b = calls(h, w)
        for name, fn in impls:
            print("lpips %dx%d first call at this shape, %s: %.2f ms" % (w, h, name, first_call(fn)), flush=True)


if __name__ == "__main__":
    main()
