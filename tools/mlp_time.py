"""Times the fused MLP: gsplat_mi355.mlp.fused_mlp (csrc/mlp.hip) against the same network as a torch module on the same
device (nn.Linear layers and nn.LeakyReLU as VanillaCondMLP chains them, the condition row expanded over the batch and
concatenated to the input as the reference does), for the three networks of the default config:
  skinning  3 -> 128 x4 -> 25          nonrigid  32 (+144 cond) -> 128 x3 -> 26          texture  79 -> 64 x2 -> 3
Forward alone (no_grad) and forward + backward (torch.autograd.grad with an upstream gradient, to x, the condition and every
parameter).  After a warm-up, `--iters` calls are enqueued between two synchronisations; one sample is their mean, taken
twice over the same calls: wall time on the host, and device time between two events on the stream.  Reported: the median
of `--runs` samples and, in brackets, their smallest and largest.

Usage:  python tools/mlp_time.py [--iters 20] [--runs 15] [--rows 50000 200000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

from gsplat_mi355 import mlp  # noqa: E402

DEV = torch.device("cuda:0")
NETWORKS = (("skinning", 3, 0, 128, 4, 25), ("nonrigid", 32, 144, 128, 3, 26), ("texture", 79, 0, 64, 2, 3))


class TorchMLP(torch.nn.Module):
    def __init__(self, din, C, width, n_hidden, dout):
        super().__init__()
        dims = [din + C] + [width] * n_hidden + [dout]
        self.layers = torch.nn.ModuleList(torch.nn.Linear(i, o) for i, o in zip(dims[:-1], dims[1:]))
        self.activation = torch.nn.LeakyReLU()

    def forward(self, x, cond=None):
        if cond is not None:
            x = torch.cat([x, cond.expand(x.shape[0], -1)], 1)
        for l, layer in enumerate(self.layers):
            x = layer(x)
            if l + 1 < len(self.layers):
                x = self.activation(x)
        return x


def timed(fn, iters, runs):
    """((median, min, max) wall ms, (median, min, max) device ms) per call."""
    for _ in range(5):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--rows", type=int, nargs="+", default=[50000, 200000])
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    fmt = lambda s: "%.3f [%.3f .. %.3f]" % s
    for name, din, C, width, n_hidden, dout in NETWORKS:
        torch.manual_seed(0)
        net = TorchMLP(din, C, width, n_hidden, dout).to(DEV)
        weights, biases = [l.weight for l in net.layers], [l.bias for l in net.layers]
        cond = torch.randn(1, C, device=DEV, generator=gen).requires_grad_(True) if C else None
        for n in args.rows:
            x = (2 * torch.rand(n, din, device=DEV, generator=gen) - 1).requires_grad_(True)
            g = torch.randn(n, dout, device=DEV, generator=gen)
            leaves = [x] + ([cond] if C else []) + list(net.parameters())
            impls = (("hip", lambda: mlp.fused_mlp(x, weights, biases, cond=cond)), ("torch", lambda: net(x, cond)))
            with torch.no_grad():
                a, b = impls[0][1](), impls[1][1]()
                print("%s N=%d: largest difference between the two outputs %.3g of %.3g"
                      % (name, n, float((a - b).abs().max()), float(b.abs().max())), flush=True)
            res = {}
            for impl, fn in impls:
                def fwd():
                    with torch.no_grad():
                        fn()

                def fwd_bwd():
                    torch.autograd.grad(fn(), leaves, grad_outputs=g)
                res[impl] = (timed(fwd, args.iters, args.runs), timed(fwd_bwd, args.iters, args.runs))
            for k, what in enumerate(("forward", "forward + backward")):
                for j, clock in enumerate(("wall", "device")):
                    h, t = res["hip"][k][j], res["torch"][k][j]
                    clear = h[2] < t[1]  # the slowest fused sample under the fastest torch sample
                    print("mlp %s N=%d %s, %s ms: hip %s, torch %s, %.2fx%s"
                          % (name, n, what, clock, fmt(h), fmt(t), t[0] / h[0], "" if clear else "  (the ranges overlap)"), flush=True)


if __name__ == "__main__":
    main()
