"""Times the wide fused MLP: gsplat_mi355.wide_mlp.fused_wide_mlp (csrc/mlp_wide.hip) against the same module on the path it
took before these kernels existed, on the same device -- gsplat_mi355.mlp._torch_forward for a VanillaCondMLP and the
layer-by-layer HannwCondMLP forward (wide_mlp._torch_hannw_forward) -- for the reference's three wide networks:
  nonrigid  3 -> enc 39 (+144 cond) -> 256 x8 -> 26, skip_in [4]      (non_rigid/mlp.yaml)
  hannw     3 -> windowed enc 36 (+144 cond) -> 256 x8 -> 10, skip_in [4], ReLU   (non_rigid/hannw_mlp.yaml, mid-window)
  texture   271 -> 256 x4 -> 3                                        (texture/mlp.yaml)
Forward alone (no_grad) and forward + backward (torch.autograd.grad with an upstream gradient, to x, the condition and every
parameter).  After a warm-up, `--iters` calls are enqueued between two synchronisations; one sample is their mean, taken
twice over the same calls: wall time on the host, and device time between two events on the stream.  Reported: the median
of `--runs` samples and, in brackets, their smallest and largest.  The last line per network says what wide_mlp.DISPATCH
should hold for its class: on only where the fused forward + backward range at the largest N lies below torch's.

Usage:  python tools/wide_mlp_time.py [--iters 10] [--runs 15] [--rows 50000 200000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from gsplat_mi355 import mlp, wide_mlp  # noqa: E402
from mlp_time import timed  # noqa: E402

DEV = torch.device("cuda:0")
EMBEDDER = dict(kick_in_iter=3000, full_band_iter=10000)
ITERATION = 5800  # mid-window: band weights (1, 1, 0.35, 0, 0, 0)
# name: (d, multires, cond, width, hidden layers, skip_in, dout, hannw)
NETWORKS = (("nonrigid", 3, 6, 144, 256, 8, (4,), 26, False), ("hannw", 3, 6, 144, 256, 8, (4,), 10, True),
            ("texture", 271, 0, 0, 256, 4, (), 3, False))


def module(d, multires, C, width, n_hidden, skip_in, dout, hannw):
    """What VanillaCondMLP.__init__ / HannwCondMLP.__init__ leave on the module (nn.Linear's own initialisation)."""
    m = torch.nn.Module()
    m.config = dict(multires=multires, skip_in=list(skip_in), cond_in=[0] if C else [], n_neurons=width, n_hidden_layers=n_hidden)
    if hannw:
        m.config["embedder"] = dict(EMBEDDER)
    E = wide_mlp.enc_dim(d, multires, not hannw)
    m.num_layers, m.embed_fn = n_hidden + 2, None
    if multires > 0 and not hannw:
        m.embed_fn = lambda x: torch.cat([x] + [f(x * 2.0 ** k) for k in range(multires) for f in (torch.sin, torch.cos)], -1)
    for l in range(n_hidden + 1):
        out = dout if l == n_hidden else (width - E if l + 1 in skip_in else width)
        setattr(m, "lin%d" % l, torch.nn.Linear(E + C if l == 0 else width, out))
    m.activation = torch.nn.ReLU() if hannw else torch.nn.LeakyReLU()
    return m.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--rows", type=int, nargs="+", default=[50000, 200000])
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    fmt = lambda s: "%.3f [%.3f .. %.3f]" % s
    for name, d, multires, C, width, n_hidden, skip_in, dout, hannw in NETWORKS:
        torch.manual_seed(0)
        net = module(d, multires, C, width, n_hidden, skip_in, dout, hannw)
        assert wide_mlp.wide_mlp_supported(net) and not mlp.mlp_supported(net)
        lins = mlp._layers(net)
        weights, biases = [l.weight for l in lins], [l.bias for l in lins]
        cond = torch.randn(1, C, device=DEV, generator=gen).requires_grad_(True) if C else None
        band = wide_mlp.hann_band_weights(EMBEDDER, multires, ITERATION) if hannw else None
        slope = 0.0 if hannw else net.activation.negative_slope
        verdict = None
        for n in args.rows:
            x = (2 * torch.rand(n, d, device=DEV, generator=gen) - 1).requires_grad_(True)
            g = torch.randn(n, dout, device=DEV, generator=gen)
            leaves = [x] + ([cond] if C else []) + list(net.parameters())
            fused = lambda: wide_mlp.fused_wide_mlp(x, weights, biases, cond=cond, multires=multires, include_input=not hannw,
                                                    band_weights=band, skip_in=skip_in, negative_slope=slope)
            before = (lambda: wide_mlp._torch_hannw_forward(net, x, ITERATION, cond)) if hannw else (lambda: mlp._torch_forward(net, x, cond))
            impls = (("hip", fused), ("torch", before))
            with torch.no_grad():
                a, b = fused(), before()
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
                    print("wide mlp %s N=%d %s, %s ms: hip %s, torch %s, %.2fx%s"
                          % (name, n, what, clock, fmt(h), fmt(t), t[0] / h[0], "" if clear else "  (not clearly faster)"), flush=True)
            verdict = all(res["hip"][1][j][2] < res["torch"][1][j][1] for j in range(2))
        print("wide mlp %s: forward + backward at N=%d %s torch's range -> DISPATCH[%r] %s"
              % (name, args.rows[-1], "lies below" if verdict else "does not lie below",
                 "hannw" if hannw else ("coordinate" if (multires > 0 or skip_in) else "plain"), "on" if verdict else "off"), flush=True)


if __name__ == "__main__":
    main()
