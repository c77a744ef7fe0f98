"""Times the converter's optimizer step (models/gaussian_converter.py:61-67) over a parameter set of the default
modules' shape -- 129 tensors: the skinning MLP (10), the hierarchical pose encoder (98 tensors of a few hundred floats),
the hash-grid table (1.7 M floats), the non-rigid MLP (8), betas and four pose embeddings, the colour MLP (6) and its
latent embedding; weight decay 0.05 on the latent group, grad_clip 0.1, ExponentialLR -- with random gradients:

  torch   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step (foreach) + zero_grad + scheduler.step
  fused   gsplat_mi355.optim.converter_optimize on a FusedAdam (the same four steps)
  graph   a torch.cuda.graph replay of FusedAdam(capturable=True, max_grad_norm=0.1).step() alone (static gradients)

Both eager sequences re-attach the same gradient tensors before every call (zero_grad drops them).  After a warm-up,
`--iters` calls are enqueued between two synchronisations and their mean is one sample; the median of `--runs` samples
is reported.

Usage:  python tools/optim_time.py [--iters 50] [--runs 15]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

from gsplat_mi355.optim import FusedAdam, converter_optimize  # noqa: E402

DEV = torch.device("cuda:0")
FRAMES = 500


def mlp(d_in, width, depth, d_out):
    dims = [d_in] + [width] * depth + [d_out]
    return [s for a, b in zip(dims[:-1], dims[1:]) for s in ((b, a), (b,))]


# (group, lr, weight_decay, shapes)
GROUPS = [
    ("rigid", 1e-4, 0.0, mlp(39, 128, 4, 25)),                                                        # 10
    ("non_rigid", 1e-3, 0.0, [(6, 12), (6,)] + [s for _ in range(24) for s in ((16, 18), (16,), (6, 16), (6,))]   # 98
     + [(1700000,)] + mlp(176, 128, 3, 10)),                                                          # 1 + 8
    ("pose_correction", 1e-4, 0.0, [(1, 10), (FRAMES, 3), (FRAMES, 63), (FRAMES, 6), (FRAMES, 3)]),   # 5
    ("texture", 1e-3, 0.0, mlp(70, 256, 2, 3)),                                                       # 6
    ("tex_latent", 1e-3, 0.05, [(FRAMES, 16)]),                                                       # 1
]


class Opt(dict):
    pass


class Cfg(object):
    opt = Opt(grad_clip=0.1)


class Converter(torch.nn.Module):
    def __init__(self, cls, **kw):
        super().__init__()
        gen = torch.Generator(device=DEV).manual_seed(0)
        self.cfg = Cfg()
        groups = []
        self.ps = torch.nn.ParameterList()
        for _name, lr, wd, shapes in GROUPS:
            members = [torch.nn.Parameter(torch.randn(*s, device=DEV, generator=gen)) for s in shapes]
            self.ps.extend(members)
            groups.append(dict(params=members, lr=lr, weight_decay=wd))
        self.grads = [torch.randn(p.shape, device=DEV, generator=gen) for p in self.ps]
        self.optimizer = cls(groups, lr=1e-3, eps=1e-15, **kw)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=0.1 ** (1.0 / 60000))

    def attach(self):
        for p, g in zip(self.ps, self.grads):
            p.grad = g


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

    ref = Converter(torch.optim.Adam, foreach=True)

    def torch_step():
        ref.attach()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.1)
        ref.optimizer.step()
        ref.optimizer.zero_grad()
        ref.scheduler.step()

    mine = Converter(FusedAdam)

    def fused_step():
        mine.attach()
        converter_optimize(mine)

    t_torch = timed(torch_step, args.iters, args.runs)
    t_fused = timed(fused_step, args.iters, args.runs)

    cap = Converter(FusedAdam, capturable=True, max_grad_norm=0.1)
    cap.attach()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(3):
            cap.optimizer.step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.optimizer.step()
    t_graph = timed(graph.replay, args.iters, args.runs)

    n = len(mine.ps)
    print("%d tensors, %d floats | torch clip + Adam(foreach) + zero_grad + scheduler: %.4f ms | converter_optimize on FusedAdam: "
          "%.4f ms, %.1fx | graph replay of the capturable step alone: %.4f ms"
          % (n, sum(p.numel() for p in mine.ps), t_torch, t_fused, t_torch / t_fused, t_graph), flush=True)


if __name__ == "__main__":
    main()
