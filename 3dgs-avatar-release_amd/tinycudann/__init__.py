"""Drop-in for the one tiny-cuda-nn class the reference uses: `tinycudann.Encoding` with a HashGrid config
(models/network_utils.py:4,337: `import tinycudann as tcnn`; `tcnn.Encoding(3, config)`).  The work runs in
libgsplat_mi355's HIP kernels (csrc/hashgrid.hip) through gsplat_mi355.hashgrid; there is no CPU path.

Supported: HashGrid (a config without `otype` counts as one), 3-D input, linear interpolation, forward and first-order
backward.  Differences from tcnn by design: fp32 parameters and arithmetic (tcnn keeps fp16
copies and uses a loss scale of 128); fp32 output by default (`dtype=torch.float16` gives the fp32 result rounded once);
initial values uniform in [-1e-4, 1e-4] as in tcnn, but drawn from a CPU torch.Generator seeded with `seed`; a bitwise
reproducible parameter gradient.  Other tcnn classes (Network, NetworkWithInputEncoding, ...) are not provided.
"""
import torch

from gsplat_mi355 import hashgrid as _hg

__all__ = ["Encoding"]

_NOT_PROVIDED = ("Network", "NetworkWithInputEncoding", "Module", "free_temporary_memory", "supports_jit_fusion",
                 "preferred_precision")


class Encoding(_hg.HashGridEncoding):
    """tcnn.Encoding(n_input_dims, encoding_config, seed=1337, dtype=None) for HashGrid configs.  One flat fp32 parameter
    `params` (the state-dict key tcnn uses); forward(x [B, n_input_dims], any float dtype and strides) -> [B, n_output_dims]
    in `dtype` (default fp32); the gradient of x returns in x's dtype."""

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        if dtype not in (None, torch.float32, torch.float16):
            raise NotImplementedError("tinycudann.Encoding: dtype = %r; float32 or float16 are supported" % (dtype,))
        super().__init__(encoding_config, seed=seed, n_input_dims=n_input_dims)
        self.dtype = torch.float32 if dtype is None else dtype
        self.seed = seed

    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError("tinycudann.Encoding: x must be (B, %d), got %s" % (self.n_input_dims, tuple(x.shape)))
        out = super().forward(x)
        return out if self.dtype == torch.float32 else out.to(self.dtype)

    def extra_repr(self):
        return "n_input_dims=%d, n_output_dims=%d, seed=%d, dtype=%s, encoding_config=%s" % (
            self.n_input_dims, self.n_output_dims, self.seed, self.dtype, self.cfg)


def __getattr__(name):
    if name in _NOT_PROVIDED:
        raise ImportError("tinycudann.%s is not provided: this package implements tinycudann.Encoding (HashGrid) only; "
                          "the reference's MLPs are torch modules" % name)
    raise AttributeError("module 'tinycudann' has no attribute %r" % name)
