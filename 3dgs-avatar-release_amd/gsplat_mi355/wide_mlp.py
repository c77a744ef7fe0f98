"""The coordinate networks the narrow fused MLP (gsplat_mi355.mlp) turns down -- models/network_utils.py VanillaCondMLP with a
frequency encoding, skip connections or width 256 (`non_rigid: mlp`, `texture: mlp`) and HannwCondMLP (`non_rigid:
hannw_mlp`) -- on the GPU through libgsplat_mi355 (csrc/mlp_wide.hip, whose header comment carries the spec): the encoding,
every Linear, the skip concatenations and the activations in one forward launch on the exact-fp32 MFMA, a condition row
that is never expanded over the batch, and a backward without atomics (bitwise reproducible), without host
synchronisation or host-to-device copies, capture-safe.

* `fused_wide_mlp(x, weights, biases, cond=None, multires=0, include_input=True, band_weights=None, skip_in=(),
  negative_slope=0.01)` -> (N, dout), one autograd node.
* `wide_mlp_supported(module)` -- whether a VanillaCondMLP's / HannwCondMLP's configuration is one the kernels take.
* `hann_band_weights(embedder_cfg, multires, iteration)` -- the Hann window's weight per frequency band.
* `hannw_mlp_forward(self, coords, iteration, cond=None)` -- HannwCondMLP.forward ("The MLPs").
* `DISPATCH` -- which classes of network `mlp.mlp_forward` and `hannw_mlp_forward` hand to these kernels by default
  (README.md records the measurement behind it); `fused_wide_mlp` is always available as the explicit call.
The band weights are kernel arguments by value: a captured graph freezes them (capture one graph per window state, or
capture after `full_band_iter`, when they are all 1).  Device fp32 tensors only: the fused path has no CPU version.
"""
import ctypes
import math
import os

import torch

from . import _lib, _wide_lib
from .mlp import _cfg, _cond_row, _layers

MAX_WIDTH, MAX_HIDDEN, MAX_FREQS = _wide_lib.GS_WMLP_MAX_WIDTH, _wide_lib.GS_WMLP_MAX_HIDDEN, _wide_lib.GS_WMLP_MAX_FREQS
MAX_ENC, MAX_COND, MAX_OUT = _wide_lib.GS_WMLP_MAX_ENC, _wide_lib.GS_WMLP_MAX_COND, _wide_lib.GS_WMLP_MAX_OUT
TILE_ROWS = _wide_lib.GS_WMLP_TILE_ROWS

# Which networks mlp_forward / hannw_mlp_forward hand to the wide kernels by default, per class: "coordinate" = a
# VanillaCondMLP with an encoding or a skip connection (non_rigid/mlp.yaml), "hannw" = a HannwCondMLP
# (non_rigid/hannw_mlp.yaml), "plain" = a VanillaCondMLP with neither (texture/mlp.yaml).  A class is on where
# tools/wide_mlp_time.py measured the fused forward + backward at 200k rows below torch's range (README.md: "The wide
# MLPs": 1.16x for non_rigid/mlp.yaml; 0.77x and 0.67x for the other two, which therefore stay on torch).
# GSPLAT_WIDE_MLP=1 / 0 in the environment turns all of them on / off.
DISPATCH = {"coordinate": True, "hannw": False, "plain": False}
if os.environ.get("GSPLAT_WIDE_MLP") in ("0", "1"):
    DISPATCH = dict.fromkeys(DISPATCH, os.environ["GSPLAT_WIDE_MLP"] == "1")


def rows_per_partial(n):
    """Rows one partial parameter gradient sums over at N = n (csrc/mlp_wide.hip: wm_rows_per_partial)."""
    per = -(-n // _wide_lib.GS_WMLP_MAX_PARTIALS)
    return max(_wide_lib.GS_WMLP_PARTIAL_MIN_ROWS, -(-per // 32) * 32)


def enc_dim(d, multires, include_input=True):
    """Columns of the encoding of d coordinates."""
    return d * ((1 if include_input else 0) + 2 * multires) if multires > 0 else d


def _limits_ok(E, C, width, n_hidden, dout, multires, skips):
    return (1 <= E <= MAX_ENC and 0 <= C <= MAX_COND and width % 32 == 0 and 32 <= width <= MAX_WIDTH
            and 1 <= n_hidden <= MAX_HIDDEN and 1 <= dout <= MAX_OUT and 0 <= multires <= MAX_FREQS
            and all(1 <= l <= n_hidden for l in skips) and (not skips or E < width))


def _args(n, d, multires, include_input, C, width, n_hidden, dout, skip_mask, slope, band, x, cond, weights, biases):
    a = _wide_lib.GsWideMlpArgs()
    a.N, a.dim_x, a.multires, a.include_input, a.dim_cond = n, d, multires, 1 if include_input else 0, C
    a.width, a.n_hidden, a.dim_out, a.skip_mask, a.slope = width, n_hidden, dout, skip_mask, slope
    for k, w in enumerate(band):
        a.band_w[k] = w
    a.x, a.cond = _lib.ptr(x), _lib.ptr(cond)
    for l, (w, b) in enumerate(zip(weights, biases)):
        a.W[l], a.b[l] = w.data_ptr(), b.data_ptr()
    return a


class _FusedWide(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cond, meta, *params):
        ctx.set_materialize_grads(False)
        multires, include_input, band, skip_mask, slope = meta
        nl = len(params) // 2
        dev, n, d = x.device, int(x.shape[0]), int(x.shape[1])
        x = x.detach().contiguous()
        cond = cond.detach().contiguous() if cond is not None else None
        params = [p.detach().contiguous() for p in params]  # (a transposed view is copied once)
        weights, biases = params[:nl], params[nl:]
        E = enc_dim(d, multires, include_input)
        C, width, dout = int(weights[0].shape[1]) - E, int(weights[-1].shape[1]), int(weights[-1].shape[0])
        shape = (n, d, multires, include_input, C, width, nl - 1, dout, skip_mask, slope, band)
        y = torch.empty(n, dout, dtype=torch.float32, device=dev)
        saved = None
        if n > 0:
            L = _wide_lib.load()
            a = _args(*shape, x, cond, weights, biases)
            if any(ctx.needs_input_grad):
                saved = torch.empty(_lib.nbytes(L.gs_wmlp_saved_bytes, ctypes.byref(a)) // 4, dtype=torch.float32, device=dev)
            ws = torch.empty(_lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), 0) // 4, dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                _lib.check(L.gs_wmlp_forward(ctypes.byref(a), _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), 4 * ws.numel(),
                                             _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, cond, saved, *params)
        ctx.shape = shape
        return y

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        if g is None or not any(need):
            return (None,) * len(need)
        shape = ctx.shape
        n, d, C = shape[0], shape[1], shape[4]
        x, cond, saved = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        nl = len(params) // 2
        weights, biases = params[:nl], params[nl:]
        dev = g.device
        new = torch.zeros if n == 0 else torch.empty
        dx = torch.empty(n, d, dtype=torch.float32, device=dev) if need[0] else None
        dcond = new(C, dtype=torch.float32, device=dev) if (need[1] and C > 0) else None
        dparams = [new(p.shape, dtype=torch.float32, device=dev) if nd else None for p, nd in zip(params, need[3:])]
        if n > 0:
            g = _lib.contiguous_aligned(g.to(torch.float32))
            L = _wide_lib.load()
            a = _args(*shape, x, cond, weights, biases)
            a.dx, a.dcond = _lib.ptr(dx), _lib.ptr(dcond)
            for l in range(nl):
                a.dW[l], a.db[l] = _lib.ptr(dparams[l]), _lib.ptr(dparams[nl + l])
            ws = torch.empty(_lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), 1) // 4, dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                _lib.check(L.gs_wmlp_backward(ctypes.byref(a), _lib.ptr(saved), _lib.ptr(g), _lib.ptr(ws), 4 * ws.numel(),
                                              _lib.stream_ptr(dev)))
        return (dx, dcond, None) + tuple(dparams)


def _f32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("fused_wide_mlp: %s: fp32 tensor expected" % name)
    return t


def fused_wide_mlp(x, weights, biases, cond=None, multires=0, include_input=True, band_weights=None, skip_in=(),
                   negative_slope=0.01):
    """y (N, dout) of the network csrc/mlp_wide.hip describes, as one autograd node.  e = enc(x): x itself at `multires` 0,
    else [x (with `include_input`) | w_0 sin(x) | w_0 cos(x) | w_1 sin(2 x) | .. ] with `band_weights` w (floats, one per
    band; None: all 1).  `weights` and `biases` are the nn.Linear parameters of the layers in order, shaped as the
    reference constructs them: 1..8 hidden layers of width W (a multiple of 32 up to 256, what the last layer reads);
    weights[0] has E + C columns; a layer l in `skip_in` (1..n_hidden) reads [h | e] / sqrt(2), and the layer before it has
    W - E outputs; dout <= 64.  `cond` is ONE row, (C,), (1, C) or an expand of either to x's rows, given exactly when
    weights[0] has more columns than E.  LeakyReLU(negative_slope >= 0; 0 is ReLU) between the layers, none after the
    last.  Gradients reach x, cond and every parameter that requires one."""
    _f32(x, "x")
    weights, biases = list(weights), list(biases)
    for k, w in enumerate(weights):
        _f32(w, "weights[%d]" % k)
    for k, b in enumerate(biases):
        _f32(b, "biases[%d]" % k)
    if cond is not None:
        _f32(cond, "cond")
    if x.dim() != 2:
        raise ValueError("fused_wide_mlp: x must be (N, d), got %s" % (tuple(x.shape),))
    n, d, nl = int(x.shape[0]), int(x.shape[1]), len(weights)
    if nl < 2 or len(biases) != nl:
        raise ValueError("fused_wide_mlp: one bias per weight and at least two layers expected, got %d and %d" % (nl, len(biases)))
    if any(w.dim() != 2 for w in weights) or any(b.dim() != 1 for b in biases):
        raise ValueError("fused_wide_mlp: weights (out, in) and biases (out,) expected")
    multires, include_input, slope = int(multires), bool(include_input), float(negative_slope)
    skips = sorted(set(int(l) for l in skip_in))
    if not 0 <= multires <= MAX_FREQS:
        raise ValueError("fused_wide_mlp: multires must be in 0..%d, got %d" % (MAX_FREQS, multires))
    band = (1.0,) * multires if band_weights is None else tuple(float(w) for w in band_weights)
    if len(band) != multires or any(w != w for w in band):
        raise ValueError("fused_wide_mlp: one band weight per frequency (%d) expected, got %r" % (multires, band))
    if not slope >= 0.0 or math.isinf(slope):
        raise ValueError("fused_wide_mlp: negative_slope must be a finite number >= 0, got %r" % (negative_slope,))
    E = enc_dim(d, multires, include_input)
    width, dout = int(weights[-1].shape[1]), int(weights[-1].shape[0])
    C = int(weights[0].shape[1]) - E
    row = None
    if cond is not None:
        row = _cond_row(cond, n)
        if row is None:
            raise ValueError("fused_wide_mlp: cond must be one row -- (C,), (1, C) or an expand of either -- got %s with strides %s"
                             % (tuple(cond.shape), tuple(cond.stride())))
    if C < 0 or (C > 0) != (row is not None) or (row is not None and int(row.shape[0]) != C):
        raise ValueError("fused_wide_mlp: weights[0] has %d columns: the encoding has %d and cond %s"
                         % (int(weights[0].shape[1]), E, "none" if row is None else int(row.shape[0])))
    if not _limits_ok(E, C, width, nl - 1, dout, multires, skips):
        raise ValueError("fused_wide_mlp: encoding %d, cond %d, width %d, %d hidden layers, dout %d, multires %d, skip_in %s is "
                         "outside what the kernels take (wide_mlp_supported)" % (E, C, width, nl - 1, dout, multires, skips))
    for l in range(nl):
        want = (dout if l == nl - 1 else (width - E if l + 1 in skips else width), E + C if l == 0 else width)
        if tuple(weights[l].shape) != want or tuple(biases[l].shape) != want[:1]:
            raise ValueError("fused_wide_mlp: layer %d must be %s with a bias %s, got %s and %s"
                             % (l, want, want[:1], tuple(weights[l].shape), tuple(biases[l].shape)))
    for t, name in [(x, "x"), (cond, "cond")] + [(w, "weights") for w in weights] + [(b, "biases") for b in biases]:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fused_wide_mlp: %s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)
    meta = (multires, include_input, band, sum(1 << l for l in skips), slope)
    return _FusedWide.apply(x, row, meta, *(weights + biases))


def _is_hannw(module):
    return _cfg(module.config, "embedder", None) is not None


def _shape_of(module):
    """(width, n_hidden, dout, total input columns of lin0, skips, E the skips imply or None, multires, slope), or None
    when the module is not one the kernels take -- from `config`, the activation and the shapes of lin0, lin1, .. alone."""
    config = module.config
    cond_in = [int(l) for l in _cfg(config, "cond_in", [])]
    skips = sorted(set(int(l) for l in _cfg(config, "skip_in", [])))
    multires = int(_cfg(config, "multires", 0))
    if cond_in not in ([], [0]) or not 0 <= multires <= MAX_FREQS:
        return None
    act = module.activation
    if isinstance(act, torch.nn.LeakyReLU):
        slope = float(act.negative_slope)
    elif isinstance(act, torch.nn.ReLU):
        slope = 0.0
    else:
        return None
    if not slope >= 0.0:
        return None
    lins = _layers(module)
    if len(lins) < 2 or any(lin.bias is None for lin in lins):
        return None
    n_hidden, width, dout = len(lins) - 1, lins[-1].in_features, lins[-1].out_features
    if any(not 1 <= l <= n_hidden for l in skips):
        return None
    E = width - lins[skips[0] - 1].out_features if skips else None
    if skips and not 1 <= E < width:
        return None
    for l, lin in enumerate(lins):
        if l > 0 and lin.in_features != width:
            return None
        if l < n_hidden and lin.out_features != (width - E if l + 1 in skips else width):
            return None
    total = lins[0].in_features
    if skips and (total < E or (not cond_in and total != E)):
        return None
    if not (2 <= total <= MAX_ENC + MAX_COND if cond_in else 1 <= total <= MAX_ENC):
        return None
    if not (width % 32 == 0 and 32 <= width <= MAX_WIDTH and n_hidden <= MAX_HIDDEN and 1 <= dout <= MAX_OUT):
        return None
    return width, n_hidden, dout, total, skips, E, multires, slope


def wide_mlp_supported(module):
    """True when the wide kernels take this VanillaCondMLP or HannwCondMLP: `multires` 0..10, skip connections at any of
    the layers 1..n_hidden (the layer before each with W - E outputs, E < W), the condition on the first layer or nowhere,
    LeakyReLU or ReLU, 1..8 hidden layers of one width (a multiple of 32 up to 256), an encoding of at most 512 columns
    with a condition of at most 512 (how lin0's columns split between the two is known at the call), at most 64 outputs."""
    return _shape_of(module) is not None


def _dispatch_class(module, shape):
    if _is_hannw(module):
        return "hannw"
    return "coordinate" if (shape[6] > 0 or shape[4]) else "plain"


def _call(module, coords, cond, include_input, band):
    """The fused call for `module`, or None where this call is not one the kernels take (the caller evaluates it in
    torch): CPU tensors, a condition whose rows may differ, an input whose encoding does not fill lin0's columns."""
    shape = module.__dict__.get("_gsplat_wide_shape", False)
    if shape is False:
        shape = module.__dict__["_gsplat_wide_shape"] = _shape_of(module)
    if shape is None or not coords.is_cuda or coords.dtype != torch.float32:
        return None
    width, n_hidden, dout, total, skips, E_skip, multires, slope = shape
    uses_cond = len(_cfg(module.config, "cond_in", [])) > 0
    d = int(coords.shape[-1])
    n = coords.numel() // max(d, 1)
    row = None
    if uses_cond:
        row = _cond_row(cond, n) if (cond is not None and coords.dim() == 2) else None
        if row is None or not row.is_cuda:
            return None
    E = enc_dim(d, multires, include_input)
    C = int(row.shape[0]) if row is not None else 0
    if d < 1 or total != E + C or (skips and E != E_skip) or not _limits_ok(E, C, width, n_hidden, dout, multires, skips):
        return None
    lins = _layers(module)
    y = fused_wide_mlp(coords.reshape(-1, d), [lin.weight for lin in lins], [lin.bias for lin in lins], cond=row,
                       multires=multires, include_input=include_input, band_weights=band, skip_in=skips, negative_slope=slope)
    return y.reshape(tuple(coords.shape[:-1]) + (dout,))


def vanilla_forward(module, coords, cond):
    """What mlp.mlp_forward does with a VanillaCondMLP the narrow kernels turn down: the fused result where the wide
    kernels take the module and this call and DISPATCH hands its class to them, else None."""
    shape = module.__dict__.get("_gsplat_wide_shape", False)
    if shape is False:
        shape = module.__dict__["_gsplat_wide_shape"] = _shape_of(module)
    if shape is None or _is_hannw(module) or not DISPATCH[_dispatch_class(module, shape)]:
        return None
    return _call(module, coords, cond, True, None)


def hann_band_weights(embedder_cfg, multires, iteration):
    """The Hann window's weight of each of the `multires` frequency bands at `iteration`, as HannwEmbedder computes them
    (models/network_utils.py:79-92) -- the same torch fp32 operations on the CPU, all bands at once -- as Python floats:
    all 1 when full_band_iter <= 0 or kick_in_iter >= full_band_iter, else (1 - cos(pi clamp(alpha - k, 0, 1))) / 2 with
    alpha = multires max(iteration - kick_in_iter, 0) / (full_band_iter - kick_in_iter)."""
    m = int(multires)
    full, kick = _cfg(embedder_cfg, "full_band_iter", 0), _cfg(embedder_cfg, "kick_in_iter", 0)
    if full <= 0 or kick >= full:
        alpha = torch.tensor(m, dtype=torch.float32)
    else:
        kick_t = torch.tensor(kick, dtype=torch.float32)
        t = torch.clamp(iteration - kick_t, min=0.)
        alpha = m * t / (full - kick_t)
    k = torch.arange(m, dtype=torch.float32)
    w = (1. - torch.cos(math.pi * torch.clamp(alpha - k, min=0., max=1.))) / 2.
    return tuple(float(v) for v in w.tolist())


def _torch_hannw_forward(self, coords, iteration, cond):
    """HannwCondMLP.forward layer by layer in torch: the windowed encoding (no raw input), the condition on the layers in
    `cond_in`, the encoding rejoining at the layers in `skip_in` scaled by 1 / sqrt(2)."""
    config = self.config
    cond_in = [int(l) for l in _cfg(config, "cond_in", [])]
    skip_in = [int(l) for l in _cfg(config, "skip_in", [])]
    multires = int(_cfg(config, "multires", 0))
    if cond is not None:
        cond = cond.expand(coords.shape[0], -1)
    first = coords
    if multires > 0:
        band = hann_band_weights(_cfg(config, "embedder", None), multires, iteration)
        blocks = []
        for k, w in enumerate(band):
            scaled = coords * float(2 ** k)
            blocks += [w * torch.sin(scaled), w * torch.cos(scaled)]
        first = torch.cat(blocks, dim=-1)
    h, lins = first, _layers(self)
    for l, lin in enumerate(lins):
        if l in cond_in:
            h = torch.cat((h, cond), dim=1)
        if l in skip_in:
            h = torch.cat((h, first), dim=1) / math.sqrt(2.0)
        h = lin(h)
        if l + 1 < len(lins):
            h = self.activation(h)
    return h


def hannw_mlp_forward(self, coords, iteration, cond=None):
    """HannwCondMLP.forward (models/network_utils.py:299-324): the Hann-windowed encoding without the raw input, ReLU.  Through
    `fused_wide_mlp` where `wide_mlp_supported` takes the module, the tensors are on the GPU, the condition is one row and
    DISPATCH["hannw"] is on; in plain torch otherwise.  The band weights of `iteration` go to the kernels by value."""
    shape = self.__dict__.get("_gsplat_wide_shape", False)
    if shape is False:
        shape = self.__dict__["_gsplat_wide_shape"] = _shape_of(self)
    if shape is not None and DISPATCH["hannw"]:
        multires = shape[6]
        band = hann_band_weights(_cfg(self.config, "embedder", None), multires, iteration) if multires > 0 else None
        y = _call(self, coords, cond, False, band)
        if y is not None:
            return y
    return _torch_hannw_forward(self, coords, iteration, cond)
