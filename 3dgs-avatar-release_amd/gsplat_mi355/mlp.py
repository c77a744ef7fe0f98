"""The dense networks of the avatar model (models/network_utils.py VanillaCondMLP: the skinning field, the non-rigid
deformer's MLP, the colour MLP) on the GPU through libgsplat_mi355 (csrc/mlp.hip, whose header comment carries the spec):
Linear layers of one hidden width with LeakyReLU between them, the matrix products on the exact-fp32 MFMA, a row tile's
activations kept on chip from the input to the output, a condition row that is never expanded over the batch, and a
backward without atomics (bitwise reproducible), without host synchronisation or host-to-device copies, capture-safe.

* `fused_mlp(x, weights, biases, cond=None, negative_slope=0.01)` -> (N, dout), one autograd node.
* `mlp_supported(module)` -- whether a VanillaCondMLP's configuration is one the kernels take.
* `mlp_forward(self, coords, cond=None)` -- VanillaCondMLP.forward ("The MLPs"); a configuration outside
  these kernels' (positional encoding, skip connections, width 256) goes to the wide kernels (gsplat_mi355.wide_mlp ->
  csrc/mlp_wide.hip) where they take it, the tensors are on the GPU and wide_mlp.DISPATCH hands its class to them, and is
  evaluated in plain torch otherwise.
Device fp32 tensors only: the fused path has no CPU version.
"""
import ctypes
import math

import torch

from . import _lib

MAX_WIDTH, MAX_HIDDEN, MAX_IN = _lib.GS_MLP_MAX_WIDTH, _lib.GS_MLP_MAX_HIDDEN, _lib.GS_MLP_MAX_IN
MAX_COND, MAX_OUT = _lib.GS_MLP_MAX_COND, _lib.GS_MLP_MAX_OUT
TILE_ROWS = _lib.GS_MLP_TILE_ROWS


def rows_per_partial(n):
    """Rows one partial parameter gradient sums over at N = n (csrc/mlp.hip: ml_rows_per_partial)."""
    per = -(-n // _lib.GS_MLP_MAX_PARTIALS)
    return max(_lib.GS_MLP_PARTIAL_MIN_ROWS, -(-per // 32) * 32)


def _shapes_ok(din, C, width, n_hidden, dout):
    return (1 <= din <= MAX_IN and 0 <= C <= MAX_COND and width % 32 == 0 and 32 <= width <= MAX_WIDTH
            and 1 <= n_hidden <= MAX_HIDDEN and 1 <= dout <= MAX_OUT)


def _args(n, din, C, width, n_hidden, dout, slope, x, cond, weights, biases):
    a = _lib.GsMlpArgs()
    a.N, a.dim_in, a.dim_cond, a.width, a.n_hidden, a.dim_out, a.slope = n, din, C, width, n_hidden, dout, slope
    a.x, a.cond = _lib.ptr(x), _lib.ptr(cond)
    for l, (w, b) in enumerate(zip(weights, biases)):
        a.W[l], a.b[l] = w.data_ptr(), b.data_ptr()
    return a


class _Fused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cond, slope, *params):
        ctx.set_materialize_grads(False)
        nl = len(params) // 2
        dev, n, din = x.device, int(x.shape[0]), int(x.shape[1])
        x = _lib.contiguous_aligned(x.detach())
        cond = cond.detach().contiguous() if cond is not None else None
        params = [p.detach().contiguous() for p in params]  # (a transposed view is copied once)
        weights, biases = params[:nl], params[nl:]
        C, width, dout = int(weights[0].shape[1]) - din, int(weights[0].shape[0]), int(weights[-1].shape[0])
        y = torch.empty(n, dout, dtype=torch.float32, device=dev)
        acts = torch.empty(nl - 1, n, width, dtype=torch.float32, device=dev) if any(ctx.needs_input_grad) else None
        if n > 0:
            a = _args(n, din, C, width, nl - 1, dout, slope, x, cond, weights, biases)
            ws = torch.empty(width, dtype=torch.float32, device=dev) if C > 0 else None
            with _lib.on_device(dev):
                _lib.check(_lib.load().gs_mlp_forward(ctypes.byref(a), _lib.ptr(y), _lib.ptr(acts), _lib.ptr(ws),
                                                      4 * width if C > 0 else 0, _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, cond, acts, *params)
        ctx.meta = (n, din, C, width, nl, dout, slope)
        return y

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        n, din, C, width, nl, dout, slope = ctx.meta
        if g is None or not any(need):
            return (None,) * len(need)
        x, cond, acts = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        weights, biases = params[:nl], params[nl:]
        dev = g.device
        new = torch.zeros if n == 0 else torch.empty
        dx = torch.empty(n, din, dtype=torch.float32, device=dev) if need[0] else None
        dcond = new(C, dtype=torch.float32, device=dev) if (need[1] and C > 0) else None
        dparams = [new(p.shape, dtype=torch.float32, device=dev) if nd else None for p, nd in zip(params, need[3:])]
        if n > 0:
            g = _lib.contiguous_aligned(g.to(torch.float32))
            L = _lib.load()
            a = _args(n, din, C, width, nl - 1, dout, slope, x, cond, weights, biases)
            a.dx, a.dcond = _lib.ptr(dx), _lib.ptr(dcond)
            for l in range(nl):
                a.dW[l], a.db[l] = _lib.ptr(dparams[l]), _lib.ptr(dparams[nl + l])
            ws = torch.empty(_lib.nbytes(L.gs_mlp_workspace_bytes, ctypes.byref(a), 1) // 4, dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                _lib.check(L.gs_mlp_backward(ctypes.byref(a), _lib.ptr(acts), _lib.ptr(g), _lib.ptr(ws), 4 * ws.numel(),
                                             _lib.stream_ptr(dev)))
        return (dx, dcond, None) + tuple(dparams)


def _f32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("fused_mlp: %s: fp32 tensor expected" % name)
    return t


def _cond_row(cond, n):
    """The one row of a condition given as (C,), (1, C) or a stride-0 expand of either; None when its rows may differ."""
    if cond.dim() == 1:
        return cond
    if cond.dim() == 2 and (cond.shape[0] == 1 or (cond.shape[0] == n and cond.stride(0) == 0)):
        return cond[0]
    return None


def fused_mlp(x, weights, biases, cond=None, negative_slope=0.01):
    """y (N, dout) = L_last(leaky(.. leaky(L_0([x | cond])) ..)) as one autograd node: `weights` and `biases` are the
    nn.Linear parameters of the layers in order (1..6 hidden layers of one width, a multiple of 32 up to 128; weights[0]
    (width, din + C) with din <= 512 and C <= 512; dout <= 64); `cond` is ONE row, (C,), (1, C) or an expand of either to
    x's rows, given exactly when weights[0] has more columns than x; LeakyReLU(negative_slope) between the layers, none
    after the last.  Gradients reach x, cond and every parameter that requires one."""
    _f32(x, "x")
    weights, biases = list(weights), list(biases)
    for k, w in enumerate(weights):
        _f32(w, "weights[%d]" % k)
    for k, b in enumerate(biases):
        _f32(b, "biases[%d]" % k)
    if cond is not None:
        _f32(cond, "cond")
    if x.dim() != 2:
        raise ValueError("fused_mlp: x must be (N, din), got %s" % (tuple(x.shape),))
    n, din, nl = int(x.shape[0]), int(x.shape[1]), len(weights)
    if nl < 2 or len(biases) != nl:
        raise ValueError("fused_mlp: one bias per weight and at least two layers expected, got %d and %d" % (nl, len(biases)))
    if any(w.dim() != 2 for w in weights) or any(b.dim() != 1 for b in biases):
        raise ValueError("fused_mlp: weights (out, in) and biases (out,) expected")
    width, dout = int(weights[0].shape[0]), int(weights[-1].shape[0])
    C = int(weights[0].shape[1]) - din
    row = None
    if cond is not None:
        row = _cond_row(cond, n)
        if row is None:
            raise ValueError("fused_mlp: cond must be one row -- (C,), (1, C) or an expand of either -- got %s with strides %s"
                             % (tuple(cond.shape), tuple(cond.stride())))
    if C < 0 or (C > 0) != (row is not None) or (row is not None and int(row.shape[0]) != C):
        raise ValueError("fused_mlp: weights[0] has %d columns: x has %d and cond %s"
                         % (int(weights[0].shape[1]), din, "none" if row is None else int(row.shape[0])))
    for l in range(nl):
        want = (width if l < nl - 1 else dout, din + C if l == 0 else width)
        if tuple(weights[l].shape) != want or tuple(biases[l].shape) != want[:1]:
            raise ValueError("fused_mlp: layer %d must be %s with a bias %s, got %s and %s"
                             % (l, want, want[:1], tuple(weights[l].shape), tuple(biases[l].shape)))
    if not _shapes_ok(din, C, width, nl - 1, dout):
        raise ValueError("fused_mlp: din %d, cond %d, width %d, %d hidden layers, dout %d is outside what the kernels take "
                         "(mlp_supported)" % (din, C, width, nl - 1, dout))
    for t, name in [(x, "x"), (cond, "cond")] + [(w, "weights") for w in weights] + [(b, "biases") for b in biases]:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fused_mlp: %s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)
    return _Fused.apply(x, row, float(negative_slope), *(weights + biases))


def _cfg(config, name, default):
    get = getattr(config, "get", None)
    return get(name, default) if get is not None else getattr(config, name, default)


def _layers(module):
    return [getattr(module, "lin%d" % l) for l in range(int(module.num_layers) - 1)]


def mlp_supported(module):
    """True when the fused kernels take this VanillaCondMLP: no positional encoding (`multires` 0), no skip connections,
    the condition on the first layer or nowhere, LeakyReLU, 1..6 hidden layers of one width (a multiple of 32 up to 128), an
    input of at most 512 columns with a condition of at most 512 (how lin0's columns split between the two is known at the
    call: mlp_forward checks it), at most 64 outputs -- decided from `config`, the activation and the shapes of lin0, lin1,
    .. alone."""
    config = module.config
    cond_in = [int(l) for l in _cfg(config, "cond_in", [])]
    if int(_cfg(config, "multires", 0)) > 0 or len(_cfg(config, "skip_in", [])) or cond_in not in ([], [0]):
        return False
    if not isinstance(module.activation, torch.nn.LeakyReLU):
        return False
    lins = _layers(module)
    if len(lins) < 2:
        return False
    width = lins[0].out_features
    for l, lin in enumerate(lins):
        if lin.bias is None or (l > 0 and lin.in_features != width) or (l < len(lins) - 1 and lin.out_features != width):
            return False
    total = lins[0].in_features  # din + C: how it splits is known at the call (mlp_forward)
    if not (2 <= total <= MAX_IN + MAX_COND if cond_in else 1 <= total <= MAX_IN):
        return False
    return width % 32 == 0 and 32 <= width <= MAX_WIDTH and len(lins) - 1 <= MAX_HIDDEN and 1 <= lins[-1].out_features <= MAX_OUT


def _torch_forward(self, coords, cond):
    """The network as its configuration describes it, layer by layer in torch: the condition joins the input of the layers
    in `cond_in`, the (encoded) coordinates rejoin at the layers in `skip_in` scaled by 1 / sqrt(2)."""
    cond_in = [int(l) for l in _cfg(self.config, "cond_in", [])]
    skip_in = [int(l) for l in _cfg(self.config, "skip_in", [])]
    if cond is not None:
        cond = cond.expand(coords.shape[0], -1)
    embed = getattr(self, "embed_fn", None)
    first = embed(coords) if embed is not None else coords
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


def mlp_forward(self, coords, cond=None):
    """VanillaCondMLP.forward (models/network_utils.py:225-249) through `fused_mlp`; the parameters stay the module's own
    lin0, lin1, ...  A configuration `mlp_supported` turns down goes to the wide kernels where wide_mlp.vanilla_forward
    takes it (device tensors, one condition row, its class switched on), and is evaluated in plain torch otherwise, as is
    a condition whose rows may differ."""
    supported = self.__dict__.get("_gsplat_mlp_supported")
    if supported is None:
        supported = self.__dict__["_gsplat_mlp_supported"] = mlp_supported(self)
    if not supported and coords.is_cuda:
        from . import wide_mlp
        y = wide_mlp.vanilla_forward(self, coords, cond)
        if y is not None:
            return y
    uses_cond = len(_cfg(self.config, "cond_in", [])) > 0
    row = None
    if supported and uses_cond:
        row = _cond_row(cond, int(coords.shape[0])) if (cond is not None and coords.dim() == 2) else None
        supported = row is not None
    if supported:
        lins = _layers(self)
        din = int(coords.shape[-1])
        C = int(row.shape[0]) if row is not None else 0
        supported = lins[0].in_features == din + C and 1 <= din <= MAX_IN and C <= MAX_COND
    if not supported:
        return _torch_forward(self, coords, cond)
    x = coords.reshape(-1, din)
    y = fused_mlp(x, [lin.weight for lin in lins], [lin.bias for lin in lins], cond=row,
                  negative_slope=self.activation.negative_slope)
    return y.reshape(tuple(coords.shape[:-1]) + (y.shape[1],))
