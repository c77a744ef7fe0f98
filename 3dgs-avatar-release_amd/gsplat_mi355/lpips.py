"""The LPIPS-VGG perceptual loss of the avatar model (train.py:28,62-64,127-138; utils/general_utils.py:279-291) on the GPU
through libgsplat_mi355 (csrc/lpips.hip, whose header comment carries the spec): VGG16's thirteen convolutions as implicit
GEMMs on the exact-fp32 MFMA with H and W as run-time arguments, both images through every layer in one launch, a backward
to the images without atomics (bitwise reproducible), without host synchronisation, capture-safe.

* `LPIPS(...)` -- the module behind the `lpips` package of this tree (`import lpips; lpips.LPIPS(net='vgg')`).
* `foreground_box(mask)` -> (y1, y2, x1, x2) as train.py:130-133 computes it.
* `perceptual_loss(loss_fn, image, gt_image, camera)` -- train.py:129-137 in one call, the box cached on the camera.
Nothing of the upstream `lpips` package or of torchvision was available when this was written: the state-dict key names
and the constructor's signature are recalled from the public packages, not checked against them.  Device tensors only:
there is no CPU path.
"""
import collections
import ctypes
import math
import os
import re

import torch

from . import _lib

MIN_SIZE, MAX_SIZE = _lib.GS_LPIPS_MIN_SIZE, _lib.GS_LPIPS_MAX_SIZE
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)  # Cin of layer l, Cout of layer l - 1
TAP_LAYERS = (1, 3, 6, 9, 12)                                                   # relu1_2, 2_2, 3_3, 4_3, 5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)
# (slice, index in torchvision's vgg16().features) of the thirteen convolutions, as lpips's `net.slice{s}.{i}` names them
VGG_INDEX = ((1, 0), (1, 2), (2, 5), (2, 7), (3, 10), (3, 12), (3, 14), (4, 17), (4, 19), (4, 21), (5, 24), (5, 26), (5, 28))
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
WEIGHTS_ENV = "GSPLAT_LPIPS_WEIGHTS"


def trunk_keys():
    return ["net.slice%d.%d" % si for si in VGG_INDEX]


def state_dict_keys():
    """The keys `LPIPS.state_dict()` emits, in order."""
    keys = []
    for k in trunk_keys():
        keys += [k + ".weight", k + ".bias"]
    return ["scaling_layer.shift", "scaling_layer.scale"] + keys + ["lin%d.model.1.weight" % k for k in range(5)]


def random_state_dict(seed=0):
    """He-scaled trunk weights (sigma = sqrt(2 / (9 Cin))), biases of 0.05 sigma, non-negative lin vectors, all from a CPU
    torch.Generator seeded with `seed` (what `pretrained=False` draws)."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = collections.OrderedDict()
    sd["scaling_layer.shift"] = torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1)
    for l, key in enumerate(trunk_keys()):
        cin, cout = CHANNELS[l], CHANNELS[l + 1]
        sigma = math.sqrt(2.0 / (9 * cin))
        sd[key + ".weight"] = torch.randn(cout, cin, 3, 3, generator=gen, dtype=torch.float32) * sigma
        sd[key + ".bias"] = torch.randn(cout, generator=gen, dtype=torch.float32) * (0.05 * sigma)
    for k, c in enumerate(TAP_CHANNELS):
        sd["lin%d.model.1.weight" % k] = torch.rand(1, c, 1, 1, generator=gen, dtype=torch.float32) / c
    return sd


def _ints(key):
    return tuple(int(v) for v in re.findall(r"\d+", key))


def parse_state_dict(sd):
    """A state dict in any accepted spelling -> the canonical one (state_dict_keys).  The trunk is matched by ORDER and
    SHAPE: the 3x3 convolution weights, sorted by the numbers in their names, with the bias of the same prefix -- so
    `net.slice{s}.{i}.weight` (lpips) and `features.{i}.weight` (torchvision's vgg16) both load; the lin vectors are
    `lin{k}.model.1.weight` or `lins.{k}.model.1.weight`, (1, C, 1, 1); `scaling_layer.shift` / `.scale` are optional.
    Every missing or mis-shaped entry is named in the ValueError."""
    problems = []
    out = collections.OrderedDict()
    for name, default in (("shift", SHIFT), ("scale", SCALE)):
        t = sd.get("scaling_layer." + name)
        if t is None:
            t = torch.tensor(default, dtype=torch.float32)
        elif t.numel() != 3:
            problems.append("scaling_layer.%s: 3 values expected, got shape %s" % (name, tuple(t.shape)))
            continue
        out["scaling_layer." + name] = t.detach().to(torch.float32).reshape(1, 3, 1, 1)
    convs = sorted((k for k, t in sd.items() if k.endswith(".weight") and torch.is_tensor(t) and t.dim() == 4
                    and tuple(t.shape[2:]) == (3, 3)), key=_ints)
    if len(convs) != len(VGG_INDEX):
        problems.append("the trunk: %d 3x3 convolution weights expected (net.slice{1..5}.{0,2,5,7,10,12,14,17,19,21,24,26,28}"
                        ".weight or features.N.weight), found %d" % (len(VGG_INDEX), len(convs)))
    else:
        for l, (src, dst) in enumerate(zip(convs, trunk_keys())):
            w, b = sd[src], sd.get(src[:-len("weight")] + "bias")
            want = (CHANNELS[l + 1], CHANNELS[l], 3, 3)
            if tuple(w.shape) != want:
                problems.append("%s: shape %s expected, got %s" % (src, want, tuple(w.shape)))
            if b is None:
                problems.append("%sbias: missing" % src[:-len("weight")])
            elif tuple(b.shape) != want[:1]:
                problems.append("%sbias: shape %s expected, got %s" % (src[:-len("weight")], want[:1], tuple(b.shape)))
            if not problems:
                out[dst + ".weight"] = w.detach().to(torch.float32)
                out[dst + ".bias"] = b.detach().to(torch.float32)
    for k, c in enumerate(TAP_CHANNELS):
        names = ("lin%d.model.1.weight" % k, "lins.%d.model.1.weight" % k)
        t = next((sd[n] for n in names if n in sd), None)
        if t is None:
            problems.append("%s (or %s): missing" % names)
        elif tuple(t.shape) != (1, c, 1, 1):
            problems.append("%s: shape %s expected, got %s" % (names[0], (1, c, 1, 1), tuple(t.shape)))
        else:
            out[names[0]] = t.detach().to(torch.float32)
    if problems:
        raise ValueError("lpips: state dict not usable: " + "; ".join(problems))
    return collections.OrderedDict((k, out[k]) for k in state_dict_keys())


def pack_weights(sd, device):
    """The canonical state dict `sd`, repacked for both directions of the convolution kernel on `device`."""
    L = _lib.load()
    dev = torch.device(device)
    packed = torch.empty(_lib.nbytes(L.gs_lpips_packed_bytes) // 4, dtype=torch.float32, device=dev)
    keep = [t.to(dev, torch.float32).contiguous() for t in sd.values()]
    by = dict(zip(sd.keys(), keep))
    a = _lib.GsLpipsArgs()
    for l, key in enumerate(trunk_keys()):
        a.weight[l], a.bias[l] = by[key + ".weight"].data_ptr(), by[key + ".bias"].data_ptr()
    for k in range(5):
        a.lin[k] = by["lin%d.model.1.weight" % k].data_ptr()
    a.shift, a.scale = by["scaling_layer.shift"].data_ptr(), by["scaling_layer.scale"].data_ptr()
    with _lib.on_device(dev):
        _lib.check(L.gs_lpips_pack_weights(ctypes.byref(a), packed.data_ptr(), 4 * packed.numel(), _lib.stream_ptr(dev)))
    return packed


def _image(t):
    """(tensor the kernels read in place, channel stride, row stride): fp32 with adjacent pixels in a row, else one copy."""
    w = int(t.shape[2])
    if t.dtype != torch.float32 or t.stride(2) != 1 or t.stride(1) < w or t.stride(0) < 1:
        t = t.to(torch.float32).contiguous()
    return t, int(t.stride(0)), int(t.stride(1))


def workspace_bytes(h, w, grad0, grad1, which):
    return _lib.nbytes(_lib.load().gs_lpips_workspace_bytes, int(h), int(w), int(bool(grad0)), int(bool(grad1)), int(which))


class _Fused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, packed, normalize, grad_enabled):
        ctx.set_materialize_grads(False)
        dev, h, w = in0.device, int(in0.shape[1]), int(in0.shape[2])
        # (needs_input_grad says what the inputs require, also under no_grad: the caller passes the grad mode)
        need = tuple(bool(n) and bool(grad_enabled) for n in ctx.needs_input_grad[:2])
        x0, cs0, rs0 = _image(in0.detach())
        x1, cs1, rs1 = _image(in1.detach())
        L = _lib.load()
        a = _lib.GsLpipsArgs()
        a.H, a.W, a.normalize, a.need_grad0, a.need_grad1 = h, w, int(bool(normalize)), int(need[0]), int(need[1])
        a.cs0, a.rs0, a.cs1, a.rs1 = cs0, rs0, cs1, rs1
        a.in0, a.in1, a.packed = x0.data_ptr(), x1.data_ptr(), packed.data_ptr()
        n_saved = workspace_bytes(h, w, need[0], need[1], _lib.GS_LPIPS_WS_SAVED) // 4
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev) if n_saved else None
        ws = torch.empty(workspace_bytes(h, w, need[0], need[1], _lib.GS_LPIPS_WS_FORWARD) // 4, dtype=torch.float32, device=dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)  # the loss, then the five per-tap terms
        with _lib.on_device(dev):
            _lib.check(L.gs_lpips_forward(ctypes.byref(a), out.data_ptr(), out.data_ptr() + 4, _lib.ptr(saved), 4 * n_saved,
                                          ws.data_ptr(), 4 * ws.numel(), _lib.stream_ptr(dev)))
        ctx.save_for_backward(saved, packed)
        ctx.meta = (h, w, int(bool(normalize)), need, in0.dtype, in1.dtype)
        loss, taps = out[:1], out[1:]
        ctx.mark_non_differentiable(taps)
        return loss, taps

    @staticmethod
    def backward(ctx, g, _g_taps):
        h, w, normalize, need, dt0, dt1 = ctx.meta
        if g is None or not any(need):
            return None, None, None, None, None
        saved, packed = ctx.saved_tensors
        dev = g.device
        L = _lib.load()
        a = _lib.GsLpipsArgs()
        a.H, a.W, a.normalize, a.need_grad0, a.need_grad1 = h, w, normalize, int(need[0]), int(need[1])
        a.cs0 = a.cs1 = h * w
        a.rs0 = a.rs1 = w
        a.in0 = a.in1 = a.packed = packed.data_ptr()  # (the backward reads no image: any valid address)
        g = g.detach().to(torch.float32).contiguous()
        d0 = torch.empty(3, h, w, dtype=torch.float32, device=dev) if need[0] else None
        d1 = torch.empty(3, h, w, dtype=torch.float32, device=dev) if need[1] else None
        ws = torch.empty(workspace_bytes(h, w, need[0], need[1], _lib.GS_LPIPS_WS_BACKWARD) // 4, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.gs_lpips_backward(ctypes.byref(a), g.data_ptr(), _lib.ptr(d0), _lib.ptr(d1), saved.data_ptr(),
                                           4 * saved.numel(), ws.data_ptr(), 4 * ws.numel(), _lib.stream_ptr(dev)))
        return (d0.to(dt0) if d0 is not None else None), (d1.to(dt1) if d1 is not None else None), None, None, None


_UNSUPPORTED = (("lpips", True), ("spatial", False), ("pnet_tune", False))


class LPIPS(torch.nn.Module):
    """lpips.LPIPS with the upstream signature (as recalled).  Supported: net='vgg', version='0.1', lpips=True,
    spatial=False, pnet_tune=False; anything else raises NotImplementedError naming the argument.  The weights come from ONE
    local state-dict file (`model_path`, else the environment variable GSPLAT_LPIPS_WEIGHTS; torch.load(weights_only=True)):
    nothing is downloaded.  `pretrained=False` draws seeded random weights (`random_state_dict`).  Always in eval mode."""

    def __init__(self, pretrained=True, net="alex", version="0.1", lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=True):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError("lpips.LPIPS: net=%r is not provided (upstream's default is 'alex'): this package "
                                      "implements net='vgg' only -- pass net='vgg'" % (net,))
        if str(version) != "0.1":
            raise NotImplementedError("lpips.LPIPS: version=%r is not provided: version='0.1' only" % (version,))
        given = dict(lpips=lpips, spatial=spatial, pnet_tune=pnet_tune)
        for name, want in _UNSUPPORTED:
            if bool(given[name]) != want:
                raise NotImplementedError("lpips.LPIPS: %s=%r is not provided: %s=%r only" % (name, given[name], name, want))
        self.pnet_type, self.version, self.pnet_rand, self.use_dropout = net, str(version), bool(pnet_rand), bool(use_dropout)
        self.chns, self.L = list(TAP_CHANNELS), 5
        self._packed = {}
        if pretrained:
            path = model_path or os.environ.get(WEIGHTS_ENV)
            if not path:
                raise FileNotFoundError(
                    "lpips.LPIPS(net='vgg'): no weights file.  Nothing is downloaded: pass model_path=, or set %s, to a state "
                    "dict made elsewhere with the upstream package: torch.save(lpips.LPIPS(net='vgg').state_dict(), path)"
                    % WEIGHTS_ENV)
            if not os.path.exists(path):
                raise FileNotFoundError("lpips.LPIPS(net='vgg'): weights file %r not found (make it with the upstream package: "
                                        "torch.save(lpips.LPIPS(net='vgg').state_dict(), path))" % (path,))
            sd = torch.load(path, map_location="cpu", weights_only=True)
        else:
            sd = random_state_dict(0)
        self._weights = parse_state_dict(sd)
        super().train(False)

    # ---- the weights are plain tensors (frozen: no Parameters), moved with the module and repacked per device on use
    def _apply(self, fn, *args, **kwargs):
        self._weights = collections.OrderedDict((k, fn(t)) for k, t in self._weights.items())
        self._packed = {}
        return super()._apply(fn, *args, **kwargs)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = collections.OrderedDict() if destination is None else destination
        for k, t in self._weights.items():
            out[prefix + k] = t
        return out

    def load_state_dict(self, state_dict, strict=True, assign=False):
        dev = next(iter(self._weights.values())).device
        self._weights = collections.OrderedDict((k, t.to(dev)) for k, t in parse_state_dict(state_dict).items())
        self._packed = {}  # repacked at the next call
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def train(self, mode=True):
        return super().train(False)  # (upstream's eval_mode=True: the dropout in front of the lin layers stays off)

    def packed(self, device):
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._packed:
            self._packed[key] = pack_weights(self._weights, device)
        return self._packed[key]

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        for name, t in (("in0", in0), ("in1", in1)):
            if not torch.is_tensor(t) or not t.is_floating_point():
                raise TypeError("lpips.LPIPS: %s: a floating-point tensor expected" % name)
            if t.dim() not in (3, 4) or t.shape[-3] != 3:
                raise ValueError("lpips.LPIPS: %s must be (3, H, W) or (N, 3, H, W), got %s" % (name, tuple(t.shape)))
        if tuple(in0.shape) != tuple(in1.shape):
            raise ValueError("lpips.LPIPS: in0 %s and in1 %s differ in shape" % (tuple(in0.shape), tuple(in1.shape)))
        h, w = int(in0.shape[-2]), int(in0.shape[-1])
        if not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
            raise ValueError("lpips.LPIPS: images of %d..%d pixels a side are supported, got %d x %d (below %d the last pool "
                             "has nothing left)" % (MIN_SIZE, MAX_SIZE, h, w, MIN_SIZE))
        for name, t in (("in0", in0), ("in1", in1)):
            if not t.is_cuda:
                raise RuntimeError("lpips.LPIPS: %s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)
        if in0.device != in1.device:
            raise RuntimeError("lpips.LPIPS: in0 and in1 live on different devices")
        packed = self.packed(in0.device)
        a, b = (in0[None], in1[None]) if in0.dim() == 3 else (in0, in1)
        vals, taps = [], []
        for n in range(a.shape[0]):
            loss, per_tap = _Fused.apply(a[n], b[n], packed, bool(normalize), torch.is_grad_enabled())
            vals.append(loss)
            taps.append(per_tap)
        val = torch.cat(vals).reshape(-1, 1, 1, 1)
        if retPerLayer:
            per = torch.stack(taps)  # (N, 5)
            return val, [per[:, k].reshape(-1, 1, 1, 1) for k in range(5)]
        return val

    def extra_repr(self):
        return "net='vgg', version='0.1', fp32 on the matrix unit, fixed-order sums"


def foreground_box(mask):
    """(y1, y2, x1, x2) of the mask's non-zero pixels, as train.py:130-133 computes it: `mask` is (1, H, W) (or (H, W)); rows
    y1:y2 and columns x1:x2 hold every non-zero pixel.  One device-to-host copy when the mask lives on the GPU."""
    import numpy as np
    m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3:
        raise ValueError("foreground_box: mask must be (1, H, W) or (H, W), got %s" % (tuple(m.shape),))
    idx = np.where(m)
    if idx[0].size == 0:
        raise ValueError("foreground_box: the mask is empty")
    return int(idx[1].min()), int(idx[1].max()) + 1, int(idx[2].min()), int(idx[2].max()) + 1


_BOX_ATTR = "_gsplat_foreground_box"


def perceptual_loss(loss_fn, image, gt_image, camera):
    """train.py:129-137 in one call: crop `image` and `gt_image` (3, H, W) to the foreground of `camera.original_mask` and
    return loss_fn(crop, gt_crop, normalize=True).mean().  The box is computed ONCE per camera object and kept on it
    (`camera._gsplat_foreground_box`): later steps make no device-to-host copy.  The crops are views; the image's gradient
    comes back through autograd's own slice backward."""
    box = getattr(camera, _BOX_ATTR, None)
    if box is None:
        box = foreground_box(camera.original_mask)
        setattr(camera, _BOX_ATTR, box)
    y1, y2, x1, x2 = box
    return loss_fn(image[:, y1:y2, x1:x2], gt_image[:, y1:y2, x1:x2], normalize=True).mean()
