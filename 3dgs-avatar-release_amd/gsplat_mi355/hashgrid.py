"""Multiresolution hash-grid encoding (tcnn.Encoding(3, {"otype": "HashGrid", ...}) of the reference's non-rigid deformer,
models/network_utils.py:329-343) on the GPU through libgsplat_mi355 (csrc/hashgrid.hip, whose header comment carries the
spec).  fp32 parameters and arithmetic; the parameter gradient is written without atomics and is bitwise reproducible;
nothing in either direction waits for the GPU, and both directions are kernel launches only (graph-capturable).

`parse_config` reads a tcnn encoding config, `levels` returns the level table from the library (the one source of truth
for offsets, scales and resolutions), `hashgrid_encode` is the autograd function (x, params) -> (N, L F) and
`HashGridEncoding` the module.  There is no CPU path: CPU tensors raise.
"""
import ctypes

import torch

from . import _lib

DEFAULTS = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
            "per_level_scale": 2.0, "interpolation": "Linear", "hash": "CoherentPrime"}


def parse_config(n_input_dims, config):
    """A tcnn encoding config -> a dict of the five numeric keys (tcnn's defaults where absent).  Unknown keys are
    ignored.  A config without `otype` is taken to be a HashGrid: the reference's `hashgrid:` block has none, and its
    class name, its "max reso" comment and the MLP sized by n_output_dims all say that is what is meant.  Accepted:
    otype "HashGrid", or "Grid" with type "Hash" (case-insensitive); anything else raises NotImplementedError naming the
    key."""
    config = dict(config or {})
    if int(n_input_dims) != 3:
        raise NotImplementedError("hashgrid: n_input_dims = %r; only 3-D input is supported" % (n_input_dims,))
    otype = config.get("otype", "HashGrid")
    if str(otype).lower() == "grid":
        gtype = config.get("type", "Hash")
        if str(gtype).lower() != "hash":
            raise NotImplementedError("hashgrid: type = %r; only 'Hash' grids are supported" % (gtype,))
    elif str(otype).lower() != "hashgrid":
        raise NotImplementedError("hashgrid: otype = %r; only 'HashGrid' (or 'Grid' with type 'Hash') is supported" % (otype,))
    interp = config.get("interpolation", DEFAULTS["interpolation"])
    if str(interp).lower() != "linear":
        raise NotImplementedError("hashgrid: interpolation = %r; only 'Linear' is supported" % (interp,))
    hsh = config.get("hash", DEFAULTS["hash"])
    if str(hsh).lower() != "coherentprime":
        raise NotImplementedError("hashgrid: hash = %r; only 'CoherentPrime' is supported" % (hsh,))
    out = {k: config.get(k, DEFAULTS[k]) for k in ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution",
                                                    "per_level_scale")}
    if int(out["n_features_per_level"]) not in (1, 2, 4, 8):
        raise NotImplementedError("hashgrid: n_features_per_level = %r; 1, 2, 4 or 8 are supported"
                                  % (out["n_features_per_level"],))
    for k in ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution"):
        out[k] = int(out[k])
    out["per_level_scale"] = float(out["per_level_scale"])
    return out


def grid_struct(cfg):
    return _lib.GsHashGrid(n_levels=cfg["n_levels"], n_features_per_level=cfg["n_features_per_level"],
                           log2_hashmap_size=cfg["log2_hashmap_size"], base_resolution=cfg["base_resolution"],
                           per_level_scale=cfg["per_level_scale"])


def levels(cfg):
    """(offsets [L + 1] in rows of F, scales [L] float32 values, resolutions [L], n_params) from gs_hashgrid_levels."""
    key = tuple(cfg[k] for k in ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution", "per_level_scale"))
    hit = _levels_memo.get(key)
    if hit is None:
        hit = _levels_memo[key] = _levels(cfg)
    return hit


_levels_memo = {}


def _levels(cfg):
    L = int(cfg["n_levels"])
    if L < 1 or L > _lib.GS_HASHGRID_MAX_LEVELS:
        raise ValueError("hashgrid: n_levels = %d outside 1 .. %d" % (L, _lib.GS_HASHGRID_MAX_LEVELS))
    offsets = (ctypes.c_int32 * (L + 1))()
    scales = (ctypes.c_float * L)()
    res = (ctypes.c_int32 * L)()
    n = ctypes.c_int32(0)
    g = grid_struct(cfg)
    rc = _lib.load().gs_hashgrid_levels(ctypes.byref(g), offsets, scales, res, ctypes.byref(n))
    if rc != 0:
        raise ValueError("hashgrid: config %r rejected: %s" % (cfg, _lib.load().gs_status_string(rc).decode()))
    return tuple(offsets), tuple(float(s) for s in scales), tuple(res), int(n.value)


class _HashGridFunction(torch.autograd.Function):
    """(x [N, 3] fp32 contiguous, params [n_params] fp32) -> out [N, L F] fp32."""

    @staticmethod
    def forward(ctx, x, params, grid, n_out):
        dev = x.device
        N = int(x.shape[0])
        out = torch.empty((N, n_out), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().gs_hashgrid_forward(ctypes.byref(grid), N, _lib.ptr(x), _lib.ptr(params), _lib.ptr(out),
                                                       _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, params)
        ctx.grid = grid
        return out

    @staticmethod
    def backward(ctx, g):
        x, params = ctx.saved_tensors
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (want_x or want_p):
            return None, None, None, None
        dev = x.device
        N = int(x.shape[0])
        L = _lib.load()
        g = _lib.contiguous_aligned(g.to(torch.float32))
        dx = torch.empty_like(x) if want_x else None
        dp = torch.empty_like(params) if want_p else None
        ws = None
        if want_p:
            ws = torch.empty(_lib.nbytes(L.gs_hashgrid_workspace_bytes, ctypes.byref(ctx.grid), N), dtype=torch.uint8,
                             device=dev)
        with _lib.on_device(dev):
            _lib.check(L.gs_hashgrid_backward(ctypes.byref(ctx.grid), N, _lib.ptr(x), _lib.ptr(params), _lib.ptr(g),
                                              _lib.ptr(dx), _lib.ptr(dp), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                              _lib.stream_ptr(dev)))
        return dx, dp, None, None


def hashgrid_encode(x, params, cfg):
    """out [N, L F] fp32 = the encoding of x [N, 3] (any float dtype and strides: the gradient returns in x's dtype) with
    the flat fp32 table `params` [n_params]."""
    if not x.is_cuda or not params.is_cuda:
        raise RuntimeError("hashgrid: x and params must live on the GPU (no CPU fallback)")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("hashgrid: x must be (N, 3), got %s" % (tuple(x.shape),))
    if params.dtype != torch.float32 or params.dim() != 1:
        raise TypeError("hashgrid: params must be a flat fp32 tensor")
    if x.device != params.device:
        raise ValueError("hashgrid: x is on %s, params on %s" % (x.device, params.device))
    if not x.is_floating_point():
        raise TypeError("hashgrid: x must be a floating-point tensor")
    _, _, _, n_params = levels(cfg)
    if params.numel() != n_params:
        raise ValueError("hashgrid: params has %d elements, the config needs %d" % (params.numel(), n_params))
    xf = x.to(torch.float32).contiguous()
    pf = _lib.contiguous_aligned(params)
    n_out = cfg["n_levels"] * cfg["n_features_per_level"]
    return _HashGridFunction.apply(xf, pf, grid_struct(cfg), n_out)


class HashGridEncoding(torch.nn.Module):
    """The encoding as a module: one flat fp32 parameter `params`, uniform in [-1e-4, 1e-4] from a CPU generator seeded
    with `seed`.  forward(x [N, 3]) -> [N, L F] fp32."""

    def __init__(self, config, seed=1337, n_input_dims=3):
        super().__init__()
        self.cfg = parse_config(n_input_dims, config)
        self.n_input_dims = 3
        self.n_output_dims = self.cfg["n_levels"] * self.cfg["n_features_per_level"]
        _, _, _, n_params = levels(self.cfg)
        gen = torch.Generator().manual_seed(int(seed))
        init = torch.empty(n_params, dtype=torch.float32).uniform_(-1e-4, 1e-4, generator=gen)
        self.params = torch.nn.Parameter(init)

    def forward(self, x):
        return hashgrid_encode(x, self.params, self.cfg)
