"""The reference's densification cycle, fused (scene/gaussian_model.py:263-266,311-462, called at train.py:217-227):
clone, split and prune with the Adam-state surgery, `prune_points` alone, and `reset_opacity`.

The reference runs each of these as boolean-mask indexing, `torch.cat` and `torch.normal` over 18 tensors -- a `nonzero()`
with a host sync per masked index.  Here a cycle is three small launches that classify the Gaussians and build a
destination -> source map (csrc/densify.hip; the full semantics are written out at its top), ONE read of the new count
N' (the cycle's only host sync), and ONE launch that writes all 21 output tensors (6 parameters, 12 Adam moments, 3
statistics) by destination row.

The optimizer surgery works on `torch.optim.Adam` and `FusedAdam` alike (same state layout): each group's parameter
becomes a new `nn.Parameter` in `group["params"][0]`, its state dict moves to the new key with `exp_avg` / `exp_avg_sq`
replaced and `step` untouched; a group without state gets none.

`torch.cuda.empty_cache()`, which the reference calls at the end of densify_and_prune (scene/gaussian_model.py:462), is
deliberately NOT called: it hands the allocator's cached blocks back to the driver and makes the next steps allocate
them again (and it is a device-wide synchronisation).
GPU fp32 tensors only.
"""
import ctypes

import torch

from . import _lib

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
_KIND = {"xyz": _lib.GS_DENSIFY_CHILD_POSITION, "scaling": _lib.GS_DENSIFY_CHILD_SCALING}

_pinned = {}  # device index -> pinned int32 word for the count


def _check(t, name, n=None):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("gsplat_mi355.densify: %s must be a contiguous fp32 GPU tensor" % name)
    if n is not None and (t.dim() == 0 or t.shape[0] != n):
        raise ValueError("gsplat_mi355.densify: %s has %s rows, expected %d" % (name, tuple(t.shape), n))


class Plan(object):
    """The result of the classification: `n_new` rows after the cycle, `flags` (uint8 [N], GS_DENSIFY_F_* bits) and the
    workspace the apply step reads."""

    def __init__(self, n, n_new, ws, prune_only):
        self.n, self.n_new, self.ws, self.prune_only = n, n_new, ws, prune_only

    @property
    def flags(self):
        return self.ws[:self.n]

    @staticmethod
    def map_offset(n, ws_bytes):
        """Byte offset of the row map in a workspace of `ws_bytes` for N = n: it is the last region, u32[2 N] padded to
        256 bytes (csrc/densify.hip dn_carve)."""
        return ws_bytes - ((2 * n * 4 + 255) & ~255)

    def row_map(self):
        """The plan's destination -> source map as (src, slot), int64 [n_new] each (slot 0 original, 1 clone, 2 / 3 first /
        second child): what apply_plan will gather by."""
        off = self.map_offset(self.n, self.ws.numel())
        m = self.ws[off:off + 4 * self.n_new].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return m & 0x3FFFFFFF, m >> 30

    def masks(self):
        """The reference's selection masks over the N sources: clone, split, and `keep` (the original row survives)."""
        f = self.flags.to(torch.int32)
        return {"clone": (f & _lib.GS_DENSIFY_F_CLONE) != 0, "split": (f & _lib.GS_DENSIFY_F_SPLIT) != 0,
                "keep": (f & _lib.GS_DENSIFY_F_KEEP) != 0, "prune": (f & _lib.GS_DENSIFY_F_PRUNE) != 0,
                "child_prune": (f & _lib.GS_DENSIFY_F_CHILD_PRUNE) != 0}


def _run_plan(dev, n, p):
    L = _lib.load()
    ws = torch.empty(_lib.nbytes(L.gs_densify_workspace_bytes, n), dtype=torch.uint8, device=dev)
    cnt = _pinned.get(dev.index)
    if cnt is None:
        cnt = _pinned[dev.index] = torch.zeros(1, dtype=torch.int32, pin_memory=True)
    with _lib.on_device(dev):
        _lib.check(L.gs_densify_plan(ctypes.byref(p), ws.data_ptr(), ws.numel(), cnt.data_ptr(), _lib.stream_ptr(dev)))
        torch.cuda.current_stream(dev).synchronize()  # the cycle's one host sync: N' sizes every output
    return ws, int(cnt[0])


def plan_densify(params, stats, *, grad_threshold, percent_dense, extent, min_opacity, max_screen_size=None):
    """Classification of densify_and_prune (no tensor is changed).  Thresholds are formed as the reference forms them,
    in double, and rounded to fp32 once, as torch does when it compares an fp32 tensor with a Python float."""
    xyz = params["xyz"]
    n = int(xyz.shape[0])
    scaling, opacity = params["scaling"], params["opacity"]
    accum, denom = stats["xyz_gradient_accum"], stats["denom"]
    for t, name in ((scaling, "scaling"), (opacity, "opacity"), (accum, "xyz_gradient_accum"), (denom, "denom")):
        _check(t, name, n)
    p = _lib.GsDensifyPlan(N=n, scaling=_lib.ptr(scaling), opacity=_lib.ptr(opacity), grad_accum=_lib.ptr(accum),
                           denom=_lib.ptr(denom), prune_mask=None, grad_threshold=float(grad_threshold),
                           split_scale=percent_dense * extent, min_opacity=float(min_opacity), max_world_scale=0.1 * extent,
                           max_screen_size=float(max_screen_size or 0.0), prune_size=1 if max_screen_size else 0)
    ws, n_new = _run_plan(xyz.device, n, p)
    return Plan(n, n_new, ws, prune_only=False)


def plan_prune(params, mask):
    """Classification of prune_points(mask): rows where `mask` is True go, nothing is added."""
    xyz = params["xyz"]
    n = int(xyz.shape[0])
    if mask.dtype != torch.bool or mask.numel() != n or not mask.is_cuda:
        raise ValueError("gsplat_mi355.densify: the prune mask must be a bool GPU tensor of N = %d elements" % n)
    m = mask.reshape(-1).contiguous().view(torch.uint8)
    p = _lib.GsDensifyPlan(N=n, prune_mask=_lib.ptr(m))
    ws, n_new = _run_plan(xyz.device, n, p)
    return Plan(n, n_new, ws, prune_only=True)


def _groups_by_name(optimizer, params):
    if optimizer is None:
        return {}
    out = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name not in params:
            raise KeyError("gsplat_mi355.densify: optimizer group %r is not among the parameters %s" % (name, sorted(params)))
        if len(group["params"]) != 1 or group["params"][0] is not params[name]:
            raise ValueError("gsplat_mi355.densify: optimizer group %r does not hold params[%r]" % (name, name))
        out[name] = group
    return out


def _install(optimizer, groups, name, new_param, moments):
    """Moves the group's state to `new_param` with the moments replaced (the reference's *_to_optimizer helpers)."""
    group = groups.get(name)
    if group is None:
        return
    old = group["params"][0]
    st = optimizer.state.get(old, None)
    if st is not None:
        st["exp_avg"], st["exp_avg_sq"] = moments
        del optimizer.state[old]
    group["params"][0] = new_param
    if st is not None:
        optimizer.state[new_param] = st


def apply_plan(plan, params, optimizer, stats, noise=None):
    """Writes the cycle a plan describes: returns (new params, new stats) and updates `optimizer` (may be None)."""
    xyz = params["xyz"]
    dev, n, n_new = xyz.device, plan.n, plan.n_new
    groups = _groups_by_name(optimizer, params)
    jobs, out_params, out_moments, out_stats = [], {}, {}, {}

    def add(src, kind, name):
        _check(src, name, n)
        dst = torch.empty((n_new,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        width = 1
        for d in src.shape[1:]:
            width *= int(d)
        jobs.append(_lib.GsDensifyTensor(_lib.ptr(src) if n else None, dst.data_ptr() if n_new else None, width, kind))
        return dst

    for name in GROUPS:
        kind = _lib.GS_DENSIFY_COPY if plan.prune_only else _KIND.get(name, _lib.GS_DENSIFY_COPY)
        out_params[name] = add(params[name], kind, name)
        group = groups.get(name)
        st = optimizer.state.get(group["params"][0], None) if group is not None else None
        if st is not None and "exp_avg" in st:
            out_moments[name] = (add(st["exp_avg"], _lib.GS_DENSIFY_ZERO_IF_NEW, name + ".exp_avg"),
                                 add(st["exp_avg_sq"], _lib.GS_DENSIFY_ZERO_IF_NEW, name + ".exp_avg_sq"))
    for name in STATS:
        out_stats[name] = add(stats[name], _lib.GS_DENSIFY_COPY if plan.prune_only else _lib.GS_DENSIFY_ZERO, name)
    scaling, rotation = params["scaling"], params["rotation"]
    _check(rotation, "rotation", n)
    if not plan.prune_only and n > 0:
        if noise is None:
            noise = torch.randn((n, 2, 3), device=dev)
        _check(noise, "noise", n)
        if tuple(noise.shape) != (n, 2, 3):
            raise ValueError("gsplat_mi355.densify: noise must be (N, 2, 3)")
    L = _lib.load()
    arr = (_lib.GsDensifyTensor * len(jobs))(*jobs)
    with _lib.on_device(dev):
        _lib.check(L.gs_densify_apply(n, n_new, plan.ws.data_ptr(), plan.ws.numel(), len(jobs), arr, _lib.ptr(scaling),
                                      _lib.ptr(rotation), None if plan.prune_only else _lib.ptr(noise),
                                      _lib.stream_ptr(dev)))
    new_params = {}
    for name in GROUPS:
        p = torch.nn.Parameter(out_params[name], requires_grad=True)
        new_params[name] = p
        _install(optimizer, groups, name, p, out_moments.get(name))
    return new_params, out_stats


def densify_and_prune(params, optimizer, stats, *, grad_threshold, percent_dense, extent, min_opacity,
                      max_screen_size=None, noise=None):
    """GaussianModel.densify_and_prune on raw parameters (`params`: dict keyed xyz, f_dc, f_rest, opacity, scaling,
    rotation), their optimizer (torch.optim.Adam or FusedAdam, groups named as the reference names them; may be None) and
    the statistics (`stats`: xyz_gradient_accum [N,1], denom [N,1], max_radii2D [N]).  `noise`: the split children's
    standard-normal draws, (N, 2, 3) indexed by source and copy; drawn with torch.randn when None.
    Returns (new params: nn.Parameters, new stats: zeros of the new N)."""
    plan = plan_densify(params, stats, grad_threshold=grad_threshold, percent_dense=percent_dense, extent=extent,
                        min_opacity=min_opacity, max_screen_size=max_screen_size)
    return apply_plan(plan, params, optimizer, stats, noise)


def prune_points(params, optimizer, stats, mask):
    """GaussianModel.prune_points(mask): the rows where `mask` is True go from parameters, moments and statistics."""
    return apply_plan(plan_prune(params, mask), params, optimizer, stats)


def reset_opacity(params, optimizer):
    """GaussianModel.reset_opacity: opacity = logit(min(sigmoid(opacity), 0.01)) as a new nn.Parameter, its moments
    zeroed (new tensors), `step` kept.  Returns the new params dict."""
    op = params["opacity"]
    _check(op, "opacity")
    groups = _groups_by_name(optimizer, params)
    new = torch.empty_like(op)
    group = groups.get("opacity")
    st = optimizer.state.get(group["params"][0], None) if group is not None else None
    moments = (torch.empty_like(op), torch.empty_like(op)) if st is not None else None
    L = _lib.load()
    with _lib.on_device(op.device):
        _lib.check(L.gs_reset_opacity(op.numel(), _lib.ptr(op), _lib.ptr(new), _lib.ptr(moments[0]) if moments else None,
                                      _lib.ptr(moments[1]) if moments else None, _lib.stream_ptr(op.device)))
    p = torch.nn.Parameter(new, requires_grad=True)
    _install(optimizer, groups, "opacity", p, moments)
    out = dict(params)
    out["opacity"] = p
    return out


_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}


class ModelDensifier(object):
    """The three methods on an object with the reference GaussianModel's attribute names (`_xyz` ... `_rotation`,
    `optimizer`, `percent_dense`, `xyz_gradient_accum`, `denom`, `max_radii2D`), updating it as the reference's own
    methods do.  train.py:224 / :227 become `ModelDensifier(gaussians).densify_and_prune(opt, scene, size_threshold)` /
    `ModelDensifier(gaussians).reset_opacity()`."""

    def __init__(self, model):
        self.model = model

    def _params(self):
        return {k: getattr(self.model, a) for k, a in _ATTR.items()}

    def _stats(self):
        return {k: getattr(self.model, k) for k in STATS}

    def _store(self, params, stats=None):
        for k, a in _ATTR.items():
            setattr(self.model, a, params[k])
        for k, v in (stats or {}).items():
            setattr(self.model, k, v)

    def densify_and_prune(self, opt, scene, max_screen_size, noise=None):
        m = self.model
        params, stats = densify_and_prune(self._params(), m.optimizer, self._stats(), grad_threshold=opt.densify_grad_threshold,
                                          percent_dense=m.percent_dense, extent=scene.cameras_extent,
                                          min_opacity=opt.opacity_threshold, max_screen_size=max_screen_size, noise=noise)
        self._store(params, stats)

    def prune_points(self, mask):
        params, stats = prune_points(self._params(), self.model.optimizer, self._stats(), mask)
        self._store(params, stats)

    def reset_opacity(self):
        self._store(reset_opacity(self._params(), self.model.optimizer))
