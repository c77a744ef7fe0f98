"""Training-step bookkeeping after the backward pass, fused.

* `FusedAdam` -- a drop-in for the `torch.optim.Adam(l, lr=0.0, eps=1e-15)` the reference builds over its six
  parameter groups (scene/gaussian_model.py:201-216): same constructor arguments, same `param_groups`, same state
  keys (`step`, `exp_avg`, `exp_avg_sq`) -- the reference's densification code edits those state tensors directly
  (scene/gaussian_model.py: cat_tensors_to_optimizer / _prune_optimizer) -- but `step()` is ONE kernel launch
  for all parameters.
  With `weight_decay`, `max_grad_norm` or `capturable=True` it is the converter's optimizer too
  (models/gaussian_converter.py:22-39: six groups, ~130 tensors, weight decay on the two latent groups): the global
  gradient norm, the clip and the update in a handful of launches with no host synchronisation, and with
  `capturable=True` a step that `torch.cuda.graph` can capture.
* `clip_grad_norm_` -- `torch.nn.utils.clip_grad_norm_` (2-norm) with a deterministic norm: the same gradients give
  the same bits on every run.
* `converter_optimize` -- `GaussianConverter.optimize` (models/gaussian_converter.py:61-67) on the two above.
* `densify_stats` -- train.py:219-220 + scene/gaussian_model.py:464-466 in one kernel, without the boolean-mask
  indexing (and its host sync) of the torch formulation.
GPU fp32 tensors only.
"""
import ctypes

import torch

from . import _lib


def densify_stats(radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom):
    """In place, for Gaussians with radii > 0: max_radii2D = max(max_radii2D, radii);
    xyz_gradient_accum += |viewspace_grad[:, :2]|; denom += 1."""
    n = int(radii.shape[0])
    for t, name in ((viewspace_grad, "viewspace_grad"), (max_radii2D, "max_radii2D"),
                    (xyz_gradient_accum, "xyz_gradient_accum"), (denom, "denom")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("densify_stats: %s must be a contiguous fp32 GPU tensor" % name)
    if radii.dtype != torch.int32 or not radii.is_cuda or not radii.is_contiguous():
        raise RuntimeError("densify_stats: radii must be a contiguous int32 GPU tensor")
    if tuple(viewspace_grad.shape) != (n, 3) or max_radii2D.numel() != n or xyz_gradient_accum.numel() != n or denom.numel() != n:
        raise ValueError("densify_stats: shapes do not match N = %d" % n)
    L = _lib.load()
    with _lib.on_device(radii.device):
        sptr = _lib.stream_ptr(radii.device)
        _lib.check(L.gs_densify_stats(n, _lib.ptr(radii), _lib.ptr(viewspace_grad), _lib.ptr(max_radii2D),
                                      _lib.ptr(xyz_gradient_accum), _lib.ptr(denom), sptr))
    _bump_versions(max_radii2D, xyz_gradient_accum, denom)


def _bump_versions(*tensors):
    """The HIP kernels write through raw pointers, which torch cannot see: bump the autograd version counters as any
    in-place torch op would, so that whatever keys on them (saved-tensor checks, the rasterizer's shared-geometry
    matching) sees the write."""
    torch.autograd.graph.increment_version(tensors)


def _grad_table(grads):
    arr = (_lib.GsGradTensor * len(grads))()
    for k, g in enumerate(grads):
        arr[k] = _lib.GsGradTensor(g.data_ptr(), g.numel())
    return arr


def _grad_norm(L, grads, max_norm, out, workspace):
    """Enqueues the global norm of `grads` (one device, checked by the caller): out[0] = total_norm, out[1] = clip_coef.
    Returns the workspace it used (`workspace` itself, or a larger one)."""
    dev = out.device
    arr = _grad_table(grads)
    need = _lib.nbytes(L.gs_grad_norm_workspace_bytes, len(grads), arr)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.gs_grad_norm(len(grads), arr, float(max_norm), out.data_ptr(), workspace.data_ptr(),
                                  workspace.numel() * 4, _lib.stream_ptr(dev)))
    return workspace, arr


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """`torch.nn.utils.clip_grad_norm_` for contiguous fp32 GPU gradients: the gradients are scaled in place by
    min(max_norm / (total_norm + 1e-6), 1) and the total norm is returned as a 0-dim device tensor, without a host
    synchronisation (unless `error_if_nonfinite`).  The norm is summed in a fixed order: same gradients, same bits.
    `foreach` is accepted and ignored (there is one path)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_: only norm_type=2 is implemented")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if len(grads) == 0:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
            raise RuntimeError("clip_grad_norm_: contiguous fp32 GPU gradients expected")
        if g.device != dev:
            raise RuntimeError("clip_grad_norm_: all gradients must be on one device")
    if len(grads) > _lib.GS_OPTIM_MAX_TENSORS:
        raise RuntimeError("clip_grad_norm_: more than %d tensors" % _lib.GS_OPTIM_MAX_TENSORS)
    if error_if_nonfinite and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("clip_grad_norm_: error_if_nonfinite reads the norm on the host, which a stream capture cannot do")
    L = _lib.load()
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _ws, arr = _grad_norm(L, grads, max_norm, out, None)
    total_norm = out[0]
    if error_if_nonfinite and not bool(torch.isfinite(total_norm)):
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    with _lib.on_device(dev):
        _lib.check(L.gs_grad_scale(len(grads), arr, out[1:].data_ptr(), _lib.stream_ptr(dev)))
    _bump_versions(*grads)
    return total_norm


def converter_optimize(self):
    """`GaussianConverter.optimize` (models/gaussian_converter.py:61-67): clip to cfg.opt.grad_clip, step, zero_grad,
    scheduler step.  With a `FusedAdam` as `self.optimizer` the clip happens inside the fused step (the gradients are
    left unscaled; zero_grad drops them next); with any other optimizer this is the reference's sequence."""
    grad_clip = self.cfg.opt.get('grad_clip', 0.)
    if isinstance(self.optimizer, FusedAdam):
        self.optimizer.step(max_grad_norm=grad_clip if grad_clip > 0 else None)
    else:
        if grad_clip > 0:
            torch.nn.utils.clip_grad_norm_(self.parameters(), grad_clip)
        self.optimizer.step()
    self.optimizer.zero_grad()
    self.scheduler.step()


_UNSET = object()


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (betas, eps, per-group lr and weight decay; no amsgrad, no maximize) with a fused `step()`.
    State layout identical to torch.optim.Adam's (`step` tensor, `exp_avg`, `exp_avg_sq`).

    * With every new argument at its default, `step()` is ONE `gs_adam_step` launch per 16 tensors that share a step number.
    * `max_grad_norm`: `step()` first takes the global 2-norm of all gradients (`self.total_norm`, a 0-dim device tensor)
      and applies min(max_grad_norm / (total_norm + 1e-6), 1) inside the update.  THE GRADIENTS ARE LEFT UNSCALED -- the
      one difference from `clip_grad_norm_` + `step()`, which scales them in place.
    * `capturable=True`: the `step` state entries are 0-dim fp32 device tensors and `group["lr"]` may be one, as in torch;
      `step()` then reads nothing on the host and can be captured by `torch.cuda.graph`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, capturable=False,
                 max_grad_norm=None):
        if amsgrad:
            raise NotImplementedError("FusedAdam: amsgrad is not used by the reference and not implemented")
        if not weight_decay >= 0:
            raise ValueError("FusedAdam: invalid weight_decay %r" % (weight_decay,))
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError("FusedAdam: invalid max_grad_norm %r" % (max_grad_norm,))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      capturable=bool(capturable)))
        self.max_grad_norm = max_grad_norm
        self.total_norm = None   # 0-dim device tensor after a step with max_grad_norm
        self._clip_out = None    # device float[2]: total_norm, clip_coef
        self._clip_ws = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("capturable", False)
        for name in ("max_grad_norm", "total_norm", "_clip_out", "_clip_ws"):
            self.__dict__.setdefault(name, None)

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_UNSET):
        """`max_grad_norm` overrides the constructor's for this call (None: no clipping)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_grad_norm is _UNSET:
            max_grad_norm = self.max_grad_norm
        plain = max_grad_norm is None
        for group in self.param_groups:
            if group.get("amsgrad", False) or group.get("maximize", False):
                raise NotImplementedError("FusedAdam: amsgrad / maximize are not implemented")
            if group["weight_decay"] != 0 or group.get("capturable", False) or isinstance(group["lr"], torch.Tensor):
                plain = False
        if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing() and \
                not all(g.get("capturable", False) for g in self.param_groups):
            raise RuntimeError("FusedAdam: step() under stream capture needs capturable=True (with a host-side step number a "
                               "replay would repeat the captured step's bias correction); nothing was enqueued")
        L = _lib.load()
        if plain:
            self._step_plain(L)
        else:
            self._step_ex(L, max_grad_norm)
        return loss

    def _step_plain(self, L):
        # tensors that share (betas, eps, step number, device) go into one launch
        batches = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: contiguous fp32 GPU parameters expected")
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam: sparse gradients are not supported")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                step = int(st["step"].item()) if st["step"].device.type == "cpu" else int(st["step"])
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                key = (float(b1), float(b2), float(group["eps"]), step, p.device.index)
                batches.setdefault(key, []).append((p, g, st["exp_avg"], st["exp_avg_sq"], float(group["lr"])))
        for (b1, b2, eps, step, dev_index), items in batches.items():
            dev = torch.device("cuda", dev_index)
            for i in range(0, len(items), _lib.GS_ADAM_MAX_TENSORS):
                chunk = items[i:i + _lib.GS_ADAM_MAX_TENSORS]
                arr = (_lib.GsAdamTensor * len(chunk))()
                for k, (p, g, m, v, lr) in enumerate(chunk):
                    arr[k] = _lib.GsAdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr)
                with _lib.on_device(dev):
                    sptr = _lib.stream_ptr(dev)
                    _lib.check(L.gs_adam_step(len(chunk), arr, b1, b2, eps, step, sptr))
                for p, _g, m, v, _lr in chunk:
                    _bump_versions(p, m, v)

    def _step_ex(self, L, max_grad_norm):
        """Clip coefficient, weight decay, device-resident step numbers and learning rates: gs_grad_norm + gs_adam_step_ex."""
        # tensors that share (betas, eps, host step number or 0 for a device one, device) go into one call
        batches = {}
        grads = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            capturable = bool(group.get("capturable", False))
            lr, lr_dev = group["lr"], None
            if isinstance(lr, torch.Tensor):
                if lr.is_cuda:
                    if lr.dtype != torch.float32 or lr.numel() != 1:
                        raise RuntimeError("FusedAdam: a tensor lr must hold one fp32 value")
                    lr_dev, lr = lr.data_ptr(), 0.0
                elif capturable:
                    raise RuntimeError("FusedAdam: with capturable=True a tensor lr must be on the device")
            wd = float(group["weight_decay"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: contiguous fp32 GPU parameters expected")
                if g.is_sparse:
                    raise RuntimeError("FusedAdam: sparse gradients are not supported")
                if lr_dev is not None and group["lr"].device != p.device:
                    raise RuntimeError("FusedAdam: a tensor lr must be on its parameters' device")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else \
                        torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if capturable:
                    s = st["step"]
                    if s.device != p.device or s.dtype != torch.float32 or s.numel() != 1:
                        # (a state loaded from a non-capturable optimizer: moved once, outside any capture)
                        s = st["step"] = s.to(device=p.device, dtype=torch.float32).reshape(())
                    step, step_dev = 0, s.data_ptr()
                else:
                    st["step"] += 1
                    step, step_dev = int(st["step"].item()), None
                if not g.is_contiguous():
                    g = g.contiguous()
                grads.append(g)
                key = (float(b1), float(b2), float(group["eps"]), step, p.device.index)
                batches.setdefault(key, []).append(
                    (_lib.GsAdamTensorEx(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                         p.numel(), float(lr), wd, step_dev, lr_dev), p, st))
        if not grads:
            return
        coef = None
        if max_grad_norm is not None:
            dev = grads[0].device
            if any(g.device != dev for g in grads):
                raise RuntimeError("FusedAdam: max_grad_norm needs all parameters on one device")
            if len(grads) > _lib.GS_OPTIM_MAX_TENSORS:
                raise RuntimeError("FusedAdam: max_grad_norm over more than %d tensors" % _lib.GS_OPTIM_MAX_TENSORS)
            if self._clip_out is None or self._clip_out.device != dev:
                self._clip_out = torch.empty(2, dtype=torch.float32, device=dev)
                self.total_norm = self._clip_out[0]
                self._clip_ws = None
            self._clip_ws, _arr = _grad_norm(L, grads, max_grad_norm, self._clip_out, self._clip_ws)
            coef = self._clip_out.data_ptr() + 4
        for (b1, b2, eps, step, dev_index), items in batches.items():
            dev = torch.device("cuda", dev_index)
            for i in range(0, len(items), _lib.GS_OPTIM_MAX_TENSORS):
                chunk = items[i:i + _lib.GS_OPTIM_MAX_TENSORS]
                arr = (_lib.GsAdamTensorEx * len(chunk))(*[c[0] for c in chunk])
                with _lib.on_device(dev):
                    _lib.check(L.gs_adam_step_ex(len(chunk), arr, b1, b2, eps, step, coef, _lib.stream_ptr(dev)))
                written = []
                for _rec, p, st in chunk:
                    written += (p, st["exp_avg"], st["exp_avg_sq"])
                    if step == 0:
                        written.append(st["step"])
                _bump_versions(*written)
