"""Float64 numpy restatement of the converter's optimizer step, from torch's documented formulas
(torch.nn.utils.clip_grad_norm_; torch.optim.Adam, algorithm of the docs with weight_decay, no amsgrad, no maximize):

    total_norm = sqrt(sum over all tensors of sum(g^2))
    clip_coef  = min(max_norm / (total_norm + 1e-6), 1)          (a NaN stays a NaN, as torch.clamp keeps it)
    g          = clip_coef * g
    g          = g + weight_decay * p                            (Adam's L2 form, not AdamW's)
    m          = beta1 m + (1 - beta1) g
    v          = beta2 v + (1 - beta2) g^2
    p          = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
"""
import numpy as np


def total_norm(grads):
    """2-norm of all gradients taken together (None entries are skipped)."""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return float(c) if np.isnan(c) else float(min(c, 1.0))


def clip_grads(grads, max_norm):
    """(scaled gradients, total_norm): what clip_grad_norm_ leaves in .grad and returns."""
    norm = total_norm(grads)
    c = clip_coef(norm, max_norm)
    with np.errstate(invalid="ignore"):
        return [None if g is None else np.asarray(g, np.float64) * c for g in grads], norm


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """One Adam step at step number `step` (>= 1) on an (already clipped) gradient; returns new (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(invalid="ignore", over="ignore"):
        if weight_decay != 0:
            g = g + weight_decay * p
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1 = 1.0 - beta1 ** step
        bc2 = 1.0 - beta2 ** step
        p = p - lr / bc1 * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def clip_adam_step(params, grads, ms, vs, hyper, steps, max_norm=None):
    """The fused step over many tensors.  `hyper[k]` = dict(lr, betas, eps, weight_decay); `steps[k]` = the step number
    this update runs at (the previous one + 1); a tensor whose gradient is None is left alone.  Returns
    (params, ms, vs, total_norm or None)."""
    norm = None
    if max_norm is not None:
        grads, norm = clip_grads(grads, max_norm)
    out_p, out_m, out_v = [], [], []
    for p, g, m, v, h, t in zip(params, grads, ms, vs, hyper, steps):
        if g is None:
            q = tuple(np.asarray(a, np.float64) for a in (p, m, v))
        else:
            q = adam_step(p, g, m, v, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h.get("weight_decay", 0.0), t)
        out_p.append(q[0]); out_m.append(q[1]); out_v.append(q[2])
    return out_p, out_m, out_v, norm
