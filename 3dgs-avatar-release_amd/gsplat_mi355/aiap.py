"""`aiap_loss` and `full_aiap_loss` with the reference's signatures (utils/loss_utils.py:69-102, called at
train.py:163-171): the as-isometric-as-possible regularisers, on the GPU through libgsplat_mi355 (csrc/aiap.hip, whose
header comment carries the spec).  Forward and backward of one or two losses that share a neighbour list are one
autograd node; the backward is deterministic (no atomics) and nothing in either direction waits for the GPU.

Drop-in: `from gsplat_mi355.aiap import full_aiap_loss` in place of the reference's import.
Neighbours come from gsplat_mi355.knn.knn_points; there is no CPU path.  GSPLAT_DEBUG=1: after every forward the
count of neighbour indices outside [0, N) is read back (a host sync) and a nonzero count raises.
"""
import os

import torch

from . import _lib
from .knn import knn_points

_DEBUG = os.environ.get("GSPLAT_DEBUG", "0") == "1"


def _rows(x, name):
    if not x.is_cuda:
        raise RuntimeError("aiap: %s must live on the GPU (no CPU fallback)" % name)
    if x.dtype != torch.float32:
        raise TypeError("aiap: %s must be fp32" % name)
    if x.dim() != 2 or x.shape[1] not in (3, 6):
        raise NotImplementedError("aiap: (N, 3) or (N, 6) rows expected, got %s" % (tuple(x.shape),))
    return x.detach().contiguous()


class _AiapFunction(torch.autograd.Function):
    """(idx, xc0, xd0[, xc1, xd1]) -> (loss0, loss1): one or two sets sharing idx.  With one set loss1 is a zero that
    carries no gradient."""

    @staticmethod
    def forward(ctx, idx, xc0, xd0, xc1, xd1):
        ctx.set_materialize_grads(False)
        two = xc1 is not None
        dev = xc0.device
        N, K = int(idx.shape[0]), int(idx.shape[1])
        xs = [_rows(xc0, "x_canonical"), _rows(xd0, "x_deformed")]
        if two:
            xs += [_rows(xc1, "x_canonical"), _rows(xd1, "x_deformed")]
        idx = idx.detach().to(device=dev, dtype=torch.int64).contiguous()
        n_sets = 2 if two else 1
        L = _lib.load()
        ws = torch.empty(_lib.nbytes(L.gs_aiap_workspace_bytes, N, K, n_sets), dtype=torch.uint8, device=dev)
        loss0 = torch.empty((), dtype=torch.float32, device=dev)
        loss1 = torch.empty((), dtype=torch.float32, device=dev) if two else torch.zeros((), dtype=torch.float32, device=dev)
        losses = (loss0, loss1)
        sets = (_lib.GsAiapSet * 2)()
        for s in range(n_sets):
            sets[s] = _lib.GsAiapSet(xc=xs[2 * s].data_ptr(), xd=xs[2 * s + 1].data_ptr(), D=int(xs[2 * s].shape[1]),
                                     loss=losses[s].data_ptr())
        with _lib.on_device(dev):
            _lib.check(L.gs_aiap_forward(N, K, idx.data_ptr(), n_sets, sets, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        if _DEBUG:
            bad = int(ws[:4].view(torch.int32).item())
            if bad:
                raise IndexError("aiap: %d neighbour indices outside [0, %d)" % (bad, N))
        ctx.save_for_backward(idx, ws, *xs)
        ctx.n_sets = n_sets
        return loss0, loss1

    @staticmethod
    def backward(ctx, g0, g1):
        idx, ws = ctx.saved_tensors[:2]
        xs = ctx.saved_tensors[2:]
        n_sets = ctx.n_sets
        need = ctx.needs_input_grad[1:1 + 2 * n_sets]
        out = [None] * 4
        if not any(need):
            return (None,) * 5
        dev = xs[0].device
        N, K = int(idx.shape[0]), int(idx.shape[1])
        gs = [g0, g1]
        sets = (_lib.GsAiapSet * 2)()
        keep = []
        for s in range(n_sets):
            g = gs[s]
            if g is None:  # an unused loss: its gradient is zero
                g = torch.zeros((), dtype=torch.float32, device=dev)
            g = g.detach().to(torch.float32).contiguous()
            keep.append(g)
            for t in (2 * s, 2 * s + 1):
                if need[t]:
                    out[t] = torch.empty_like(xs[t])
            sets[s] = _lib.GsAiapSet(xc=xs[2 * s].data_ptr(), xd=xs[2 * s + 1].data_ptr(), D=int(xs[2 * s].shape[1]),
                                     dL_dloss=g.data_ptr(), dL_dxc=_lib.ptr(out[2 * s]), dL_dxd=_lib.ptr(out[2 * s + 1]))
        L = _lib.load()
        with _lib.on_device(dev):
            _lib.check(L.gs_aiap_backward(N, K, idx.data_ptr(), n_sets, sets, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        return (None,) + tuple(out)


def _check_idx(nn_ix, N):
    if nn_ix.dim() != 2 or int(nn_ix.shape[0]) != N:
        raise ValueError("aiap: nn_ix must be (N, K) with N = %d rows, got %s" % (N, tuple(nn_ix.shape)))
    K = int(nn_ix.shape[1])
    if K < 2 or K > 8:
        raise NotImplementedError("aiap: 2 <= K <= 8 neighbour columns (column 0 is dropped), got %d" % K)


def aiap_loss(x_canonical, x_deformed, n_neighbors=5, nn_ix=None):
    """utils/loss_utils.py aiap_loss: mean over i and k = 1 .. K-1 of
    | |xc_i - xc_idx[i,k]| - |xd_i - xd_idx[i,k]| |; nn_ix None: the K = n_neighbors + 1 nearest canonical points."""
    if x_canonical.shape != x_deformed.shape:
        raise ValueError("Input point sets must have the same shape.")
    if nn_ix is None:
        if x_canonical.dim() != 2 or x_canonical.shape[1] != 3:
            raise NotImplementedError("aiap_loss: the K-NN search (nn_ix=None) is for (N, 3) points only")
        _, nn_ix, _ = knn_points(x_canonical.detach().unsqueeze(0), x_canonical.detach().unsqueeze(0), K=n_neighbors + 1,
                                 return_sorted=True)
        nn_ix = nn_ix.squeeze(0)
    _check_idx(nn_ix, int(x_canonical.shape[0]))
    loss, _ = _AiapFunction.apply(nn_ix, x_canonical, x_deformed, None, None)
    return loss


def full_aiap_loss(gs_can, gs_obs, n_neighbors=5):
    """utils/loss_utils.py full_aiap_loss: (aiap_loss(xyz_can, xyz_obs), aiap_loss(cov_can, cov_obs)) with ONE
    knn_points(xyz_can, K = n_neighbors) neighbour list, both losses in one fused call.  The objects need only
    `get_xyz` and `get_covariance()`."""
    xyz_can, xyz_obs = gs_can.get_xyz, gs_obs.get_xyz
    cov_can, cov_obs = gs_can.get_covariance(), gs_obs.get_covariance()
    _, nn_ix, _ = knn_points(xyz_can.detach().unsqueeze(0), xyz_can.detach().unsqueeze(0), K=n_neighbors, return_sorted=True)
    nn_ix = nn_ix.squeeze(0)
    if xyz_can.shape != xyz_obs.shape or cov_can.shape != cov_obs.shape:
        raise ValueError("Input point sets must have the same shape.")
    _check_idx(nn_ix, int(xyz_can.shape[0]))
    return _AiapFunction.apply(nn_ix, xyz_can, xyz_obs, cov_can, cov_obs)
