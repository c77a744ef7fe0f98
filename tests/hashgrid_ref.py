"""A float64 restatement of the hash-grid encoding (tinycudann.Encoding, HashGrid, 3-D, linear; the spec at the top of
csrc/hashgrid.hip), written from the spec.  numpy form: cells, corner entries, weights, the encoding and both gradients
(the parameter gradient by np.bincount).  pos = float32(float64(scale) * float64(x) + 0.5): the float64 product of two
float32 values is exact, so this is fmaf on every input the tests draw, and cells and entries match the kernels bit for
bit.  A torch form of the same encoding (gathers plus autograd, any dtype and device) serves the end-to-end test.  The
level table comes from the library (gs_hashgrid_levels) through gsplat_mi355.hashgrid.levels.
"""
import numpy as np

PRIMES = (1, 2654435761, 805459861)
M32 = 0xFFFFFFFF


def cells(x, scale):
    """(c uint32 [N, 3], t float64 [N, 3]) of level scale `scale` (a float32 value) for x [N, 3] (float32 values)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    pos = (np.float64(np.float32(scale)) * x + 0.5).astype(np.float32)
    fl = np.floor(pos)
    c = fl.astype(np.int64).astype(np.int32).astype(np.uint32)
    t = (pos - fl).astype(np.float64)  # exact in float32
    return c, t


def corner_index(v, res, size):
    """entry of corner cells v uint32 [..., 3] on a level of resolution `res` and `size` table rows (uint32 arithmetic)."""
    v = np.asarray(v, np.uint64) & M32
    stride = np.uint64(1)
    idx = np.zeros(v.shape[:-1], np.uint64)
    for d in range(3):
        if not int(stride) <= size:
            break
        idx = (idx + v[..., d] * stride) & M32
        stride = np.uint64((int(stride) * int(res)) & M32)
    if size < int(stride):
        idx = np.zeros(v.shape[:-1], np.uint64)
        for d in range(3):
            idx ^= (v[..., d] * np.uint64(PRIMES[d])) & M32
    return (idx % np.uint64(size)).astype(np.int64)


def corners(x, scale, res, size):
    """(entries int64 [N, 8], weights float64 [N, 8], t [N, 3]) of one level; corner k = bits (d0, d1, d2) of k."""
    c, t = cells(x, scale)
    ent = np.empty((c.shape[0], 8), np.int64)
    w = np.empty((c.shape[0], 8), np.float64)
    for k in range(8):
        b = np.array([(k >> d) & 1 for d in range(3)], np.uint64)
        v = (c.astype(np.uint64) + b) & M32
        ent[:, k] = corner_index(v, res, size)
        w[:, k] = np.prod(np.where(b.astype(bool), t, 1.0 - t), axis=1)
    return ent, w, t


def encode(x, params, table, F):
    """out float64 [N, L F]; table = (offsets, scales, resolutions, n_params)."""
    offsets, scales, res, _ = table
    L = len(scales)
    th = np.asarray(params, np.float64).reshape(-1, F)
    x = np.asarray(x, np.float32)
    out = np.zeros((x.shape[0], L * F), np.float64)
    for l in range(L):
        size = offsets[l + 1] - offsets[l]
        ent, w, _ = corners(x, scales[l], res[l], size)
        out[:, l * F:(l + 1) * F] = np.einsum("nk,nkf->nf", w, th[offsets[l] + ent])
    return out


def backward(x, params, G, table, F):
    """(dL/dx float64 [N, 3], dL/dparams float64 [n_params]) for upstream G [N, L F]."""
    offsets, scales, res, n_params = table
    L = len(scales)
    th = np.asarray(params, np.float64).reshape(-1, F)
    G = np.asarray(G, np.float64)
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    dx = np.zeros((n, 3), np.float64)
    dp = np.zeros((n_params // F, F), np.float64)
    for l in range(L):
        size = offsets[l + 1] - offsets[l]
        ent, w, t = corners(x, scales[l], res[l], size)
        g = G[:, l * F:(l + 1) * F]
        rows = (offsets[l] + ent).reshape(-1)
        for f in range(F):
            dp[:, f] += np.bincount(rows, weights=(w * g[:, f:f + 1]).reshape(-1), minlength=n_params // F)
        s = np.einsum("nf,nkf->nk", g, th[offsets[l] + ent])  # sum_f g_f theta_k,f
        for d in range(3):
            dd = np.zeros(n, np.float64)
            for k in range(8):
                bits = [(k >> e) & 1 for e in range(3)]
                other = np.ones(n, np.float64)
                for e in range(3):
                    if e != d:
                        other *= t[:, e] if bits[e] else 1.0 - t[:, e]
                dd += (1.0 if bits[d] else -1.0) * other * s[:, k]
            dx[:, d] += np.float64(np.float32(scales[l])) * dd
    return dx, dp.reshape(-1)


def encode_torch(x, params, table, F):
    """The same encoding as a torch graph (gathers, autograd; any float dtype and device): out [N, L F] in params' dtype.
    pos = scale * x + 0.5 in that dtype (float64 for the parity tests: the cells then match the kernels' on every input
    the tests draw, as in the numpy form)."""
    import torch
    offsets, scales, res, _ = table
    L = len(scales)
    th = params.reshape(-1, F)
    outs = []
    xq = x.to(params.dtype)
    for l in range(L):
        size = offsets[l + 1] - offsets[l]
        pos = (float(np.float32(scales[l])) * xq + 0.5).float().to(params.dtype)
        fl = torch.floor(pos)
        t = pos - fl
        c = cells(x.detach().float().cpu().numpy(), scales[l])[0]
        acc = 0
        for k in range(8):
            b = np.array([(k >> d) & 1 for d in range(3)], np.uint64)
            ent = corner_index((c.astype(np.uint64) + b) & M32, res[l], size)
            idx = torch.as_tensor(offsets[l] + ent, device=params.device)
            w = 1
            for d in range(3):
                w = w * (t[:, d] if b[d] else 1.0 - t[:, d])
            acc = acc + w[:, None] * th[idx]
        outs.append(acc)
    return torch.cat(outs, dim=1)
