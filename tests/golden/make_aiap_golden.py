"""Generates tests/golden/aiap.npz by EXECUTING the reference's own aiap_loss / full_aiap_loss (utils/loss_utils.py) on
the CPU (only possible where the reference tree exists; the tests only read the .npz).

Only those two function definitions are taken from the file's syntax tree and executed (the module imports packages
that are absent here), with `torch`, `F` and a brute-force CPU stand-in for pytorch3d's knn_points in scope (same
return shape; ties broken by index).  Stored: inputs, idx, the losses and the autograd gradients of all four inputs, in
fp32 (the precision the reference trains in) and fp64; nothing of the reference's text.

Cases (keys "<case>/idx", "<case>/<set>/{xc,xd}" (fp32 inputs; the fp64 runs use the same values),
"<case>/<set>/loss_{f32,f64}", "<case>/<set>/{gxc,gxd}_{f32,f64}"):
  a  full_aiap_loss (sets xyz, D = 3, and cov, D = 6) on a body-like cloud under a smooth non-rigid deformation
  b  aiap_loss(nn_ix=None), n_neighbors = 5 (K = 6)
  c  explicit idx with duplicate canonical points (a = 0) and coincident deformed pairs (b = 0), and both at once
  d  xd equal to xc bit for bit (D = 6): loss 0, every gradient 0
  e  a hub: an explicit idx in which most rows name row 0
Outside c and d every pair has |a - b| >= 1e-3 max(a, b) (fp32 decides every sign as fp64 does), and the K-NN
distances of a and b have no near-ties (relative gaps >= 1e-4), so a GPU K-NN in fp32 returns the same idx.

Run:  python tests/golden/make_aiap_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aiap_ref  # noqa: E402

N_A, N_B, N_C, N_D, N_E = 1024, 384, 256, 128, 320


def _load_functions(rel, names, scope):
    """Executes only the named top-level function definitions of a reference file."""
    path = os.path.join(REF, rel)
    tree = ast.parse(open(path).read(), filename=path)
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in picked) == sorted(names), [n.name for n in picked]
    ns = dict(scope)
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns


def knn_points(p1, p2, K=1, return_sorted=True):
    """pytorch3d.ops.knn_points for one batch, brute force: (dists (1, N1, K), idx (1, N1, K), None), ties by index."""
    q, r = p1[0].detach().double(), p2[0].detach().double()
    d2 = ((q[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    d, i = torch.sort(d2, dim=1, stable=True)
    return d[None, :, :K].to(p1.dtype), i[None, :, :K], None


class _Gs(object):
    def __init__(self, xyz, cov):
        self._xyz, self._cov = xyz, cov

    @property
    def get_xyz(self):
        return self._xyz

    def get_covariance(self):
        return self._cov


def _rot(axis_angle):
    th = np.linalg.norm(axis_angle, axis=-1, keepdims=True)
    k = axis_angle / np.maximum(th, 1e-12)
    K = np.zeros(axis_angle.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    K = K - np.swapaxes(K, -1, -2)
    s, c = np.sin(th)[..., None], np.cos(th)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def _strip(c):
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], 1)


def _body(n, rng):
    """Points on a torso, a head and four limbs (capsule surfaces), 1.7 units tall."""
    parts = [((0, 1.1, 0), (0, 1.5, 0), 0.16), ((0, 1.62, 0), (0, 1.62, 0), 0.1), ((-0.1, 0.95, 0), (-0.12, 0.05, 0), 0.07),
             ((0.1, 0.95, 0), (0.12, 0.05, 0), 0.07), ((-0.2, 1.45, 0), (-0.75, 1.45, 0), 0.05),
             ((0.2, 1.45, 0), (0.75, 1.45, 0), 0.05)]
    out = []
    for p in range(n):
        a, b, r = parts[rng.integers(len(parts))]
        a, b = np.array(a, float), np.array(b, float)
        u = rng.normal(size=3)
        out.append(a + rng.random() * (b - a) + r * u / np.linalg.norm(u))
    return np.array(out)


def _deform(x, rng):
    """Smooth non-rigid: a height-dependent twist, a bend of the arms, a breathing scale; J its local rotation."""
    aa = np.stack([0.3 * np.sin(2.0 * x[:, 0]), 0.4 * x[:, 1] - 0.3, 0.5 * np.tanh(3.0 * x[:, 0]) * (x[:, 1] > 1.3)], 1)
    R = _rot(aa)
    y = np.einsum("nij,nj->ni", R, x) * (1.0 + 0.05 * np.sin(4.0 * x[:, 1]))[:, None] + 0.02 * np.sin(5.0 * x[:, [2, 0, 1]])
    return y, R


def _knn_ok(x, k):
    d2, _ = aiap_ref.knn(x, k + 1)
    gap = np.diff(d2, axis=1) / np.maximum(d2[:, 1:], 1e-30)
    return (gap[:, :k] >= 1e-4).all(1)  # the first k + 1 distances strictly ordered (the point itself: 0 first)


def _cloud(x, k, rng):
    """Jitters points until their K-NN has no near-ties."""
    x = x.copy()
    for _ in range(100):
        ok = _knn_ok(x, k)
        if ok.all():
            return x
        x[~ok] += rng.normal(scale=1e-3, size=(int((~ok).sum()), 3))
    raise RuntimeError("could not break the K-NN ties")


def _margins_by_jitter(xc, xd, idx, rng, scale):
    """Jitters the deformed rows of pairs whose |a - b| < 1e-3 max(a, b) (the neighbour list is fixed here)."""
    xd = xd.copy()
    for _ in range(200):
        a, b = aiap_ref.distances(xc, xd, idx)
        i, j = aiap_ref.pairs(idx)
        bad = (a > 0) & (b > 0) & (np.abs(a - b) < 1e-3 * np.maximum(a, b))
        if not bad.any():
            return xd
        rows = np.unique(i[bad])
        xd[rows] += rng.normal(scale=scale, size=(rows.shape[0], xd.shape[1]))
        xd = xd.astype(np.float32).astype(np.float64)
    raise RuntimeError("could not separate a from b")


def _run(fn, sets, dt):
    """Calls fn(*tensors) -> loss or tuple of losses; returns per set (loss, gxc, gxd) as numpy of dtype dt."""
    ts = [[torch.tensor(x, dtype=dt, requires_grad=True) for x in s] for s in sets]
    losses = fn(ts)
    if not isinstance(losses, tuple):
        losses = (losses,)
    sum(losses).backward()
    return [(l.detach().numpy(), t[0].grad.numpy(), t[1].grad.numpy()) for l, t in zip(losses, ts)]


def _store(out, case, names, sets, fn, idx):
    out["%s/idx" % case] = np.asarray(idx, np.int64)
    for dt_tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for name, s, (l, gc, gd) in zip(names, sets, _run(fn, sets, dt)):
            p = "%s/%s/" % (case, name)
            out[p + "xc"], out[p + "xd"] = s[0].astype(np.float32), s[1].astype(np.float32)
            out[p + "loss_" + dt_tag] = np.asarray(l)
            out[p + "gxc_" + dt_tag], out[p + "gxd_" + dt_tag] = gc, gd


def main():
    ns = _load_functions("utils/loss_utils.py", ["aiap_loss", "full_aiap_loss"], dict(torch=torch, F=F, knn_points=knn_points))
    aiap_loss, full_aiap_loss = ns["aiap_loss"], ns["full_aiap_loss"]
    rng = np.random.default_rng(20261016)
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # values exactly representable in fp32
    out = {}

    # (a) full_aiap_loss, body-like cloud
    xc = f32(_cloud(f32(_body(N_A, rng)), 5, rng))
    xd, R = _deform(xc, rng)
    xd = f32(xd)
    S = np.exp(rng.normal(-4.0, 0.4, size=(N_A, 3)))
    Q = _rot(rng.normal(size=(N_A, 3)))
    L = Q * S[:, None, :]
    cc = f32(_strip(L @ np.swapaxes(L, 1, 2)))
    Lo = R @ Q * (S * (1.0 + 0.3 * rng.random((N_A, 3))))[:, None, :]
    co = f32(_strip(Lo @ np.swapaxes(Lo, 1, 2)))
    _, idx = aiap_ref.knn(xc, 5)
    xd = _margins_by_jitter(xc, xd, idx, rng, 1e-3)
    co = _margins_by_jitter(cc, co, idx, rng, 1e-5)
    full = lambda ts: full_aiap_loss(_Gs(ts[0][0], ts[1][0]), _Gs(ts[0][1], ts[1][1]))
    _store(out, "a", ("xyz", "cov"), [(xc, xd), (cc, co)], full, idx)
    _, ref_idx, _ = knn_points(torch.tensor(xc)[None], torch.tensor(xc)[None], K=5)
    assert np.array_equal(ref_idx[0].numpy(), idx)

    # (b) aiap_loss(nn_ix=None), K = 6
    xc = f32(_cloud(f32(rng.normal(size=(N_B, 3))), 6, rng))
    xd, _ = _deform(xc, rng)
    _, idx = aiap_ref.knn(xc, 6)
    xd = _margins_by_jitter(xc, f32(xd), idx, rng, 1e-3)
    _store(out, "b", ("x",), [(xc, xd)], lambda ts: aiap_loss(ts[0][0], ts[0][1]), idx)

    # (c) duplicates: rows 0..9 copy xc of rows 10..19 (a = 0 on those pairs), rows 20..29 copy xd of 30..39 (b = 0),
    # rows 40..49 copy both of 50..59 (a = b = 0, sign 0)
    xc = f32(rng.normal(size=(N_C, 3)))
    xd = f32(xc + 0.3 * rng.normal(size=(N_C, 3)))
    xc[0:10] = xc[10:20]
    xd[20:30] = xd[30:40]
    xc[40:50], xd[40:50] = xc[50:60], xd[50:60]
    idx = np.concatenate([np.arange(N_C)[:, None], rng.integers(0, N_C, size=(N_C, 4))], 1)
    idx = aiap_ref.fix_margins(xc, xd, idx, rng)
    for lo in (0, 20, 40):
        idx[lo:lo + 10, 1] = np.arange(lo + 10, lo + 20)
        idx[lo + 10:lo + 20, 2] = np.arange(lo, lo + 10)
    idx = aiap_ref.fix_margins(xc, xd, idx, rng)
    _store(out, "c", ("x",), [(xc, xd)], lambda ts: aiap_loss(ts[0][0], ts[0][1], nn_ix=torch.tensor(idx)), idx)

    # (d) xd == xc, D = 6
    xc = f32(rng.normal(size=(N_D, 6)))
    idx = np.concatenate([np.arange(N_D)[:, None], rng.integers(0, N_D, size=(N_D, 4))], 1)
    _store(out, "d", ("x",), [(xc, xc.copy())], lambda ts: aiap_loss(ts[0][0], ts[0][1], nn_ix=torch.tensor(idx)), idx)

    # (e) a hub: columns 1 and 2 of two thirds of the rows name row 0
    xc = f32(rng.normal(size=(N_E, 3)))
    xd = f32(xc * (1.0 + 0.2 * rng.random((N_E, 1))) + 0.1 * rng.normal(size=(N_E, 3)))
    idx = np.concatenate([np.arange(N_E)[:, None], rng.integers(0, N_E, size=(N_E, 4))], 1)
    hub = rng.random(N_E) < 2.0 / 3.0
    idx[hub, 1] = 0
    idx[hub, 2] = 0
    idx = aiap_ref.fix_margins(xc, xd, idx, rng)
    _store(out, "e", ("x",), [(xc, xd)], lambda ts: aiap_loss(ts[0][0], ts[0][1], nn_ix=torch.tensor(idx)), idx)

    path = os.path.join(HERE, "aiap.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
