"""A float64 restatement of the AIAP regularisers (utils/loss_utils.py aiap_loss; the spec at the top of
csrc/aiap.hip), written from the spec: the losses and the gradients of all four inputs.  numpy only, so it runs
wherever the tests do.  tests/test_aiap_host.py pins it to the reference's own autograd results (tests/golden/aiap.npz).
"""
import numpy as np


def pairs(idx):
    """(i, j) of every pair: row i with idx[i, k], k = 1 .. K-1 (column 0 is dropped, whatever it holds)."""
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    return np.repeat(np.arange(n, dtype=np.int64), k - 1), idx[:, 1:].reshape(-1)


def distances(xc, xd, idx):
    i, j = pairs(idx)
    xc, xd = np.asarray(xc, np.float64), np.asarray(xd, np.float64)
    a = np.sqrt(((xc[i] - xc[j]) ** 2).sum(1))
    b = np.sqrt(((xd[i] - xd[j]) ** 2).sum(1))
    return a, b


def aiap(xc, xd, idx, g=1.0):
    """(loss, dL/dxc, dL/dxd) in float64 for upstream gradient g."""
    xc, xd = np.asarray(xc, np.float64), np.asarray(xd, np.float64)
    i, j = pairs(idx)
    dc, dd = xc[i] - xc[j], xd[i] - xd[j]
    a, b = np.sqrt((dc * dc).sum(1)), np.sqrt((dd * dd).sum(1))
    m = i.shape[0]
    loss = np.abs(a - b).sum() / m
    s = np.sign(a - b) * (g / m)
    wa = np.where(a > 0, s / np.where(a > 0, a, 1.0), 0.0)[:, None] * dc
    wb = np.where(b > 0, s / np.where(b > 0, b, 1.0), 0.0)[:, None] * dd
    gc, gd = np.zeros_like(xc), np.zeros_like(xd)
    np.add.at(gc, i, wa)
    np.add.at(gc, j, -wa)
    np.add.at(gd, i, -wb)
    np.add.at(gd, j, wb)
    return loss, gc, gd


def knn(x, k):
    """Brute-force K nearest points of every point (itself first), squared distances in float64, ties by index."""
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, order, 1), order


def fix_margins(xc, xd, idx, rng, rel=1e-3, rounds=50):
    """Redraws neighbour j of every pair whose |a - b| < rel max(a, b), so that fp32 decides every sign as float64
    does (a pair with a or b exactly 0 is decided exactly either way and stays); a pair still short after `rounds`
    redraws becomes (i, i) (a = b = 0 exactly).  Returns a new idx."""
    idx = np.array(idx, dtype=np.int64)
    n, k = idx.shape
    for r in range(rounds + 1):
        a, b = distances(xc, xd, idx)
        i, j = pairs(idx)
        bad = (a > 0) & (b > 0) & (np.abs(a - b) < rel * np.maximum(a, b))
        if not bad.any():
            return idx
        rows, cols = i[bad], np.nonzero(bad)[0] % (k - 1) + 1
        idx[rows, cols] = rng.integers(0, n, size=rows.shape[0]) if r < rounds else rows
    return idx
