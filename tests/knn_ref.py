"""References and point clouds for the knn_points / distCUDA2 tests (numpy only; no GPU, no oracle).

Two kinds of truth are used by tests/test_gpu_knn.py:

* On an integer lattice the truth is computed here, in integers: `lattice_expect` orders exact int64 squared
  distances by (distance, index).  The fp32 points are `g * step + offset` with step and offset chosen so that every
  coordinate, every coordinate difference and every squared distance is exact in fp32 -- any correct fp32 search
  must then return exactly `d_int * step^2`, whatever its operation order.  A lattice is nothing but ties: every
  distance is shared by many points, on and across the boundaries of the search's boxes, so the (distance, index)
  order is decided by the index alone.
* On every other cloud the truth is the C oracle's brute force (oracle.knn_points / oracle.dist2), which uses the
  search's fp32 operation order (dx*dx + dy*dy + dz*dz, no contraction), so answers agree bit for bit.

Every builder is seeded and cached; the arrays it returns are read-only so that tests can share them.
"""
import functools

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
STEP = 0.25
OFFSETS = (0.0, -1.5, 1000.0)  # with STEP = 0.25 and m <= 23: coordinates <= 1005.5 need 10 + 2 bits -- exact in fp32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- lattices --------------------------------------------------------------------------------------------------------

def lattice(m, seed, step=STEP, offset=0.0):
    """An m^3 integer lattice in a seeded random order: (gi (m^3, 3) int64, pts (m^3, 3) fp32 = gi * step + offset).
    Asserts that the fp32 points are exact (so that differences and squared distances are too: they are multiples of
    step and step^2 far below 2^24 of them)."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    g = g[np.random.default_rng(seed).permutation(len(g))]
    return g, lattice_points(g, step, offset)


def lattice_points(gi, step=STEP, offset=0.0):
    """fp32 points of integer coordinates, checked to be exact."""
    exact = gi.astype(np.float64) * step + offset
    pts = exact.astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), exact), "lattice coordinates are not exact in fp32"
    span = float(np.ptp(gi, axis=0).max()) if len(gi) else 0.0
    assert 3 * span * span < 2 ** 24, "squared lattice distances are not exact in fp32"
    return pts


def lattice_expect(gi, K, qi=None, block=256):
    """The K nearest of the integer points `gi` for every query (`qi`, default `gi` itself: a self-search, which finds
    the point itself first): (d_int (Nq, K) int64 squared distances, idx (Nq, K) int64), ordered by (distance, index).
    Exact integer arithmetic, evaluated in row blocks (no Nq x Nr matrix is ever held).  Needs K <= len(gi)."""
    gi = np.asarray(gi, np.int64)
    qi = gi if qi is None else np.asarray(qi, np.int64)
    n = len(gi)
    assert 1 <= K <= n
    ids = np.arange(n, dtype=np.int64)
    d_out = np.empty((len(qi), K), np.int64)
    i_out = np.empty((len(qi), K), np.int64)
    for s in range(0, len(qi), block):
        q = qi[s:s + block]
        d = np.zeros((len(q), n), np.int64)
        for c in range(3):
            t = q[:, c, None] - gi[None, :, c]
            d += t * t
        key = d * n + ids[None, :]  # unique per row, ordered like (distance, index)
        part = np.partition(key, K - 1, axis=1)[:, :K]
        part.sort(axis=1)
        d_out[s:s + block] = part // n
        i_out[s:s + block] = part % n
    return d_out, i_out


def lattice_dists(d_int, step=STEP):
    """The fp32 squared distances of integer ones (exact: d_int * step^2 is a small multiple of a power of two)."""
    exact = d_int.astype(np.float64) * (step * step)
    out = exact.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), exact)
    return out


@functools.lru_cache(maxsize=None)
def lattice_case(m, seed=0, dup=1):
    """(gi, d_int, idx) of the m^3 lattice (each point `dup` times, then shuffled) with its self-search answer for
    K = 9: one more column than any K the search supports, so that column K (0-based) is the best candidate a K-list
    leaves out.  The first K columns are the K-list: the order is total, so a shorter list is a prefix of a longer."""
    gi, _ = lattice(m, seed)
    if dup > 1:
        gi = np.repeat(gi, dup, axis=0)
        gi = gi[np.random.default_rng(seed + 1000).permutation(len(gi))]
    d, i = lattice_expect(gi, 9)
    return _frozen(gi, d, i)


# ---- the search's boxes, restated (only to choose interesting queries: no expectation depends on it) ---------------------

def _spread8(x):
    x = x.astype(np.uint32)
    x = (x | (x << 8)) & np.uint32(0x0000F00F)
    x = (x | (x << 4)) & np.uint32(0x000C30C3)
    x = (x | (x << 2)) & np.uint32(0x00249249)
    return x


def morton_boxes(pts, box=64):
    """Order the points by the 24-bit Morton code of their position in the cloud's bounding box (8 bits per axis, equal
    codes by index) and bound every run of `box` consecutive points: (order (N,), lo (nbox, 3), hi (nbox, 3))."""
    p = np.asarray(pts, np.float32)
    lo, hi = p.min(0), p.max(0)
    ext = np.maximum(hi - lo, np.float32(1e-30))
    u = np.clip((p - lo) / ext * np.float32(255.0), 0, 255).astype(np.uint32)
    code = _spread8(u[:, 0]) | (_spread8(u[:, 1]) << 1) | (_spread8(u[:, 2]) << 2)
    order = np.argsort(code, kind="stable")
    s = p[order]
    starts = np.arange(0, len(p), box)
    blo = np.stack([s[a:a + box].min(0) for a in starts])
    bhi = np.stack([s[a:a + box].max(0) for a in starts])
    return order, blo, bhi


# ---- other clouds ----------------------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


@functools.lru_cache(maxsize=None)
def uniform(n, seed=0):
    return _frozen((_rng(seed).random((n, 3)) * 2 - 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def anisotropic(n, seed=0):
    """Boxes of very unequal extent: one axis 0.3, one 0.01 of the third."""
    p = _rng(seed).random((n, 3)) * 2 - 1
    p[:, 1] *= 0.3
    p[:, 2] *= 0.01
    return _frozen(p.astype(np.float32))


@functools.lru_cache(maxsize=None)
def mixture(n, seed=0):
    """80 % uniform in [-1, 1]^3, 20 % in a cube of side 1e-3 (many boxes inside one Morton cell), interleaved."""
    r = _rng(seed)
    p = r.random((n, 3)) * 2 - 1
    dense = r.random(n) < 0.2
    p[dense] = np.array([0.31, -0.42, 0.17]) + r.random((int(dense.sum()), 3)) * 1e-3
    return _frozen(p.astype(np.float32))


@functools.lru_cache(maxsize=None)
def identical(n):
    return _frozen(np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (n, 1)))


@functools.lru_cache(maxsize=None)
def collinear(n, seed=0):
    """Two axes constant: their extent is 0, clamped to 1e-30 by the Morton kernel."""
    p = np.empty((n, 3), np.float32)
    p[:, 0] = (_rng(seed).random(n) * 2 - 1).astype(np.float32)
    p[:, 1] = np.float32(0.7)
    p[:, 2] = np.float32(-2.0)
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def coplanar(n, seed=0):
    p = (_rng(seed).random((n, 3)) * 2 - 1).astype(np.float32)
    p[:, 1] = np.float32(0.125)
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def island(n=5000, seed=0):
    """2 points far away (first and last row) from n others in a unit cube: with K >= 3 the island's list must reach
    the far cluster, and the cluster occupies one corner cell of the Morton grid."""
    r = _rng(seed)
    body = r.random((n, 3)).astype(np.float32)
    far = (np.array([[40.0, -30.0, 55.0]]) + r.random((2, 3)) * 0.01).astype(np.float32)
    return _frozen(np.concatenate([far[:1], body, far[1:]]))


@functools.lru_cache(maxsize=None)
def offset(n, seed=3):
    """rand * 0.01 + 1000: one fp32 step is 6.1e-5 up there, so there are only ~164 positions per axis and squared
    distances collide exactly all the time."""
    r = _rng(seed).random((n, 3)).astype(np.float32)
    return _frozen(r * np.float32(0.01) + np.float32(1000.0))


BUILDERS = dict(uniform=uniform, anisotropic=anisotropic, mixture=mixture, collinear=collinear, coplanar=coplanar,
                offset=offset)


def sample_rows(n, count, seed):
    """`count` distinct rows of 0..n-1 in ascending order, rows 0 and n-1 always among them."""
    inner = _rng(seed).choice(n - 2, count - 2, replace=False) + 1
    return np.sort(np.concatenate([[0], inner, [n - 1]])).astype(np.int64)


def ties_in_rows(d):
    """Number of rows of an ascending (N, K) distance table that hold two equal entries."""
    return int((d[:, 1:] == d[:, :-1]).any(1).sum())
