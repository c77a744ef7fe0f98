"""knn_points and distCUDA2 (csrc/knn.hip) at every K, every queries-per-wave variant, on ties, tails and degenerate
clouds.  Everything is compared bit for bit -- indices with np.array_equal, distances as uint32 views -- against the
integer lattice reference of tests/knn_ref.py or the oracle's brute force; no tolerance, no exempt row.

The search has 8 K instantiations x 3 queries-per-wave variants (16 below 2^17 queries, 32 below 2^18, 64 from there)
and two paths (self: the queries are the Morton-ordered reference points, the walk starts in the wave's own chunk;
non-self: queries in the given order, the walk starts at chunk 0 with empty lists).  The parametrisation ids name K,
the path and the query count of every case.
"""
import numpy as np
import pytest
import torch

import knn_ref

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
k_ids = lambda K: "K%d" % K
off_ids = lambda o: "off%g" % o
FLT_MAX_BITS = 0x7F7FFFFF


def _knn(*a, **k):
    from gsplat_mi355.knn import knn_points
    return knn_points(*a, **k)


def _dist2(x):
    from simple_knn._C import distCUDA2
    return distCUDA2(x)


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(res, want_d, want_i, rows=None, tag=None):
    """Every row of the result (or its rows `rows`) equals the expectation: indices, then distance bits."""
    d, i = res.dists.cpu().numpy(), res.idx.cpu().numpy()
    assert d.dtype == np.float32 and i.dtype == np.int64
    d, i = d.reshape(-1, d.shape[-1]), i.reshape(-1, i.shape[-1])
    if rows is not None:
        d, i = d[rows], i[rows]
    assert i.shape == want_i.shape and d.shape == want_d.shape, (tag, i.shape, want_i.shape)
    bad = np.flatnonzero((i != want_i).any(1) | (_bits(d) != _bits(want_d)).any(1))
    if len(bad):
        r = bad[0]
        raise AssertionError("%s: %d of %d rows differ; first row %d: idx %s want %s, d %s want %s"
                             % (tag, len(bad), len(i), r, i[r], want_i[r], d[r], want_d[r]))
    assert np.array_equal(i, want_i) and np.array_equal(_bits(d), _bits(want_d))


_SHARED = {}


def _oracle8(oracle, key, q, r):
    """The oracle's K = 8 answer, computed once per cloud and left unchanged: a K-list is its first K columns
    ((distance, index) is a total order; tests/test_knn_ref_host.py checks that prefix property of the oracle)."""
    if key not in _SHARED:
        d, i = oracle.knn_points(q, r, 8)
        d.setflags(write=False)
        i.setflags(write=False)
        _SHARED[key] = (d, i)
    return _SHARED[key]


# ---- a. every K, small: tails of the box, the chunk and the wave ---------------------------------------------------------

SELF_N = (1, 5, 63, 64, 65, 129, 3000)  # 1 and 5: fewer points than K on the self path
NONSELF_NQ_NR = ((1, 1), (17, 5), (65, 64), (500, 4095), (500, 4096), (500, 4097), (500, 12000))


@pytest.mark.parametrize("cloud", ["uniform", "mixture"])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_self_small(oracle, K, cloud):
    """Self-search (16 queries per wave): one box short of a point, full, one point over, two boxes and a tail, 47 boxes."""
    for n in SELF_N:
        x = knn_ref.BUILDERS[cloud](n, n)
        want_d, want_i = oracle.knn_points(x, x, K)
        if n < K:
            assert (want_i[:, n:] == -1).all() and (_bits(want_d[:, n:]) == FLT_MAX_BITS).all()
        xd = _dev(x)
        _check(_knn(xd, xd, K=K), want_d, want_i, tag="N=%d" % n)


@pytest.mark.parametrize("cloud", ["uniform", "mixture"])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_nonself_small(oracle, K, cloud):
    """Non-self search from chunk 0 over one chunk less a point, exactly one, one plus a point (two chunks) and three
    chunks; query counts around the 16 queries of a wave; fewer reference points than K give (-1, FLT_MAX)."""
    for nq, nr in NONSELF_NQ_NR:
        q = knn_ref.uniform(nq, 100 + nq) * np.float32(1.1)  # some queries outside the reference's bounding box
        r = knn_ref.BUILDERS[cloud](nr, nr)
        want_d, want_i = oracle.knn_points(q, r, K)
        if nr < K:
            assert (want_i[:, nr:] == -1).all() and (_bits(want_d[:, nr:]) == FLT_MAX_BITS).all() and (want_i[:, :nr] >= 0).all()
        _check(_knn(_dev(q), _dev(r), K=K), want_d, want_i, tag="Nq=%d Nr=%d" % (nq, nr))


@pytest.mark.parametrize("nq", [15, 16, 17, 63, 64, 65])
def test_query_count_tails(oracle, nq):
    """Query counts around one wave's 16 queries and around 64, all K, against 1000 points."""
    q, r = knn_ref.mixture(nq, 200 + nq), knn_ref.mixture(1000, 7)
    qd, rd = _dev(q), _dev(r)
    for K in KS:
        _check(_knn(qd, rd, K=K), *oracle.knn_points(q, r, K), tag="K=%d" % K)


# ---- b. the self path and the non-self path agree --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3000, 12288])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_self_and_nonself_paths_agree(oracle, K, n):
    x = knn_ref.mixture(n, 11)
    d8, i8 = _oracle8(oracle, ("paths", n), x, x)
    want = (d8[:, :K], i8[:, :K])
    xd = _dev(x)
    _check(_knn(xd, xd, K=K), *want, tag="self")
    _check(_knn(xd.clone(), xd, K=K), *want, tag="non-self")
    res = _knn(xd[None], xd[None], K=K)
    assert res.dists.shape == (1, n, K) and res.idx.shape == (1, n, K)
    _check(res, *want, tag="batched self")
    wide = torch.zeros(n, 4, device="cuda")
    wide[:, :3] = xd
    assert not wide[:, :3].is_contiguous()
    _check(_knn(wide[:, :3], xd, K=K), *want, tag="strided query")
    _check(_knn(wide[:, :3], wide[:, :3], K=K), *want, tag="strided query that is the reference")
    twice = xd.repeat_interleave(2, 0)
    _check(_knn(xd, twice[::2], K=K), *want, tag="strided reference")


# ---- c. ties ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["self", "nonself"])
@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=off_ids)
@pytest.mark.parametrize("m", [12, 23], ids=["m12", "m23"])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_lattice(K, m, offset, path):
    """Nothing but ties: every list of K >= 2 is cut inside a shell of equally distant points that spans box (and at
    23^3: chunk) boundaries, so the index decides.  12^3 = 27 boxes; 23^3 = 191 boxes in three chunks, so waves start
    their walk in chunk 0, 1 and 2.  Non-self: the same lattice searched for a shuffled copy of itself."""
    gi, d_int, idx = knn_ref.lattice_case(m)
    pts = knn_ref.lattice_points(gi, knn_ref.STEP, offset)
    want_d, want_i = knn_ref.lattice_dists(d_int[:, :K]), idx[:, :K]
    xd = _dev(pts)
    if path == "self":
        _check(_knn(xd, xd, K=K), want_d, want_i)
    else:
        perm = np.random.default_rng(m).permutation(len(gi))
        _check(_knn(_dev(pts[perm]), xd, K=K), want_d[perm], want_i[perm])


def _half_step_case(m, e):
    key = ("half", m, e)
    if key not in _SHARED:
        gi, _, _ = knn_ref.lattice_case(m)
        qi = 2 * gi + np.array(e)
        d, i = knn_ref.lattice_expect(2 * gi, 8, qi)
        _SHARED[key] = (2 * gi, qi, d, i)
    return _SHARED[key]


@pytest.mark.parametrize("m,e", [(12, (1, 0, 0)), (12, (1, 1, 0)), (12, (1, 1, 1)), (23, (1, 1, 1))],
                         ids=["m12-x", "m12-xy", "m12-xyz", "m23-xyz"])
@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=off_ids)
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_lattice_half_step_queries(K, offset, m, e):
    """Queries half a step off the lattice are equally far from 2, 4 or 8 lattice points: the nearest neighbour itself
    is a tie (the one case a self-search on distinct points cannot make: K = 1)."""
    ri, qi, d_int, idx = _half_step_case(m, e)
    h = knn_ref.STEP / 2
    res = _knn(_dev(knn_ref.lattice_points(qi, h, offset)), _dev(knn_ref.lattice_points(ri, h, offset)), K=K)
    _check(res, knn_ref.lattice_dists(d_int[:, :K], h), idx[:, :K])


@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=off_ids)
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_duplicated_lattice(K, offset):
    """Every lattice point four times (6912 points, 108 boxes, two chunks): ties at distance 0, and boxes of zero extent."""
    gi, d_int, idx = knn_ref.lattice_case(12, 0, 4)
    pts = knn_ref.lattice_points(gi, knn_ref.STEP, offset)
    want_d, want_i = knn_ref.lattice_dists(d_int[:, :K]), idx[:, :K]
    assert (want_d[:, :min(K, 4)] == 0).all()
    xd = _dev(pts)
    _check(_knn(xd, xd, K=K), want_d, want_i, tag="self")
    _check(_knn(xd.clone(), xd, K=K), want_d, want_i, tag="non-self")


@pytest.mark.parametrize("n", [1000, 5000])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_all_points_identical(K, n):
    """One Morton code, boxes of zero extent, nothing can be pruned: every list is indices 0..K-1 at distance +0."""
    xd = _dev(knn_ref.identical(n))
    want_i = np.tile(np.arange(K, dtype=np.int64), (n, 1))
    want_d = np.zeros((n, K), np.float32)  # +0: all bits clear
    _check(_knn(xd, xd, K=K), want_d, want_i, tag="self")
    _check(_knn(xd.clone(), xd, K=K), want_d, want_i, tag="non-self")
    if K == 1:
        assert np.array_equal(_bits(_dist2(xd).cpu().numpy()), np.zeros(n, np.uint32))


# ---- d. degenerate geometry -----------------------------------------------------------------------------------------------------

def _degenerate(name):
    if name == "island":
        return knn_ref.island()
    return knn_ref.BUILDERS[name](3000, 3)


@pytest.mark.parametrize("path", ["self", "nonself"])
@pytest.mark.parametrize("cloud", ["collinear", "coplanar", "island", "offset", "anisotropic"])
@pytest.mark.parametrize("K", [1, 3, 8], ids=k_ids)
def test_degenerate_clouds(oracle, K, cloud, path):
    """Zero extent along two axes / one axis (the Morton kernel's extent clamp), two points far from everything else
    (their K = 8 lists must reach the far cluster), a large common offset (fp32 near-ties and exact ties), boxes of
    very unequal extent."""
    x = _degenerate(cloud)
    xd = _dev(x)
    if path == "self":
        _check(_knn(xd, xd, K=K), *oracle.knn_points(x, x, K))
        return
    # the cloud's own points in another order, and other points of the same kind
    other = _degenerate(cloud)[::-1] if cloud == "island" else knn_ref.BUILDERS[cloud](700, 4)
    q = np.concatenate([x[::7], other[:700]])
    _check(_knn(_dev(q), xd, K=K), *oracle.knn_points(q, x, K))


@pytest.mark.parametrize("K", [1, 3, 8], ids=k_ids)
def test_queries_far_outside_the_reference(oracle, K):
    """Queries 100 x the reference's extent away: every box bound is large and nearly equal."""
    r = knn_ref.uniform(5000, 21)
    dirs = knn_ref.uniform(100, 22).astype(np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    q = (np.concatenate([dirs, axes]) * 200.0).astype(np.float32)  # extent 2
    _check(_knn(_dev(q), _dev(r), K=K), *oracle.knn_points(q, r, K))


@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=off_ids)
@pytest.mark.parametrize("K", [1, 3, 8], ids=k_ids)
def test_queries_on_box_corners(K, offset):
    """Queries exactly on the corners of the search's boxes of the 23^3 lattice: the distance to that box is exactly 0
    and the bound of its neighbours equals candidate distances exactly."""
    gi, _, _ = knn_ref.lattice_case(23)
    pts = knn_ref.lattice_points(gi, knn_ref.STEP, offset)
    key = ("corners", offset)
    if key not in _SHARED:
        _, lo, hi = knn_ref.morton_boxes(pts)
        corners = np.concatenate([np.where(np.array(s, bool), hi, lo) for s in np.ndindex(2, 2, 2)])
        qi = np.rint((corners.astype(np.float64) - offset) / knn_ref.STEP).astype(np.int64)
        _SHARED[key] = (qi,) + knn_ref.lattice_expect(gi, 8, qi)
    qi, d_int, idx = _SHARED[key]
    q = knn_ref.lattice_points(qi, knn_ref.STEP, offset)
    assert len(q) == 8 * 191 and (d_int[:, 0] == 0).all()  # a corner of a box of a full lattice is a lattice point
    _check(_knn(_dev(q), _dev(pts), K=K), knn_ref.lattice_dists(d_int[:, :K]), idx[:, :K])


# ---- e. the 32- and 64-query waves ----------------------------------------------------------------------------------------------

WIDE_NQ_NR = [(nq, nr) for nq in ((1 << 17) + 5, (1 << 18) + 5) for nr in (300, 5000)]


@pytest.mark.parametrize("nq,nr", WIDE_NQ_NR, ids=["Nq%d-Nr%d" % c for c in WIDE_NQ_NR])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_nonself_32_and_64_query_waves(oracle, K, nq, nr):
    """Non-self search with 2^17 + 5 (32 queries per wave) and 2^18 + 5 (64) queries: every row."""
    q = knn_ref.uniform(nq, 31) * np.float32(1.2)
    r = knn_ref.mixture(nr, 32)
    d8, i8 = _oracle8(oracle, ("wide", nq, nr), q, r)
    _check(_knn(_dev(q), _dev(r), K=K), d8[:, :K], i8[:, :K])


@pytest.mark.parametrize("n", [140000, 270000], ids=["N140000", "N270000"])
@pytest.mark.parametrize("K", KS, ids=k_ids)
def test_self_32_and_64_query_waves(oracle, K, n):
    """Self-search of 140 000 (32 queries per wave) and 270 000 (64) points: 2002 seeded sample rows, the original
    rows 0 and N-1 among them, every one of which must match."""
    x = knn_ref.mixture(n, 41)
    rows = knn_ref.sample_rows(n, 2002, 42)
    assert len(rows) >= 2000 and rows[0] == 0 and rows[-1] == n - 1
    d8, i8 = _oracle8(oracle, ("wide-self", n), x[rows], x)
    xd = _dev(x)
    _check(_knn(xd, xd, K=K), d8[:, :K], i8[:, :K], rows=rows)


# ---- f. distCUDA2 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 4097])
def test_dist2_small(oracle, P):
    """P = 1, 2: +inf (FLT_MAX summed); P = 3: (d0 + d1 + FLT_MAX) / 3; from P = 4 the mean of three real distances."""
    for cloud in ("uniform", "mixture"):
        x = knn_ref.BUILDERS[cloud](P, 50 + P)
        want = oracle.dist2(x)
        if P <= 2:
            assert (_bits(want) == 0x7F800000).all()
        elif P == 3:
            assert np.isfinite(want).all() and (want > 1e38).all()
        else:
            assert (want < 12).all()
        got = _dist2(_dev(x)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (P,)
        assert np.array_equal(_bits(got), _bits(want)), cloud


@pytest.mark.parametrize("P", [(1 << 17) + 3, (1 << 18) + 3])
def test_dist2_32_and_64_query_waves(oracle, P):
    """The sampled rows against the oracle's K = 4 lists: whether or not a point has a twin with a smaller index, the
    distances to its three nearest OTHER points are entries 1..3 of its own list (entry 0 is a zero)."""
    x = knn_ref.mixture(P, 61)
    rows = knn_ref.sample_rows(P, 2002, 62)
    d4, _ = oracle.knn_points(x[rows], x, 4)
    assert (d4[:, 0] == 0).all()
    want = ((d4[:, 1] + d4[:, 2]) + d4[:, 3]) / np.float32(3.0)
    got = _dist2(_dev(x)).cpu().numpy()
    assert got.shape == (P,)
    assert np.array_equal(_bits(got[rows]), _bits(want))


@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=off_ids)
@pytest.mark.parametrize("m", [12, 23], ids=["m12", "m23"])
def test_dist2_lattice(oracle, m, offset):
    gi, d_int, _ = knn_ref.lattice_case(m)
    pts = knn_ref.lattice_points(gi, knn_ref.STEP, offset)
    d = knn_ref.lattice_dists(d_int[:, 1:4])  # distinct points: column 0 is the point itself
    want = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
    assert np.array_equal(_bits(want), _bits(oracle.dist2(pts)))
    assert np.array_equal(_bits(_dist2(_dev(pts)).cpu().numpy()), _bits(want))


def test_dist2_degenerate_and_strided_input(oracle):
    for n in (1000, 5000):
        assert np.array_equal(_bits(_dist2(_dev(knn_ref.identical(n))).cpu().numpy()), np.zeros(n, np.uint32))
    gi, _, _ = knn_ref.lattice_case(12, 0, 4)  # every point four times: three twins at distance 0
    assert np.array_equal(_bits(_dist2(_dev(knn_ref.lattice_points(gi))).cpu().numpy()), np.zeros(len(gi), np.uint32))
    for x in (knn_ref.offset(3000), knn_ref.collinear(3000, 3), knn_ref.coplanar(3000, 3), knn_ref.island()):
        assert np.array_equal(_bits(_dist2(_dev(x)).cpu().numpy()), _bits(oracle.dist2(x)))
    # a strided fp64 input goes through .contiguous().float(): the bits of its fp32 copy
    x = knn_ref.mixture(3000, 71)
    wide = torch.zeros(3000, 4, dtype=torch.float64, device="cuda")
    wide[:, :3] = _dev(x).double() + 1e-9  # not representable in fp32: rounds back to x
    view = wide[:, :3]
    assert not view.is_contiguous() and view.dtype == torch.float64
    got = _dist2(view).cpu().numpy()
    assert got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(_dist2(view.float().contiguous()).cpu().numpy()))
    assert np.array_equal(_bits(got), _bits(oracle.dist2(view.float().cpu().numpy())))


# ---- g. front-end behaviour -------------------------------------------------------------------------------------------------------

def test_return_nn_and_batch_dimension(oracle):
    q, r = knn_ref.uniform(300, 81), knn_ref.mixture(1000, 82)
    qd, rd = _dev(q), _dev(r)
    want_d, want_i = oracle.knn_points(q, r, 4)
    flat = _knn(qd, rd, K=4, return_nn=True)
    assert flat.dists.shape == (300, 4) and flat.idx.shape == (300, 4) and flat.knn.shape == (300, 4, 3)
    _check(flat, want_d, want_i)
    assert torch.equal(flat.knn, rd[flat.idx])
    assert np.array_equal(flat.knn.cpu().numpy(), r[want_i])
    batched = _knn(qd[None], rd[None], K=4, return_nn=True, return_sorted=True)
    assert batched.dists.shape == (1, 300, 4) and batched.idx.shape == (1, 300, 4) and batched.knn.shape == (1, 300, 4, 3)
    _check(batched, want_d, want_i)
    assert torch.equal(batched.knn[0], flat.knn)
    assert _knn(qd, rd, K=4).knn is None and _knn(qd, rd).dists.shape == (300, 1)  # K defaults to 1


def test_no_queries_and_rejected_calls():
    r = _dev(knn_ref.uniform(100, 83))
    for K in (1, 8):
        res = _knn(torch.empty(0, 3, device="cuda"), r, K=K)
        assert res.dists.shape == (0, K) and res.idx.shape == (0, K)
        assert res.dists.dtype == torch.float32 and res.idx.dtype == torch.int64
        res = _knn(torch.empty(1, 0, 3, device="cuda"), r[None], K=K)
        assert res.dists.shape == (1, 0, K) and res.idx.shape == (1, 0, K)
    with pytest.raises(ValueError):
        _knn(r, torch.empty(0, 3, device="cuda"), K=1)
    for K in (0, 9):
        with pytest.raises(NotImplementedError):
            _knn(r, r, K=K)
    two = torch.stack([r, r])
    with pytest.raises(NotImplementedError):
        _knn(two, two, K=1)
    with pytest.raises(NotImplementedError):
        _knn(r[None], r, K=1)  # a batched query needs a batched reference
    with pytest.raises(RuntimeError):
        _knn(r.cpu(), r.cpu(), K=1)
    with pytest.raises(RuntimeError):
        _knn(r, r.cpu(), K=1)
    with pytest.raises(RuntimeError):
        _dist2(r.cpu())
    for bad in (r.double(), r.half(), r.long()):
        with pytest.raises(TypeError):
            _knn(bad, r, K=1)
        with pytest.raises(TypeError):
            _knn(r, bad, K=1)
    with pytest.raises(TypeError):
        _knn(r[:, :2], r, K=1)


def test_a_view_at_the_references_address_is_not_the_reference(oracle):
    """The self path is for the SAME points.  A strided query that merely starts at the reference's address and has its
    shape (every other row of a buffer whose first half is the reference) is another point set."""
    buf = knn_ref.uniform(2000, 84)
    q, r = buf[::2], buf[:1000]
    bd = _dev(buf)
    qd, rd = bd[::2], bd[:1000]
    assert qd.data_ptr() == rd.data_ptr() and qd.shape == rd.shape
    for K in (1, 5):
        _check(_knn(qd, rd, K=K), *oracle.knn_points(q, r, K), tag="K=%d" % K)


def test_repeatable_and_stream_independent(oracle):
    x = knn_ref.mixture(20000, 85)
    xd = _dev(x)
    first = _knn(xd, xd, K=5)
    again = _knn(xd, xd, K=5)
    assert torch.equal(first.idx, again.idx) and torch.equal(first.dists.view(torch.int32), again.dists.view(torch.int32))
    d2 = _dist2(xd)
    assert torch.equal(d2.view(torch.int32), _dist2(xd).view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = _knn(xd, xd, K=5)
        there_ns = _knn(xd.clone(), xd, K=5)
        d2_there = _dist2(xd)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for res in (there, there_ns):
        assert torch.equal(first.idx, res.idx) and torch.equal(first.dists.view(torch.int32), res.dists.view(torch.int32))
    assert torch.equal(d2.view(torch.int32), d2_there.view(torch.int32))
    rows = knn_ref.sample_rows(20000, 500, 86)
    _check(first, *oracle.knn_points(x[rows], x, 5), rows=rows)
