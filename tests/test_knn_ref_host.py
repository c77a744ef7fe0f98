"""The references of tests/test_gpu_knn.py checked against each other on the CPU, and the properties of the test
clouds that the GPU tests rely on (that the ties they mean to exercise really exist)."""
import numpy as np
import pytest

import knn_ref

FLT_MAX = knn_ref.FLT_MAX


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("offset", knn_ref.OFFSETS, ids=lambda o: "off%g" % o)
def test_lattice_expect_equals_the_oracle(oracle, offset):
    """The integer reference and the C brute force are independent and agree on the 12^3 lattice: identical indices,
    distances bitwise d_int * step^2, at all three offsets, K = 1, 3, 8 -- as a self-search and for shuffled queries."""
    gi, pts = knn_ref.lattice(12, 0, knn_ref.STEP, offset)
    perm = np.random.default_rng(7).permutation(len(gi))
    for K in (1, 3, 8):
        d_int, idx = knn_ref.lattice_expect(gi, K)
        od, oi = oracle.knn_points(pts, pts, K)
        assert np.array_equal(oi, idx), K
        assert np.array_equal(_bits(od), _bits(knn_ref.lattice_dists(d_int))), K
        assert np.array_equal(od.astype(np.float64), d_int * knn_ref.STEP ** 2), K
        qd_int, qidx = knn_ref.lattice_expect(gi, K, gi[perm])
        assert np.array_equal(qidx, idx[perm]) and np.array_equal(qd_int, d_int[perm])
    # the cached K = 9 answer: its first K columns are the K-list
    cgi, cd, ci = knn_ref.lattice_case(12)
    assert np.array_equal(cgi, gi)
    d_int, idx = knn_ref.lattice_expect(gi, 8)
    assert np.array_equal(cd[:, :8], d_int) and np.array_equal(ci[:, :8], idx)


def test_a_shorter_list_is_a_prefix_of_a_longer_one(oracle):
    """The GPU tests compute the oracle's K = 8 answer once per cloud and compare a K-list with its first K columns.
    That is the oracle's own K-list because (distance, index) is a total order -- checked here on the cloud with the
    most ties, and under padding (fewer reference points than K)."""
    x = knn_ref.offset(3000)
    d8, i8 = oracle.knn_points(x[:500], x, 8)
    for K in range(1, 8):
        d, i = oracle.knn_points(x[:500], x, K)
        assert np.array_equal(_bits(d), _bits(d8[:, :K])) and np.array_equal(i, i8[:, :K]), K
    few = knn_ref.uniform(5, 1)
    d8, i8 = oracle.knn_points(x[:17], few, 8)
    for K in range(1, 8):
        d, i = oracle.knn_points(x[:17], few, K)
        assert np.array_equal(_bits(d), _bits(d8[:, :K])) and np.array_equal(i, i8[:, :K]), K


def test_lattice_neighbour_shells():
    """Every interior point of the lattice has 6 neighbours at step^2 and 12 at 2 step^2 (so lists of every K >= 2 are
    cut inside a shell of equal distances)."""
    for m in (12, 23):
        gi, _ = knn_ref.lattice(m, 0)
        interior = np.flatnonzero(((gi >= 2) & (gi <= m - 3)).all(1))[:200]
        d, _ = knn_ref.lattice_expect(gi, 20, gi[interior])
        assert (d[:, 0] == 0).all() and (d[:, 1:7] == 1).all() and (d[:, 7:19] == 2).all() and (d[:, 19] == 3).all()
        exact = knn_ref.lattice_dists(d)
        assert (exact[:, 1:7] == np.float32(knn_ref.STEP ** 2)).all() and (exact[:, 7:19] == np.float32(2 * knn_ref.STEP ** 2)).all()


@pytest.mark.parametrize("m,dup", [(12, 1), (23, 1), (12, 4)], ids=["12", "23", "12x4"])
def test_lattice_lists_are_cut_inside_ties(m, dup):
    """In the shuffled order the GPU tests use, the K-th and the (K+1)-th candidate are equally far for at least a few
    hundred queries -- so the index decides which of them enters the list.  A self-search on distinct points cannot have
    that at K = 1 (the point itself is at 0, everything else farther): there it is the lattice with every point four
    times that ties (and the half-step queries of the next test); that lattice in turn has none at K = 4 (four copies
    at 0, then the first shell)."""
    _, d, idx = knn_ref.lattice_case(m, 0, dup)
    tied = {K: int((d[:, K - 1] == d[:, K]).sum()) for K in range(1, 9)}
    for K in range(1, 9):
        if (dup == 1 and K == 1) or (dup == 4 and K == 4):
            assert tied[K] == 0
        else:
            assert tied[K] >= 700, (K, tied)
        # ... and where they tie, the one kept has the smaller index
        t = d[:, K - 1] == d[:, K]
        assert (idx[t, K - 1] < idx[t, K]).all()


def test_half_step_queries_tie_at_every_K():
    """Queries half a step off the lattice along one, two or three axes are equally far from 2, 4 or 8 lattice points:
    between them, a few hundred lists are cut inside a tie at every K from 1 to 8 -- K = 1 included."""
    gi, _, _ = knn_ref.lattice_case(12)
    tied = np.zeros(9, np.int64)
    for e in ((1, 0, 0), (1, 1, 0), (1, 1, 1)):
        qi = 2 * gi + np.array(e)
        d, _ = knn_ref.lattice_expect(2 * gi, 9, qi)
        tied[1:] += [(d[:, K - 1] == d[:, K]).sum() for K in range(1, 9)]
        # exact in fp32 at half the step, at every offset
        for off in knn_ref.OFFSETS:
            knn_ref.lattice_points(qi, knn_ref.STEP / 2, off)
    assert (tied[1:] >= 1000).all(), tied


def test_lattice_sizes_are_the_ones_the_search_branches_on():
    """12^3 points are 27 boxes (one chunk); 23^3 are 191 boxes in three chunks of 64."""
    for m, nbox in ((12, 27), (23, 191)):
        gi, pts = knn_ref.lattice(m, 0)
        order, lo, hi = knn_ref.morton_boxes(pts)
        assert len(lo) == nbox and sorted(order.tolist()) == list(range(m ** 3))
        assert (lo <= hi).all()
        # a box corner of a full lattice is itself a lattice point
        corners = np.concatenate([np.where(np.array(s, bool), hi, lo) for s in np.ndindex(2, 2, 2)])
        have = {tuple(r) for r in pts.tolist()}
        assert all(tuple(c) in have for c in corners.tolist())
    assert (191 + 63) // 64 == 3


def test_offset_cloud_has_exact_ties(oracle):
    x = knn_ref.offset(3000)
    assert x.min() >= 1000 and x.max() <= np.float32(1000.0101)
    d, _ = oracle.knn_points(x, x, 8)
    assert knn_ref.ties_in_rows(d) > 100


def test_oracle_pins_padding_and_small_P(oracle):
    """With fewer reference points than K the tail of a list is (-1, FLT_MAX); dist2 of 1 or 2 points is +inf (FLT_MAX
    summed), of 3 points (d0 + d1 + FLT_MAX) / 3.  Those are the bits the device must give."""
    q, r = knn_ref.uniform(17, 0), knn_ref.uniform(5, 1)
    d, i = oracle.knn_points(q, r, 8)
    assert (i[:, 5:] == -1).all() and (_bits(d[:, 5:]) == 0x7F7FFFFF).all()
    assert (np.sort(i[:, :5], 1) == np.arange(5)).all() and (np.diff(d[:, :5], axis=1) >= 0).all() and (d[:, :5] < 12).all()
    d, i = oracle.knn_points(r[:1], r[:1], 3)
    assert i.tolist() == [[0, -1, -1]] and _bits(d).tolist() == [[0, 0x7F7FFFFF, 0x7F7FFFFF]]
    for P in (1, 2):
        assert np.array_equal(_bits(oracle.dist2(r[:P])), np.full(P, 0x7F800000, np.uint32))
    p3 = r[:3]
    d3, _ = oracle.knn_points(p3, p3, 3)  # (self, nearer, farther)
    want = ((d3[:, 1] + d3[:, 2]) + FLT_MAX) / np.float32(3.0)
    got = oracle.dist2(p3)
    assert np.array_equal(_bits(got), _bits(want)) and np.isfinite(got).all() and (got > 1e38).all()


def test_cloud_builders_are_what_they_say():
    assert len(np.unique(knn_ref.identical(1000), axis=0)) == 1
    c = knn_ref.collinear(3000)
    assert np.ptp(c[:, 1]) == 0 and np.ptp(c[:, 2]) == 0 and len(np.unique(c[:, 0])) > 2900
    p = knn_ref.coplanar(3000)
    assert np.ptp(p[:, 1]) == 0 and np.ptp(p[:, 0]) > 1.9 and np.ptp(p[:, 2]) > 1.9
    isl = knn_ref.island()
    assert len(isl) == 5002 and np.abs(isl[[0, -1]]).min() > 29 and np.abs(isl[1:-1]).max() <= 1
    mix = knn_ref.mixture(3000, 1)
    dense = ((mix - np.array([0.31, -0.42, 0.17], np.float32)) >= 0).all(1) & ((mix - np.array([0.31, -0.42, 0.17], np.float32)) <= 1.1e-3).all(1)
    assert 0.15 < dense.mean() < 0.25
    rows = knn_ref.sample_rows(140000, 2002, 5)
    assert len(np.unique(rows)) == 2002 and rows[0] == 0 and rows[-1] == 139999
    with pytest.raises(ValueError):
        knn_ref.uniform(10)[0, 0] = 1.0  # shared between tests: read-only
