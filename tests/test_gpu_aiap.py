"""The fused AIAP regularisers (gsplat_mi355.aiap, csrc/aiap.hip) on the GPU: parity with the reference's own fp64
autograd results (tests/golden/aiap.npz), edges of the block, sort and scan sizes against the float64 restatement
tests/aiap_ref.py, device-side grad scalars, bitwise determinism with a hub, and no host synchronisation.

Sign decisions: every fixture pair outside cases c and d has |a - b| >= 1e-3 max(a, b), and a flipped sign moves a
row's gradient by 2 g / M times a unit vector, hundreds of times the 1e-5 tolerance: the gradient checks are exact on
the signs.  Where the reference's gradient is exactly 0 (cases c and d), the kernel's must be exactly 0 too."""
import os

import numpy as np
import pytest
import torch

import aiap_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CASES = {"a": ("xyz", "cov"), "b": ("x",), "c": ("x",), "d": ("x",), "e": ("x",)}


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(ROOT, "tests", "golden", "aiap.npz"))
    return {k: d[k] for k in d.files}


def _fn():
    from gsplat_mi355 import aiap
    return aiap


def _leaf(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).requires_grad_(True)


def _close(got, want, tol=1e-5, what=""):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, "%s: max err %.3g of max %.3g" % (what, err, scale)
    assert (got[want == 0] == 0).all(), "%s: nonzero where the reference is exactly 0" % what


def _run_sets(idx, sets, scales=None):
    """Fused forward + backward of one or two (xc, xd) numpy sets; returns per set (loss, gxc, gxd) and the leaves."""
    a = _fn()
    leaves = [(_leaf(xc), _leaf(xd)) for xc, xd in sets]
    t_idx = torch.from_numpy(np.asarray(idx, np.int64)).to(DEV)
    if len(sets) == 2:
        l0, l1 = a._AiapFunction.apply(t_idx, leaves[0][0], leaves[0][1], leaves[1][0], leaves[1][1])
        losses = [l0, l1]
    else:
        losses = [a.aiap_loss(leaves[0][0], leaves[0][1], nn_ix=t_idx)]
    scales = scales or [1.0] * len(losses)
    sum(s * l for s, l in zip(scales, losses)).backward()
    torch.cuda.synchronize()
    return [(float(l.detach()), lv[0].grad, lv[1].grad) for l, lv in zip(losses, leaves)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_fixture_parity(fx, case):
    idx = fx["%s/idx" % case]
    sets = [(fx["%s/%s/xc" % (case, n)], fx["%s/%s/xd" % (case, n)]) for n in CASES[case]]
    for name, (loss, gc, gd) in zip(CASES[case], _run_sets(idx, sets)):
        p = "%s/%s/" % (case, name)
        want = float(fx[p + "loss_f64"])
        assert abs(loss - want) <= 1e-6 * abs(want), (case, name, loss, want)
        if want == 0.0:
            assert loss == 0.0
        _close(gc, fx[p + "gxc_f64"], what=p + "gxc")
        _close(gd, fx[p + "gxd_f64"], what=p + "gxd")


def test_full_aiap_loss_end_to_end(fx):
    """Through knn_points: the same idx as the reference's K-NN and the same values as case (a)."""
    from gsplat_mi355.knn import knn_points

    class Gs(object):
        def __init__(self, xyz, cov):
            self.get_xyz, self._cov = xyz, cov

        def get_covariance(self):
            return self._cov

    xyz_c, xyz_o, cov_c, cov_o = (_leaf(fx["a/" + k]) for k in ("xyz/xc", "xyz/xd", "cov/xc", "cov/xd"))
    _, idx, _ = knn_points(xyz_c.detach()[None], xyz_c.detach()[None], K=5)
    assert np.array_equal(idx[0].cpu().numpy(), fx["a/idx"])
    l_xyz, l_cov = _fn().full_aiap_loss(Gs(xyz_c, cov_c), Gs(xyz_o, cov_o))
    (l_xyz + l_cov).backward()
    for name, l, g_c, g_o in (("xyz", l_xyz, xyz_c, xyz_o), ("cov", l_cov, cov_c, cov_o)):
        want = float(fx["a/%s/loss_f64" % name])
        assert abs(float(l) - want) <= 1e-6 * want
        _close(g_c.grad, fx["a/%s/gxc_f64" % name], what=name + " gxc")
        _close(g_o.grad, fx["a/%s/gxd_f64" % name], what=name + " gxd")


def _random_case(n, k, d, seed, hub=0):
    rng = np.random.default_rng(seed)
    xc = rng.normal(size=(n, d)).astype(np.float32)
    xd = (xc * (1.0 + 0.2 * rng.random((n, 1))) + 0.1 * rng.normal(size=(n, d))).astype(np.float32)
    idx = np.concatenate([np.arange(n)[:, None], rng.integers(0, n, size=(n, k - 1))], 1)
    if hub:
        idx[:hub, 1] = 0
    idx = aiap_ref.fix_margins(xc.astype(np.float64), xd.astype(np.float64), idx, rng)
    return xc, xd, idx


# N: 1, 2, K, block edges, the sort's pass-count edges (keys of 8 / 16 bits) and block sizes, a partly filled last block,
# the small / large sort switch (M around 2^20), 200k and 1.1 M
EDGES = [(1, 5, (3,)), (2, 5, (3, 6)), (5, 5, (3,)), (8, 8, (6,)), (63, 2, (3,)), (64, 5, (3, 6)), (65, 6, (6, 3)),
         (255, 5, (3,)), (256, 8, (3, 6)), (257, 2, (6,)), (1023, 5, (3,)), (1025, 6, (6, 6)), (4097, 5, (3, 3)),
         (65535, 5, (3,)), (65536, 2, (3, 6)), (262144, 5, (3,)), (262145, 5, (3, 6)), (200000, 5, (3, 6)),
         (200000, 8, (6,)), (1100000, 5, (3, 6))]


@pytest.mark.parametrize("n,k,ds", EDGES, ids=["N%d-K%d-D%s" % (n, k, "".join(map(str, ds))) for n, k, ds in EDGES])
def test_edges_against_restatement(n, k, ds):
    sets, idx = [], None
    for s, d in enumerate(ds):
        xc, xd, idx_s = _random_case(n, k, d, seed=n * 31 + k * 7 + s)
        if idx is None:
            idx = idx_s
        else:  # one shared idx: the second set's margins are kept by redrawing on it too
            idx = aiap_ref.fix_margins(xc.astype(np.float64), xd.astype(np.float64), idx, np.random.default_rng(n + s))
        sets.append((xc, xd))
    if len(ds) == 2:  # the first set's margins again, after the second set's redraws
        idx = aiap_ref.fix_margins(sets[0][0].astype(np.float64), sets[0][1].astype(np.float64), idx,
                                   np.random.default_rng(n), rounds=0)
    got = _run_sets(idx, sets)
    for s, ((xc, xd), (loss, gc, gd)) in enumerate(zip(sets, got)):
        want_l, want_c, want_d = aiap_ref.aiap(xc, xd, idx)
        # a - b cancels: fp32 a and b carry up to half an ulp each, which is more than 1e-6 of |a - b| where the
        # deformation is small against the distances (N = 2: a few pairs, nothing to average it out)
        a, b = aiap_ref.distances(xc, xd, idx)
        tol = 1e-6 * abs(want_l) + 2.0 ** -24 * float((a + b).mean())
        assert abs(loss - want_l) <= tol, (s, loss, want_l, tol)
        _close(gc, want_c, what="set %d gxc" % s)
        _close(gd, want_d, what="set %d gxd" % s)


def test_views_and_partial_requires_grad():
    xc, xd, idx = _random_case(3000, 5, 3, seed=3)
    a = _fn()
    # non-contiguous views: every other row of a wider buffer, and a transposed layout
    big_c = torch.zeros(6000, 4, device=DEV)
    big_c[::2, :3] = torch.from_numpy(xc).to(DEV)
    v_c = big_c[::2, :3].requires_grad_(False)
    t_d = torch.from_numpy(np.ascontiguousarray(xd.T)).to(DEV).requires_grad_(True)
    v_d = t_d.t()
    assert not v_c.is_contiguous() and not v_d.is_contiguous()
    loss = a.aiap_loss(v_c, v_d, nn_ix=torch.from_numpy(idx).to(DEV))
    loss.backward()
    want_l, want_c, want_d = aiap_ref.aiap(xc, xd, idx)
    assert abs(float(loss) - want_l) <= 1e-6 * want_l
    _close(t_d.grad.t(), want_d, what="gxd through a view")
    # only the canonical side requires grad
    lc = _leaf(xc)
    a.aiap_loss(lc, torch.from_numpy(xd).to(DEV), nn_ix=torch.from_numpy(idx).to(DEV)).backward()
    _close(lc.grad, want_c, what="gxc alone")


def test_device_grad_scalars():
    """backward of 1.0 l_xyz + 100 l_cov = the separately scaled gradients (the scalars are read on the device)."""
    xc, xd, idx = _random_case(5000, 5, 3, seed=11)
    cc, cd, _ = _random_case(5000, 5, 6, seed=12)
    idx = aiap_ref.fix_margins(cc.astype(np.float64), cd.astype(np.float64), idx, np.random.default_rng(1))
    idx = aiap_ref.fix_margins(xc.astype(np.float64), xd.astype(np.float64), idx, np.random.default_rng(2), rounds=0)
    both = _run_sets(idx, [(xc, xd), (cc, cd)], scales=[1.0, 100.0])
    only_xyz = _run_sets(idx, [(xc, xd), (cc, cd)], scales=[1.0, 0.0])
    only_cov = _run_sets(idx, [(xc, xd), (cc, cd)], scales=[0.0, 1.0])
    for k in (1, 2):
        assert torch.equal(both[0][k], only_xyz[0][k])
        ref = (100.0 * only_cov[1][k]).cpu().numpy().astype(np.float64)
        _close(both[1][k], ref, tol=1e-6, what="cov x100")
        assert not only_xyz[1][k].any()  # a zero upstream gradient gives zero gradients
    _, want_c, _ = aiap_ref.aiap(cc, cd, idx, g=100.0)
    _close(both[1][1], want_c, what="cov x100 against the restatement")


def test_bitwise_deterministic_with_a_hub():
    n = 200000
    xc, xd, idx = _random_case(n, 5, 3, seed=5, hub=12000)
    counts = np.bincount(idx[:, 1:].reshape(-1), minlength=n)
    assert counts[0] >= 10000
    r1 = _run_sets(idx, [(xc, xd)])[0]
    r2 = _run_sets(idx, [(xc, xd)])[0]
    assert r1[0] == r2[0]
    assert torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2])
    want_l, want_c, want_d = aiap_ref.aiap(xc, xd, idx)
    _close(r1[1], want_c, what="hub gxc")
    _close(r1[2], want_d, what="hub gxd")


def test_no_host_sync():
    class Gs(object):
        def __init__(self, xyz, cov):
            self.get_xyz, self._cov = xyz, cov

        def get_covariance(self):
            return self._cov

    xc, xd, _ = _random_case(20000, 5, 3, seed=7)
    cc, cd, _ = _random_case(20000, 5, 6, seed=8)
    leaves = [_leaf(x) for x in (xc, xd, cc, cd)]
    a = _fn()
    a.full_aiap_loss(Gs(leaves[0], leaves[2]), Gs(leaves[1], leaves[3]))  # warm-up: library load, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l_xyz, l_cov = a.full_aiap_loss(Gs(leaves[0], leaves[2]), Gs(leaves[1], leaves[3]))
        (1.0 * l_xyz + 100.0 * l_cov).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaves)


def test_bad_indices_counted_and_raised(monkeypatch):
    a = _fn()
    xc, xd, idx = _random_case(1000, 5, 3, seed=9)
    idx[3, 2], idx[7, 4] = -1, 1000
    idx[5, 0] = 12345  # column 0 is dropped whatever it holds: not counted
    t = torch.from_numpy(idx).to(DEV)
    loss = a.aiap_loss(_leaf(xc), _leaf(xd), nn_ix=t)  # (not in debug mode: no check, no sync)
    ok = (idx[:, 1:] >= 0) & (idx[:, 1:] < 1000)
    i, j = aiap_ref.pairs(idx)
    keep = ok.reshape(-1)
    ra, rb = np.sqrt(((xc[i[keep]].astype(np.float64) - xc[j[keep]]) ** 2).sum(1)), \
        np.sqrt(((xd[i[keep]].astype(np.float64) - xd[j[keep]]) ** 2).sum(1))
    want = np.abs(ra - rb).sum() / idx.shape[0] / 4  # bad pairs add nothing; the mean is still over N (K - 1)
    assert abs(float(loss) - want) <= 1e-6 * want
    monkeypatch.setattr(a, "_DEBUG", True)
    with pytest.raises(IndexError, match="2 neighbour indices"):
        a.aiap_loss(_leaf(xc), _leaf(xd), nn_ix=t)
