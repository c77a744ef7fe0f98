"""The hash-grid encoding (tinycudann.Encoding -> gsplat_mi355.hashgrid -> csrc/hashgrid.hip) on the GPU: forward and
backward parity with the float64 restatement tests/hashgrid_ref.py across block and list-length edges, bitwise
determinism with lists of N pairs and heavy hash collisions, other feature widths and level counts, every requires_grad
combination, fp64 and strided input, no host synchronisation, graph capture, and an end-to-end restatement of the
reference's HashGrid + AABB.normalize + MLP against a float64 twin built on the restatement's torch form."""
import numpy as np
import pytest
import torch

import hashgrid_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REF_CFG = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 16, "base_resolution": 16,
           "per_level_scale": float(np.exp(np.log(2048 / 16) / 15)), "max_resolution": 2048}


def _hg():
    from gsplat_mi355 import hashgrid
    return hashgrid


def _cfg(**kw):
    hg = _hg()
    return hg.parse_config(3, dict(REF_CFG, **kw))


def _points(n, seed):
    """[0, 1]^3 with exact 0.0 and 1.0 coordinates and a share in [-0.05, 1.05]^3 (float32)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    if n >= 4:
        x[0] = 0.0
        x[1] = 1.0
        x[2] = (0.0, 1.0, 0.5)
        out = rng.random(n) < 0.1
        out[:3] = False
        x[out] = rng.uniform(-0.05, 1.05, (int(out.sum()), 3)).astype(np.float32)
    return x


def _params(cfg, seed):
    n = _hg().levels(cfg)[3]
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def _run(cfg, x, params, G=None, want_x=True, want_p=True):
    hg = _hg()
    xt = torch.from_numpy(x).to(DEV).requires_grad_(want_x)
    pt = torch.from_numpy(params).to(DEV).requires_grad_(want_p)
    out = hg.hashgrid_encode(xt, pt, cfg)
    if G is not None:
        out.backward(torch.from_numpy(G).to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), xt.grad, pt.grad


def _close(got, want, tol, what):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, "%s: max err %.3g of max %.3g" % (what, err, scale)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097, 50000, 200000])
def test_forward_backward_parity(n):
    cfg = _cfg()
    table = _hg().levels(cfg)
    x = _points(n, n)
    params = _params(cfg, 1)
    G = np.random.default_rng(n + 1).normal(size=(n, 32)).astype(np.float32)
    out, gx, gp = _run(cfg, x, params, G)
    _close(out, ref.encode(x, params, table, 2), 1e-6, "out N=%d" % n)
    dx, dp = ref.backward(x, params, G, table, 2)
    _close(gx, dx, 1e-5, "dL/dx N=%d" % n)
    _close(gp, dp, 1e-5, "dL/dparams N=%d" % n)
    got = gp.cpu().numpy()
    assert np.array_equal(got == 0, dp == 0), "zero pattern of dL/dparams differs at N=%d" % n


def _twice(cfg, x, params, G):
    a = _run(cfg, x, params, G)
    b = _run(cfg, x, params, G)
    assert np.array_equal(a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "gradients differ between two backward passes"
    return a


@pytest.mark.parametrize("n", [3000, 120000])
def test_deterministic_one_cell(n):
    """Every point inside one level-0 cell: level 0's eight entries each get a list of N pairs (chunked beyond 1024)."""
    cfg = _cfg()
    table = _hg().levels(cfg)
    rng = np.random.default_rng(5)
    x = rng.uniform(0.51, 0.52, (n, 3)).astype(np.float32)
    params = _params(cfg, 2)
    G = rng.normal(size=(n, 32)).astype(np.float32)
    out, gx, gp = _twice(cfg, x, params, G)
    dx, dp = ref.backward(x, params, G, table, 2)
    _close(gx, dx, 1e-5, "dL/dx")
    _close(gp, dp, 1e-5, "dL/dparams")
    assert np.array_equal(gp.cpu().numpy() == 0, dp == 0)


def test_deterministic_collisions():
    """log2_hashmap_size 4: 16 rows per hashed level, lists of thousands of pairs from unrelated points."""
    cfg = _cfg(log2_hashmap_size=4)
    table = _hg().levels(cfg)
    n = 40000
    x = _points(n, 9)
    params = _params(cfg, 3)
    G = np.random.default_rng(10).normal(size=(n, 32)).astype(np.float32)
    out, gx, gp = _twice(cfg, x, params, G)
    _close(out, ref.encode(x, params, table, 2), 1e-6, "out")
    dx, dp = ref.backward(x, params, G, table, 2)
    _close(gx, dx, 1e-5, "dL/dx")
    _close(gp, dp, 1e-5, "dL/dparams")


@pytest.mark.parametrize("F,L", [(1, 16), (4, 16), (8, 8), (2, 1), (8, 1)])
def test_features_and_levels(F, L):
    cfg = _cfg(n_features_per_level=F, n_levels=L, log2_hashmap_size=14)
    table = _hg().levels(cfg)
    n = 3001
    x = _points(n, F * 100 + L)
    params = _params(cfg, F)
    G = np.random.default_rng(F).normal(size=(n, F * L)).astype(np.float32)
    out, gx, gp = _run(cfg, x, params, G)
    _close(out, ref.encode(x, params, table, F), 1e-6, "out")
    dx, dp = ref.backward(x, params, G, table, F)
    _close(gx, dx, 1e-5, "dL/dx")
    _close(gp, dp, 1e-5, "dL/dparams")
    assert np.array_equal(gp.cpu().numpy() == 0, dp == 0)


@pytest.mark.parametrize("want_x,want_p", [(True, True), (True, False), (False, True), (False, False)])
def test_requires_grad_combinations(want_x, want_p):
    cfg = _cfg()
    table = _hg().levels(cfg)
    n = 777
    x = _points(n, 4)
    params = _params(cfg, 4)
    G = np.random.default_rng(4).normal(size=(n, 32)).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(want_x)
    pt = torch.from_numpy(params).to(DEV).requires_grad_(want_p)
    out = _hg().hashgrid_encode(xt, pt, cfg)
    assert out.requires_grad == (want_x or want_p)
    if want_x or want_p:
        out.backward(torch.from_numpy(G).to(DEV))
    dx, dp = ref.backward(x, params, G, table, 2)
    if want_x:
        _close(xt.grad, dx, 1e-5, "dL/dx")
    else:
        assert xt.grad is None
    if want_p:
        _close(pt.grad, dp, 1e-5, "dL/dparams")
    else:
        assert pt.grad is None


def test_tcnn_encoding_fp64_strided_input_and_empty_batch():
    import tinycudann as tcnn
    enc = tcnn.Encoding(3, REF_CFG).to(DEV)
    cfg = enc.cfg
    table = _hg().levels(cfg)
    n = 1000
    x = _points(n, 12).astype(np.float64)
    big = torch.zeros(n, 7, dtype=torch.float64, device=DEV)
    big[:, 2:5] = torch.from_numpy(x).to(DEV)
    leaf = big.requires_grad_(True)
    xs = leaf[:, 2:5]  # non-contiguous fp64 view
    assert not xs.is_contiguous()
    out = enc(xs)
    assert out.dtype == torch.float32 and out.shape == (n, 32)
    G = np.random.default_rng(3).normal(size=(n, 32))
    out.backward(torch.from_numpy(G).float().to(DEV))
    params = enc.params.detach().cpu().numpy()
    x32 = x.astype(np.float32)
    _close(out, ref.encode(x32, params, table, 2), 1e-6, "out")
    dx, dp = ref.backward(x32, params, G.astype(np.float32), table, 2)
    assert leaf.grad.dtype == torch.float64
    _close(leaf.grad[:, 2:5], dx, 1e-5, "dL/dx")
    assert float(leaf.grad[:, :2].abs().max()) == 0.0
    _close(enc.params.grad, dp, 1e-5, "dL/dparams")
    # fp16 output: the fp32 result rounded once
    enc16 = tcnn.Encoding(3, REF_CFG, dtype=torch.float16).to(DEV)
    o16 = enc16(torch.from_numpy(x32).to(DEV))
    o32 = _hg().hashgrid_encode(torch.from_numpy(x32).to(DEV), enc16.params, cfg)
    assert o16.dtype == torch.float16 and torch.equal(o16, o32.half())
    # an empty batch
    e = torch.zeros(0, 3, device=DEV, requires_grad=True)
    oe = enc(e)
    assert oe.shape == (0, 32)
    enc.params.grad = None
    oe.sum().backward()
    assert float(enc.params.grad.abs().max()) == 0.0 and e.grad.shape == (0, 3)


def test_no_host_sync():
    import tinycudann as tcnn
    enc = tcnn.Encoding(3, REF_CFG).to(DEV)
    x = torch.rand(5000, 3, device=DEV, requires_grad=True)
    enc(x).square().sum().backward()  # warm-up
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enc(x).square().sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


def test_graph_capture_replays_bit_identical():
    """torch's whole-network recipe (as tests/test_gpu_capture.py): fresh leaves first used on the side stream, then
    captured on it (leaves used on the default stream first bind their autograd nodes to it, and a capture cannot wait
    for another stream)."""
    cfg = _cfg()
    n = 20000
    x0 = torch.from_numpy(_points(n, 21)).to(DEV)
    p0 = torch.from_numpy(_params(cfg, 21)).to(DEV)
    G = torch.randn(n, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))

    def step(x, p):
        out = _hg().hashgrid_encode(x, p, cfg)
        gx, gp = torch.autograd.grad((out * G).sum(), [x, p])
        return out, gx, gp

    eager = [t.detach().clone() for t in step(x0.clone().requires_grad_(True), p0.clone().requires_grad_(True))]
    xg, pg = x0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step(xg, pg)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(xg, pg)
    for _ in range(2):
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


class _AABB(torch.nn.Module):  # utils/dataset_utils.py AABB.normalize, restated
    def __init__(self, cmax, cmin, dtype):
        super().__init__()
        self.register_buffer("coord_max", torch.tensor(cmax, dtype=dtype))
        self.register_buffer("coord_min", torch.tensor(cmin, dtype=dtype))

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1.0 if sym else x


class _Deformer(torch.nn.Module):
    """models/network_utils.py HashGrid ((x + 1) / 2 into the encoding) + a small torch MLP, as the reference's
    HashGridwithMLP.forward uses them: xyz -> AABB.normalize(sym) -> encoding -> MLP(feature, cond) -> deltas."""

    def __init__(self, encode, n_feat, dtype, seed=0):
        super().__init__()
        self.encode = encode
        g = torch.Generator().manual_seed(seed)
        self.l0 = torch.nn.Linear(n_feat + 4, 64).to(dtype)
        self.l1 = torch.nn.Linear(64, 10).to(dtype)
        with torch.no_grad():
            for m in (self.l0, self.l1):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)

    def forward(self, xyz, aabb, cond):
        x = aabb.normalize(xyz, sym=True)
        feat = self.encode((x + 1.0) * 0.5)
        h = torch.nn.functional.softplus(self.l0(torch.cat([feat, cond.expand(xyz.shape[0], -1)], 1)))
        return self.l1(h)


def test_end_to_end_against_float64_twin():
    import tinycudann as tcnn
    n = 3000
    rng = np.random.default_rng(7)
    cmin, cmax = [-0.5, -1.0, -0.25], [0.5, 1.0, 0.75]  # power-of-two extents: the normalisation is exact in fp32
    xyz0 = (rng.integers(0, 1024, (n, 3)) / 1024.0 * (np.array(cmax) - cmin) + cmin).astype(np.float32)
    cond = rng.normal(size=(1, 4))
    R = rng.normal(size=(n, 10))

    enc = tcnn.Encoding(3, REF_CFG, seed=3)
    with torch.no_grad():
        enc.params.mul_(5000.0)  # table values of order 0.5: the gradients reach the MLP and xyz in earnest
    model = _Deformer(enc, 32, torch.float32).to(DEV)
    aabb = _AABB(cmax, cmin, torch.float32).to(DEV)
    xyz = torch.from_numpy(xyz0).to(DEV).requires_grad_(True)
    d = model(xyz, aabb, torch.from_numpy(cond).float().to(DEV))
    loss = ((xyz + d[:, :3]) * torch.from_numpy(R[:, :3]).float().to(DEV)).sum() + \
        (d[:, 3:] * torch.from_numpy(R[:, 3:]).float().to(DEV)).sum()
    loss.backward()

    cfg = enc.cfg
    table = _hg().levels(cfg)
    p64 = torch.nn.Parameter(enc.params.detach().double().clone())
    twin = _Deformer(lambda x: ref.encode_torch(x, p64, table, 2), 32, torch.float64).to(DEV)
    twin.p64 = p64
    aabb64 = _AABB(cmax, cmin, torch.float64).to(DEV)
    xyz64 = torch.from_numpy(xyz0.astype(np.float64)).to(DEV).requires_grad_(True)
    d64 = twin(xyz64, aabb64, torch.from_numpy(cond).to(DEV))
    loss64 = ((xyz64 + d64[:, :3]) * torch.from_numpy(R[:, :3]).to(DEV)).sum() + \
        (d64[:, 3:] * torch.from_numpy(R[:, 3:]).to(DEV)).sum()
    loss64.backward()

    pairs = [("params", enc.params.grad, p64.grad), ("xyz", xyz.grad, xyz64.grad)]
    for name in ("l0", "l1"):
        for a in ("weight", "bias"):
            pairs.append((name + "." + a, getattr(getattr(model, name), a).grad, getattr(getattr(twin, name), a).grad))
    for name, got, want in pairs:
        _close(got, want.cpu().numpy(), 1e-5, name)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = enc.params.detach().clone()
    opt.step()
    assert not torch.equal(before, enc.params.detach())
    assert torch.isfinite(enc.params).all()
