"""Linear blend skinning (gsplat_mi355.skinning -> csrc/skinning.hip) on the GPU: parity with the reference's own fp32 and
fp64 results (tests/golden/skinning.npz), sizes from 0 to 1.1 M across block and reduction edges against the float64
restatement tests/skinning_ref.py, row independence, bitwise determinism of every gradient, exact one-hot blends,
partial requires_grad, extreme logits, no host synchronisation, graph capture and an end-to-end SkinningField.forward
with a real MLP against the same chain in plain torch."""
import os

import numpy as np
import pytest
import torch

import skinning_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5  # no element beyond 1e-5 of its tensor's largest magnitude
KIND_W = {"hierarchical": 25, "softmax": 24, "weights": 24}


def _sk():
    from gsplat_mi355 import skinning
    return skinning


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "skinning.npz"))


def _close(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert np.isfinite(got).all() and err <= BAR, "%s: %.3g of the largest magnitude" % (what, err)


def _run(w, tfs, xyz, rot, kind, g, G, need=(True, True, True, True)):
    """Fused forward and backward on the GPU: (xbar, Rbar, T, {name: grad})."""
    leaves = [torch.as_tensor(a).to(DEV).requires_grad_(r) for a, r in zip((w, tfs, xyz, rot), need)]
    xb, Rb, T = _sk().linear_blend_skinning(*leaves, weights=kind == "weights")
    out = {}
    if any(need):
        loss = (xb * torch.as_tensor(g).to(DEV)).sum() + (Rb * torch.as_tensor(G).to(DEV)).sum()
        wanted = [l for l in leaves if l.requires_grad]
        grads = iter(torch.autograd.grad(loss, wanted))
        for name, leaf in zip(("dw", "dtfs", "dxyz", "drot"), leaves):
            if leaf.requires_grad:
                out[name] = next(grads)
    return xb, Rb, T, out


def _inputs(n, kind, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    if kind == "weights":
        w = rng.dirichlet(np.full(24, 0.3), size=n).astype(np.float32)
    else:
        w = rng.normal(scale=scale, size=(n, KIND_W[kind])).astype(np.float32)
    tfs = np.zeros((24, 4, 4), np.float32)
    tfs[:] = np.eye(4) + rng.normal(scale=0.3, size=(24, 4, 4))
    tfs[:, 3] = (0, 0, 0, 1)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4))
    rot = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)
    g = rng.normal(size=(n, 3)).astype(np.float32)
    G = rng.normal(size=(n, 3, 3)).astype(np.float32)
    return w, tfs, xyz, rot, g, G


@pytest.mark.parametrize("case", "abcde")
def test_fixture_parity(fx, case):
    p = case + "/"
    kind = str(fx[p + "kind"])
    xb, Rb, T, grads = _run(fx[p + "w"], fx[p + "tfs"], fx[p + "xyz"], fx[p + "rot"], kind, fx[p + "g"], fx[p + "G"])
    got = dict(xbar=xb, Rbar=Rb, T=T, **grads)
    for prec in ("f32", "f64"):
        for name, v in got.items():
            _close(v, fx["%s%s_%s" % (p, name, prec)], "%s %s vs %s" % (case, name, prec))


def test_fixture_parity_hierarchical_softmax(fx):
    x = torch.from_numpy(fx["f/x"]).to(DEV).requires_grad_(True)
    W = _sk().hierarchical_softmax(x)
    (dx,) = torch.autograd.grad((W * torch.from_numpy(fx["f/gW"]).to(DEV)).sum(), [x])
    for prec in ("f32", "f64"):
        _close(W, fx["f/W_" + prec], "W vs " + prec)
        _close(dx, fx["f/dx_" + prec], "dx vs " + prec)


# block edges (256 rows), thirds of a block, and block counts around multiples of 64 (the dtfs reduction's lane runs)
SIZES = [0, 1, 63, 64, 65, 85, 86, 87, 255, 256, 257, 511, 513, 64 * 256 - 1, 64 * 256 + 1, 65 * 256 + 7, 128 * 256 + 255]


@pytest.mark.parametrize("kind", ["hierarchical", "softmax", "weights"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_restatement(n, kind):
    w, tfs, xyz, rot, g, G = _inputs(n, kind, seed=n + 7)
    xb, Rb, T, grads = _run(w, tfs, xyz, rot, kind, g, G)
    want = ref.forward_backward(w, tfs, xyz, rot, kind, g, G)
    assert tuple(xb.shape) == (n, 3) and tuple(Rb.shape) == (n, 3, 3) and tuple(T.shape) == (n, 4, 4)
    if n == 0:
        assert not grads["dtfs"].any() and grads["dw"].shape == (0, KIND_W[kind])
        return
    for name, v in dict(xbar=xb, Rbar=Rb, T=T, **grads).items():
        _close(v, want[name], "%s n=%d %s" % (kind, n, name))


@pytest.mark.parametrize("n", [200000, 1100000])
def test_large_against_restatement(n):
    w, tfs, xyz, rot, g, G = _inputs(n, "hierarchical", seed=3)
    xb, Rb, T, grads = _run(w, tfs, xyz, rot, "hierarchical", g, G)
    want = ref.forward_backward(w, tfs, xyz, rot, "hierarchical", g, G)
    for name, v in dict(xbar=xb, Rbar=Rb, T=T, **grads).items():
        _close(v, want[name], "n=%d %s" % (n, name))


@pytest.mark.parametrize("kind", ["hierarchical", "softmax", "weights"])
def test_row_results_do_not_depend_on_the_batch(kind):
    n, r = 200000, 199999
    w, tfs, xyz, rot, g, G = _inputs(n, kind, seed=11)
    big = _run(w, tfs, xyz, rot, kind, g, G)
    one = _run(w[r:r + 1], tfs, xyz[r:r + 1], rot[r:r + 1], kind, g[r:r + 1], G[r:r + 1])
    for a, b in zip(big[:3], one[:3]):
        assert torch.equal(a[r:r + 1], b)
    for name in ("dw", "dxyz", "drot"):
        assert torch.equal(big[3][name][r:r + 1], one[3][name]), name


@pytest.mark.parametrize("kind", ["hierarchical", "softmax", "weights"])
def test_backward_is_bitwise_reproducible(kind):
    w, tfs, xyz, rot, g, G = _inputs(300000, kind, seed=5)
    first = _run(w, tfs, xyz, rot, kind, g, G)[3]
    second = _run(w, tfs, xyz, rot, kind, g, G)[3]
    for name in first:
        assert torch.equal(first[name], second[name]), name


def test_one_hot_weights_give_the_bone_transform_exactly():
    rng = np.random.default_rng(1)
    n = 1000
    j = rng.integers(24, size=n)
    w = np.eye(24, dtype=np.float32)[j]
    _, tfs, xyz, rot, _, _ = _inputs(n, "weights", seed=2)
    tfs[:, 3] = rng.normal(size=(24, 4))
    _, _, T, _ = _run(w, tfs, xyz, rot, "weights", None, None, need=(False,) * 4)
    assert torch.equal(T, torch.from_numpy(tfs[j]).to(DEV))


@pytest.mark.parametrize("need", [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                                  (False, False, False, True), (False, True, True, False), (True, False, False, True)])
def test_partial_requires_grad(need):
    w, tfs, xyz, rot, g, G = _inputs(5000, "hierarchical", seed=17)
    want = ref.forward_backward(w, tfs, xyz, rot, "hierarchical", g, G)
    _, _, _, grads = _run(w, tfs, xyz, rot, "hierarchical", g, G, need=need)
    assert sorted(grads) == sorted(n for n, r in zip(("dw", "dtfs", "dxyz", "drot"), need) if r)
    for name, v in grads.items():
        _close(v, want[name], name)


def test_only_one_upstream_gradient():
    w, tfs, xyz, rot, g, G = _inputs(3000, "softmax", seed=19)
    leaves = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (w, tfs, xyz, rot)]
    xb, Rb, _ = _sk().linear_blend_skinning(*leaves)
    got = torch.autograd.grad((xb * torch.from_numpy(g).to(DEV)).sum(), leaves)
    want = ref.forward_backward(w, tfs, xyz, rot, "softmax", g, None)
    for name, v in zip(("dw", "dtfs", "dxyz", "drot"), got):
        _close(v, want[name], name)
    assert not got[3].any()  # the rotation sees no gradient without G


def test_extreme_logits_stay_finite():
    for kind in ("hierarchical", "softmax"):
        w, tfs, xyz, rot, g, G = _inputs(4096, kind, seed=23)
        w = np.sign(w) * 1000.0
        w[::7] = -1000.0
        w[1::7] = 1000.0
        xb, Rb, T, grads = _run(w.astype(np.float32), tfs, xyz, rot, kind, g, G)
        want = ref.forward_backward(w, tfs, xyz, rot, kind, g, G)
        for name, v in dict(xbar=xb, Rbar=Rb, T=T, **grads).items():
            assert torch.isfinite(v).all(), (kind, name)
            _close(v, want[name], "%s %s" % (kind, name))


def test_weights_alone_match_restatement():
    for kind, fn in (("hierarchical", _sk().hierarchical_softmax), ("softmax", _sk().skinning_softmax)):
        for n in (1, 255, 257, 100000):
            rng = np.random.default_rng(n)
            x = rng.normal(scale=3.0, size=(n, KIND_W[kind])).astype(np.float32)
            gW = rng.normal(size=(n, 24)).astype(np.float32)
            xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
            W = fn(xt)
            (dx,) = torch.autograd.grad((W * torch.from_numpy(gW).to(DEV)).sum(), [xt])
            Wr, dxr = ref.weights_forward_backward(x, kind, gW)
            _close(W, Wr, "%s W n=%d" % (kind, n))
            _close(dx, dxr, "%s dx n=%d" % (kind, n))
    assert torch.equal(_sk().skinning_softmax(torch.zeros(4, 25, device=DEV)),
                       _sk().hierarchical_softmax(torch.zeros(4, 25, device=DEV)))
    with pytest.raises(TypeError):
        _sk().skinning_softmax(torch.zeros(4, 25, device=DEV, dtype=torch.float64))


def test_strided_inputs():
    w, tfs, xyz, rot, g, G = _inputs(2000, "hierarchical", seed=29)
    want = ref.forward_backward(w, tfs, xyz, rot, "hierarchical", g, G)
    big = torch.zeros(2000, 40, device=DEV)
    big[:, 3:28] = torch.from_numpy(w).to(DEV)
    wv = big[:, 3:28].requires_grad_(False)
    xyz_t = torch.from_numpy(np.ascontiguousarray(xyz.T)).to(DEV).t()
    xb, Rb, T = _sk().linear_blend_skinning(wv, torch.from_numpy(tfs).to(DEV), xyz_t, torch.from_numpy(rot).to(DEV))
    _close(xb, want["xbar"], "xbar")
    _close(Rb, want["Rbar"], "Rbar")


def test_no_host_sync():
    w, tfs, xyz, rot, g, G = _inputs(20000, "hierarchical", seed=31)
    leaves = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (w, tfs, xyz, rot)]
    gt, Gt = torch.from_numpy(g).to(DEV), torch.from_numpy(G).to(DEV)
    sk = _sk()

    def step():
        xb, Rb, _ = sk.linear_blend_skinning(*leaves)
        ((xb * gt).sum() + (Rb * Gt).sum() + sk.hierarchical_softmax(leaves[0]).square().sum()).backward()

    step()  # warm-up: library load, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaves)


def test_graph_capture_replays_bit_identical():
    """torch's whole-network recipe (as tests/test_gpu_capture.py): fresh leaves first used on the side stream, then
    captured on it."""
    w, tfs, xyz, rot, g, G = _inputs(20000, "hierarchical", seed=37)
    gt, Gt = torch.from_numpy(g).to(DEV), torch.from_numpy(G).to(DEV)
    sk = _sk()

    def step(leaves):
        xb, Rb, T = sk.linear_blend_skinning(*leaves)
        grads = torch.autograd.grad((xb * gt).sum() + (Rb * Gt).sum(), leaves)
        return (xb, Rb, T) + tuple(grads)

    fresh = lambda: [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (w, tfs, xyz, rot)]
    eager = [t.detach().clone() for t in step(fresh())]
    leaves = fresh()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step(leaves)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(leaves)
    for _ in range(2):
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


class _AABB(object):  # utils/dataset_utils.py AABB.normalize, restated
    def __init__(self, cmax, cmin):
        self.coord_max, self.coord_min = cmax, cmin

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1.0 if sym else x


class _Gaussians(object):
    def __init__(self, xyz, rotation):
        self._xyz, self._rotation = xyz, rotation

    @property
    def get_xyz(self):
        return self._xyz

    def clone(self):
        return _Gaussians(self._xyz, self._rotation)

    def set_fwd_transform(self, T):
        self.fwd_transform = T


def _mlp(seed):
    """VanillaCondMLP's shape for the skinning network: 3 -> 128 x 4 -> 25, LeakyReLU."""
    torch.manual_seed(seed)
    layers, d = [], 3
    for _ in range(4):
        layers += [torch.nn.Linear(d, 128), torch.nn.LeakyReLU()]
        d = 128
    layers.append(torch.nn.Linear(d, 25))
    return torch.nn.Sequential(*layers).to(DEV)


def test_skinning_field_forward_end_to_end():
    n = 50000
    w, tfs, xyz, rot, g, G = _inputs(n, "hierarchical", seed=41)
    mlp = _mlp(0)
    aabb = _AABB(torch.tensor([1.0, 2.0, 1.0], device=DEV), torch.tensor([-1.0, -1.5, -1.2], device=DEV))
    field = type("Field", (), {})()
    field.aabb, field.lbs_network, field.distill = aabb, mlp, False
    gt, Gt = torch.from_numpy(g).to(DEV), torch.from_numpy(G).to(DEV)

    def run(fused):
        mlp.zero_grad()
        x = torch.from_numpy(xyz).to(DEV).requires_grad_(True)
        q = torch.from_numpy(rot).to(DEV).requires_grad_(True)
        tf = torch.from_numpy(tfs).to(DEV).requires_grad_(True)
        camera = type("Camera", (), {})()
        camera.bone_transforms = tf
        gs = _Gaussians(x, q)
        if fused:
            d = _sk().skinning_field_forward(field, gs, 0, camera)
        else:  # the same statement sequence in plain torch
            logits = mlp(aabb.normalize(x, sym=True))
            xb, Rb, T = ref.skinning(logits, tf, x, q, "hierarchical")
            d = gs.clone()
            d.set_fwd_transform(T.detach())
            d._xyz, d.rotation_precomp = xb, Rb
        assert not d.fwd_transform.requires_grad
        ((d._xyz * gt).sum() + (d.rotation_precomp * Gt).sum()).backward()
        out = {"xbar": d._xyz, "Rbar": d.rotation_precomp, "T": d.fwd_transform, "dxyz": x.grad, "drot": q.grad,
               "dtfs": tf.grad}
        out.update({"p%d" % k: p.grad.clone() for k, p in enumerate(mlp.parameters())})
        return {k: v.detach().double().cpu().numpy() for k, v in out.items()}

    got, want = run(True), run(False)
    for name in want:
        _close(got[name], want[name], name)
