"""The skinning regulariser (gsplat_mi355.skinning MeshSampler / skinning_mse_loss / skinning_loss -> csrc/skinloss.hip) on
the GPU: the sampler against the float64 restatement tests/skinning_loss_ref.py at block edges on three meshes with
hand-made draws at every decision's edge, the distribution of the default draws, the loss and its gradient against the
reference's own fp32 and fp64 results (tests/golden/skinning_loss.npz) and against the restatement, bitwise
reproducibility, an end-to-end SkinningField.get_skinning_loss with a real MLP, no host synchronisation and graph capture.

Tolerances.  Sampler: 1e-6 absolute on meshes within the unit cube (a few fp32 operations on values of magnitude at most
1).  Loss: tests/test_gpu_skinning.py grants the activation BAR = 1e-5 of W's largest magnitude (at most 1), so
sum_j (W_j - t_j)^2 may move by 2 BAR sum_j |W_j - t_j| per row, and the fp32 sum of 24 terms by 24 ulp: the loss gets
2 BAR S + 2e-6 loss with S the mean over rows of sum_j |W_j - t_j| (from the restatement).  Gradient: dW = 2 g (W - t) / n
inherits W's error, 2 g BAR / n absolute, the activation's reverse (entries of magnitude at most 1) is granted the same
relative to its input's scale, and passing dW's error through it adds as much again: 3 BAR (2 g / n) absolute."""
import os

import numpy as np
import pytest
import torch

import skinning_loss_ref as ref
import skinning_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
SAMPLE_TOL = 1e-6
SIZES = [1, 255, 256, 257, 1024, 1025]
LO, HI = np.zeros(3, np.float32), np.ones(3, np.float32)


def _sk():
    from gsplat_mi355 import skinning
    return skinning


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "skinning_loss.npz"))


_SAMPLERS = {}


def _sampler(mesh):
    if mesh not in _SAMPLERS:
        v, f, w = getattr(ref, mesh)()
        _SAMPLERS[mesh] = (v, f, w, _sk().MeshSampler(v, f, w, LO, HI, DEV))
    return _SAMPLERS[mesh]


def _ulp(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(2.0 if k > 0 else -1.0), dtype=np.float32)
    return x


def _special_draws(cdf):
    """Rows at the edges of every decision: (u0, a, b).  Returns the rows and how many of them put u0 * cdf[F-1] exactly
    on a cdf value below the total."""
    total = cdf[-1]
    u0s = [np.float32(0.0), _ulp(1.0, -1)]
    hits = 0
    for i in sorted(set([0, len(cdf) // 2 - 1, len(cdf) // 2, len(cdf) - 2]) & set(range(len(cdf) - 1))):
        c = np.float32(np.float64(cdf[i]) / np.float64(total))
        for k in range(-2, 3):  # the quotient and its neighbours: below, on (where fp32 allows) and above cdf[i]
            u = _ulp(c, k)
            if 0.0 <= u < 1.0:
                u0s.append(u)
                hits += int(np.float32(u * total) == cdf[i])
    ab = [(0.25, 0.75), (0.5, 0.5), (0.5, _ulp(0.5, 1)), (0.75, _ulp(0.25, 1)), (0.6, _ulp(0.4, 3)), (0.9, 0.9), (0.0, 0.0),
          (_ulp(1.0, -1), _ulp(1.0, -1)), (0.0, _ulp(1.0, -1)), (1.0 / 3, 1.0 / 3)]
    rows = [(u, 0.3, 0.2) for u in u0s] + [(0.37, a, b) for a, b in ab]
    return np.array(rows, np.float32), hits


def _draws(n, cdf, seed):
    d = np.random.default_rng(seed).random((n, 3), dtype=np.float32)
    special, hits = _special_draws(cdf)
    if n > len(special):
        d[n - len(special):] = special  # the last rows: the tail of the last block
    return d, special, hits


def _check_samples(mesh, draws):
    v, f, w, s = _sampler(mesh)
    cdf = s.cdf.cpu().numpy()
    n = len(draws)
    pn, tg, face, bary, pts = s.sample(n, draws=torch.from_numpy(draws).to(DEV), return_index=True)
    assert tuple(pn.shape) == (n, 3) and tuple(tg.shape) == (n, 24) and tuple(face.shape) == (n,) and face.dtype == torch.int32
    pn2, tg2 = s.sample(n, draws=torch.from_numpy(draws).to(DEV))  # without the optional outputs: the same bits
    assert torch.equal(pn, pn2) and torch.equal(tg, tg2)
    want = ref.sample(v, f, cdf, w, LO, HI, draws)
    assert np.array_equal(face.cpu().numpy().astype(np.int64), want["face"]), mesh
    assert np.abs(want["bary"] - want["bary_geo"]).max() <= 1e-9  # (1 - a - b, a, b) are the point's coordinates
    for name, got in (("points", pts), ("bary", bary), ("points_norm", pn), ("target", tg)):
        err = float(np.abs(got.double().cpu().numpy() - want[name]).max())
        print("%s n=%d %s: %.3g" % (mesh, n, name, err))
        assert torch.isfinite(got).all() and err <= SAMPLE_TOL, "%s n=%d %s: %.3g" % (mesh, n, name, err)
    return want


@pytest.mark.parametrize("mesh", ["triangle", "tetrahedron_with_degenerate_face", "sphere"])
@pytest.mark.parametrize("n", SIZES)
def test_sampler_against_restatement(n, mesh):
    cdf = _sampler(mesh)[3].cdf.cpu().numpy()
    draws, special, hits = _draws(n, cdf, seed=n)
    if mesh != "triangle":
        assert hits >= 1  # some u0 lands exactly on a cdf value
    runs = [draws] + ([special] if n <= len(special) else [])
    for d in runs:
        want = _check_samples(mesh, d)
        if mesh == "tetrahedron_with_degenerate_face":
            assert (want["face"] != 2).all()  # the zero-area face is never chosen
    if mesh == "tetrahedron_with_degenerate_face" and n > len(special):
        # on either side of the zero-area face: its predecessor on the exact hit and below, its successor above
        assert {1, 3} <= set(want["face"][n - len(special):].tolist())


def test_sampler_default_draws_distribution():
    """Two triangles of area 1 : 3 and 65 536 seeded torch.rand draws: the small face's share within 5 binomial standard
    deviations of 1/4, each triangle's mean barycentric coordinates within 5 standard deviations of 1/3 (a coordinate of a
    uniform point of a triangle has variance 1/18)."""
    v, f, w, s = _sampler("two_triangles")
    n = 65536
    gen = torch.Generator(device=DEV).manual_seed(1234)
    pn, tg, face, bary, pts = s.sample(n, generator=gen, return_index=True)
    face, bary = face.cpu().numpy(), bary.double().cpu().numpy()
    share = float((face == 0).mean())
    assert abs(share - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / n), share
    assert bary.min() >= -1e-6 and np.abs(bary.sum(1) - 1).max() <= 1e-6
    for k in (0, 1):
        m = int((face == k).sum())
        mean = bary[face == k].mean(0)
        assert np.abs(mean - 1.0 / 3).max() <= 5 * np.sqrt(1.0 / 18 / m), (k, mean)
    gen.manual_seed(1234)
    again = s.sample(n, generator=gen)
    assert torch.equal(again[0], pn) and torch.equal(again[1], tg)
    assert not torch.equal(s.sample(n)[0], s.sample(n)[0])  # the default generator moves on


def _inputs(n, width, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(scale=scale, size=(n, width)).astype(np.float32)
    rows = rng.dirichlet(np.full(24, 0.1), size=(n, 3))
    t = (rows * rng.dirichlet(np.ones(3), size=n)[:, :, None]).sum(1).astype(np.float32)
    return x, t


def _run(x, t, g=1.0):
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss = _sk().skinning_mse_loss(xt, torch.from_numpy(t).to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (dx,) = torch.autograd.grad(loss * g, [xt])
    return loss, dx


def _check_loss(x, t, g, what, loss, dx):
    n = x.shape[0]
    want_loss, want_dx = ref.loss_and_grad(x, t, g)
    kind = "hierarchical" if x.shape[1] == 25 else "softmax"
    W = skinning_ref.weights(torch.from_numpy(x.astype(np.float64)), kind).numpy()
    S = float(np.abs(W - t.astype(np.float64)).sum(1).mean())
    loss = loss.detach()
    err = abs(float(loss) - want_loss)
    tol = 2 * BAR * S + 2e-6 * want_loss
    print("%s: loss %.9g, off by %.3g (granted %.3g)" % (what, float(loss), err, tol))
    assert np.isfinite(float(loss)) and err <= tol, "%s: loss off by %.3g > %.3g" % (what, err, tol)
    err = float(np.abs(dx.double().cpu().numpy() - want_dx).max())
    tol = 3 * BAR * 2 * abs(g) / n
    print("%s: dlogits off by %.3g (granted %.3g)" % (what, err, tol))
    assert torch.isfinite(dx).all() and err <= tol, "%s: dlogits off by %.3g > %.3g" % (what, err, tol)


@pytest.mark.parametrize("case", "abcd")
def test_fixture_parity(fx, case):
    x, t = fx[case + "/logits"], fx[case + "/target"]
    loss, dx = _run(x, t)
    _check_loss(x, t, 1.0, "case " + case, loss, dx)
    n = x.shape[0]
    for prec in ("f32", "f64"):  # the reference's own results, under the same bounds
        want = float(fx["%s/loss_%s" % (case, prec)])
        assert abs(float(loss) - want) <= 2 * BAR * 2 + 2e-6 * want, (case, prec)  # S <= 2: two rows that sum to one
        assert np.abs(dx.double().cpu().numpy() - fx["%s/dlogits_%s" % (case, prec)]).max() <= 3 * BAR * 2 / n, (case, prec)


@pytest.mark.parametrize("width", [25, 24])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_restatement(n, width):
    x, t = _inputs(n, width, seed=100 + n)
    loss, dx = _run(x, t)
    _check_loss(x, t, 1.0, "n=%d C=%d" % (n, width), loss, dx)


@pytest.mark.parametrize("width", [25, 24])
def test_empty(width):
    x = torch.zeros(0, width, device=DEV, requires_grad=True)
    loss = _sk().skinning_mse_loss(x, torch.zeros(0, 24, device=DEV))
    (dx,) = torch.autograd.grad(loss, [x])
    assert float(loss) == 0.0 and tuple(dx.shape) == (0, width)


@pytest.mark.parametrize("width", [25, 24])
def test_saturated_logits_stay_finite(width):
    x, t = _inputs(1025, width, seed=7)
    x = (np.sign(x) * 1000.0).astype(np.float32)
    x[::7] = -1000.0
    x[1::7] = 1000.0
    x[2::7] *= 0.03  # |x| = 30: 1 - sigmoid rounds to 0 in fp32, exp does not underflow
    loss, dx = _run(x, t)
    _check_loss(x, t, 1.0, "saturated C=%d" % width, loss, dx)


@pytest.mark.parametrize("width", [25, 24])
def test_upstream_gradient_is_honoured(width):
    x, t = _inputs(777, width, seed=9)
    loss, dx = _run(x, t, g=3.0)
    _check_loss(x, t, 3.0, "3 * loss C=%d" % width, loss, dx)
    _, dx1 = _run(x, t, g=1.0)
    assert not torch.equal(dx, dx1)
    assert float((dx - 3 * dx1).abs().max()) <= 3 * BAR * 2 * 3 / 777


def test_nothing_is_launched_backward_without_a_gradient_to_the_logits():
    from gsplat_mi355 import _lib
    x, t = _inputs(300, 25, seed=11)
    other = torch.ones(5, device=DEV, requires_grad=True)
    tt = torch.from_numpy(t).to(DEV).requires_grad_(True)  # the target never gets a gradient
    seen = {}
    for grad in (False, True):
        xt = torch.from_numpy(x).to(DEV).requires_grad_(grad)
        torch.cuda.synchronize()
        _lib.profile_collect()  # (forget what earlier tests left)
        _lib.profile_enable(True)
        try:
            loss = _sk().skinning_mse_loss(xt, tt)
            (3 * loss + other.square().sum()).backward()
            torch.cuda.synchronize()
            seen[grad] = _lib.profile_collect()
        finally:
            _lib.profile_enable(False)
        assert (xt.grad is not None) == grad and tt.grad is None and other.grad is not None
    assert "skin_loss" in seen[False] and "skin_loss_bwd" not in seen[False]
    assert seen[True]["skin_loss_bwd"][1] == 1 and seen[True]["skin_loss"][1] == 1


@pytest.mark.parametrize("width", [25, 24])
def test_bitwise_reproducible(width):
    x, t = _inputs(1024, width, seed=13)
    first, second = _run(x, t), _run(x, t)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    # a row's gradient does not depend on the batch around it, apart from the factor 1 / n: with g = n it is gone
    _, big = _run(x, t, g=1024.0)
    _, small = _run(x[:256], t[:256], g=256.0)
    assert torch.equal(big[:256], small)


# ---- end to end: SkinningField.get_skinning_loss with a real skinning MLP
class _AABB(object):  # utils/dataset_utils.py AABB, what get_skinning_loss reads of it
    def __init__(self, cmax, cmin):
        self.coord_max, self.coord_min = cmax, cmin


class _Net(torch.nn.Module):
    """What VanillaCondMLP.__init__ leaves on the module for the skinning network (3 -> 128 x 4 -> 25, LeakyReLU), with
    mlp_forward as the forward."""

    def __init__(self, seed, dtype=torch.float32):
        super().__init__()
        torch.manual_seed(seed)
        self.config = dict(multires=0, skip_in=[], cond_in=[], n_neurons=128, n_hidden_layers=4)
        self.num_layers, self.embed_fn = 6, None
        dims = [3, 128, 128, 128, 128, 25]
        for l in range(5):
            setattr(self, "lin%d" % l, torch.nn.Linear(dims[l], dims[l + 1]))
        self.activation = torch.nn.LeakyReLU()
        self.to(device=DEV, dtype=dtype)

    def forward(self, coords, cond=None):
        from gsplat_mi355 import mlp
        return mlp.mlp_forward(self, coords, cond=cond)

    def plain(self, coords):
        h = coords
        for l in range(5):
            h = getattr(self, "lin%d" % l)(h)
            if l < 4:
                h = torch.nn.functional.leaky_relu(h, 0.01)
        return h


def _field(seed=0):
    from gsplat_mi355 import mlp
    v, f, w = ref.sphere()
    field = type("Field", (), {})()
    field.smpl_verts, field.faces, field.skinning_weights = v, f, w
    field.aabb = _AABB(torch.tensor([1.1, 1.2, 1.05], device=DEV), torch.tensor([-0.1, -0.2, -0.05], device=DEV))
    field.lbs_network, field.distill = _Net(seed), False
    field.cfg = type("Cfg", (), {"n_reg_pts": 1024})()
    assert mlp.mlp_supported(field.lbs_network)
    return field


def test_skinning_loss_end_to_end():
    """skinning_loss(field, draws) against the restatement run through the same parameters in float64.  Bounds: the MLP is
    granted BAR of its output's largest magnitude (tests/test_gpu_mlp.py), so W moves by BAR (1 + max |logits|) and the
    loss by 2 S times that; a parameter gradient passes the sampler (1e-6, a tenth of BAR), the MLP forward, the loss
    gradient (3 BAR, above) and the MLP backward, each granted BAR of the largest magnitude: 5 BAR of its own."""
    field = _field()
    draws = np.random.default_rng(5).random((1025, 3), dtype=np.float32)
    with pytest.raises(NotImplementedError):
        field.distill = True
        _sk().skinning_loss(field, draws=torch.from_numpy(draws).to(DEV))
    field.distill = False
    loss = _sk().skinning_loss(field, draws=torch.from_numpy(draws).to(DEV))
    sampler = field._gsplat_mesh_sampler
    loss.backward()
    assert _sk().skinning_loss(field, draws=torch.from_numpy(draws).to(DEV)) is not None and field._gsplat_mesh_sampler is sampler
    twin = _Net(0, dtype=torch.float64)
    twin.load_state_dict({k: p.double() for k, p in field.lbs_network.state_dict().items()})
    s = ref.sample(field.smpl_verts, field.faces, sampler.cdf.cpu().numpy(), field.skinning_weights,
                   field.aabb.coord_min.cpu().numpy(), field.aabb.coord_max.cpu().numpy(), draws)
    logits = twin.plain(torch.from_numpy(s["points_norm"]).to(DEV))
    target = torch.from_numpy(s["target"]).to(DEV)
    want = ref.loss_torch(logits, target)
    want.backward()
    W = skinning_ref.weights(logits.detach(), "hierarchical")
    S = float((W - target).abs().sum(1).mean())
    err, tol = abs(float(loss) - float(want)), 2 * S * BAR * (1 + float(logits.abs().max())) + 2e-6 * float(want)
    print("loss %.9g, off by %.3g (granted %.3g)" % (float(loss), err, tol))
    assert err <= tol
    for (name, p), q in zip(field.lbs_network.named_parameters(), twin.parameters()):
        scale = float(q.grad.abs().max())
        err = float((p.grad.double() - q.grad).abs().max()) / scale
        print("%s: %.3g of the largest magnitude" % (name, err))
        assert torch.isfinite(p.grad).all() and err <= 5 * BAR, name
    # the default path: n_reg_pts samples from torch.rand
    assert float(_sk().skinning_loss(field)) > 0


def test_no_host_sync():
    field = _field(1)
    params = list(field.lbs_network.parameters())

    def step():
        _sk().skinning_loss(field).backward()

    step()  # warm-up: library load, the sampler's buffers, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)


def _capture(step):
    """torch's whole-network recipe (as tests/test_gpu_skinning.py): warm up on a side stream, then capture on it."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step()
    return graph, static


def test_graph_capture_with_pinned_draws_replays_bit_identical():
    field = _field(2)
    params = list(field.lbs_network.parameters())
    draws = torch.rand(1024, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))

    def step():
        loss = _sk().skinning_loss(field, draws=draws)
        return (loss,) + tuple(torch.autograd.grad(loss, params))

    eager = [t.detach().clone() for t in step()]
    graph, static = _capture(step)
    for _ in range(2):
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


def test_graph_capture_of_the_default_path_draws_new_samples():
    field = _field(3)
    params = list(field.lbs_network.parameters())
    sampler = _sk().MeshSampler(field.smpl_verts, field.faces, field.skinning_weights, LO, HI, DEV)

    def step():
        loss = _sk().skinning_loss(field)  # torch.rand inside
        pn, _ = sampler.sample(1024)
        return (loss, pn) + tuple(torch.autograd.grad(loss, params))

    graph, static = _capture(step)
    seen = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        seen.append([t.detach().clone() for t in static])
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(seen[a][1], seen[b][1])          # other samples
        assert float(seen[a][0]) != float(seen[b][0])            # and another loss
    for run in seen:
        assert all(torch.isfinite(t).all() for t in run) and float(run[0]) > 0
        assert float(run[1].min()) >= -1.0 - 1e-6 and float(run[1].max()) <= 1.0 + 1e-6
