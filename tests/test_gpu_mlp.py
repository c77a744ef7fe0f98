"""The fused MLP (gsplat_mi355.mlp -> csrc/mlp.hip) on the GPU: parity with the reference's own fp32 and fp64 results
(tests/golden/mlp.npz) and with the float64 restatement tests/mlp_ref.py across tile and partial edges, the default
networks and the limits of every size; partial gradients, the forms of the condition, strides, no rows, bitwise
determinism, no host synchronisation, graph capture, and `mlp_forward` end to end against the same chain in plain fp64
torch.

Tolerance: the project's bar (BAR in test_gpu_skinning.py): no element beyond 1e-5 of its tensor's largest magnitude.
Gradients are compared on rows that keep clear of the LeakyReLU's kink (mlp_ref.random_inputs: a pre-activation whose
fp32 and fp64 signs differ flips a whole gradient path, which is a threshold decision and not an error); the forward,
which is continuous there, also on unfiltered rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mlp_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
FX = ref.load_fixture(os.path.join(ROOT, "tests", "golden", "mlp.npz"))
T, R, CAP = 128, 256, 128  # rows per forward tile, least rows per gradient partial, most partials (include/gsplat_mi355.h)
SKINNING, NONRIGID, TEXTURE = (3, 0, 128, 4, 25), (32, 144, 128, 3, 26), (79, 0, 64, 2, 3)  # the default config's networks


def _mlp():
    from gsplat_mi355 import mlp
    return mlp


def _close(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.reshape(want.shape) - want).max()) / scale
    print("%s: %.3g of the largest magnitude" % (what, err))
    assert np.isfinite(got).all() and err <= BAR, "%s: %.3g of the largest magnitude" % (what, err)


def _dev(a, grad=False):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _run(x, weights, biases, cond, g, need=None):
    """(y, {name: gradient}) of fused_mlp for the upstream gradient g; `need` = the names that require one (None = all)."""
    want = lambda name: need is None or name in need
    xt, ct = _dev(x, want("dx")), _dev(cond, want("dcond"))
    Wt = [_dev(w, want("dW%d" % l)) for l, w in enumerate(weights)]
    bt = [_dev(b, want("db%d" % l)) for l, b in enumerate(biases)]
    y = _mlp().fused_mlp(xt, Wt, bt, cond=ct)
    names = ["dx"] + (["dcond"] if cond is not None else []) + ["dW%d" % l for l in range(len(Wt))] + ["db%d" % l for l in range(len(bt))]
    leaves = [xt] + ([ct] if cond is not None else []) + Wt + bt
    picked = [(k, t) for k, t in zip(names, leaves) if t.requires_grad]
    grads = torch.autograd.grad((y * _dev(g)).sum(), [t for _, t in picked]) if picked else ()
    return y.detach(), {k: v for (k, _), v in zip(picked, grads)}


def _check(shape, n, seed, what):
    """Parity with the restatement at N = n: every gradient on filtered rows, the forward on unfiltered rows too."""
    din, C, width, n_hidden, dout = shape
    weights, biases = ref.random_params(din, C, width, n_hidden, dout, seed)
    x, cond, g = ref.random_inputs(n, weights, biases, C, seed + 1)
    y, grads = _run(x, weights, biases, cond, g)
    want = ref.flat(ref.forward_backward(x, weights, biases, cond, g))
    assert tuple(y.shape) == (n, dout) and sorted(grads) == sorted(k for k in want if k != "y")
    _close(y, want["y"], "%s y" % what)
    for k, v in grads.items():
        assert tuple(v.shape) == want[k].shape, k
        _close(v, want[k], "%s %s" % (what, k))
    xu, _, _ = ref.random_inputs(n, weights, biases, C, seed + 2, filtered=False)
    yu, _ = _run(xu, weights, biases, cond, g, need=())
    _close(yu, ref.forward(xu, weights, biases, cond)[0], "%s y (unfiltered rows)" % what)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_fixture_parity(case):
    x, weights, biases, cond, g = ref.case_call(FX, case)
    y, grads = _run(x, weights, biases, cond, g)
    grads["y"] = y
    assert sorted(grads) == sorted(ref.result_names(case))
    for name in ref.result_names(case):
        for tag in ("f32", "f64"):
            _close(grads[name], FX["%s/%s_%s" % (case, name, tag)], "%s %s vs the reference's %s" % (case, name, tag))


def _cap_n():
    """An N past CAP partials of R rows: rows per partial are then derived from N."""
    n = CAP * R + 232
    rows = _mlp().rows_per_partial(n)
    assert rows > R and -(-n // rows) <= CAP
    return n


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T + 7, R + T + 5, "cap"])
def test_row_edges(n):
    n = _cap_n() if n == "cap" else n
    if n == R + T + 5:  # the first partial spans two tiles, and there is a second one
        assert _mlp().rows_per_partial(n) == R == 2 * T and -(-n // R) == 2
    _check(SKINNING, n, 500, "N=%d" % n)


NETWORKS = {
    "skinning": SKINNING, "nonrigid": NONRIGID, "texture": TEXTURE,
    "w32_one_hidden_din5_cond1_dout1": (5, 1, 32, 1, 1),
    "w96_din1_dout64": (1, 0, 96, 2, 64),
    "six_hidden_din512_cond512": (512, 512, 64, 6, 3),
    "din271_two_chunks_and_a_tail": (271, 0, 128, 4, 3),
}


@pytest.mark.parametrize("name", list(NETWORKS))
def test_networks(name):
    _check(NETWORKS[name], R + T + 5, 520 + 7 * list(NETWORKS).index(name), name)


def _inputs(shape, n, seed):
    din, C, width, n_hidden, dout = shape
    weights, biases = ref.random_params(din, C, width, n_hidden, dout, seed)
    return (weights, biases) + ref.random_inputs(n, weights, biases, C, seed + 1)


@pytest.mark.parametrize("need", [("dcond", "dW0", "db0", "dW1", "db1", "dW3", "db3"), ("dx", "dW0", "db0", "dW3"), ("dW2",), ("dx",),
                                  ("dcond",), ("db3",)])
def test_partial_requires_grad(need):
    """x, cond or layers without a gradient: what is wanted has the bits of the full run, nothing else comes back."""
    weights, biases, x, cond, g = _inputs(NONRIGID, R + 9, 540)
    y_full, full = _run(x, weights, biases, cond, g)
    y, got = _run(x, weights, biases, cond, g, need=need)
    assert torch.equal(y, y_full) and sorted(got) == sorted(need)
    for k, v in got.items():
        assert torch.equal(v, full[k]), k


def test_unwanted_gradients_are_not_written():
    """Through the C ABI: every gradient output carved from one poisoned arena with gaps; with dx (and a frozen layer, and
    dcond) NULL, every float outside the wanted outputs keeps the poison."""
    from gsplat_mi355 import _lib
    L = _lib.load()
    din, C, width, n_hidden, dout = shape = (5, 9, 32, 2, 3)
    n = R + T + 5
    weights, biases, x, cond, g = _inputs(shape, n, 550)
    xt, ct, gt = _dev(x), _dev(cond), _dev(g)
    Wt, bt = [_dev(w) for w in weights], [_dev(b) for b in biases]
    a = _mlp()._args(n, din, C, width, n_hidden, dout, 0.01, xt, ct, Wt, bt)
    y = torch.empty(n, dout, device=DEV)
    acts = torch.empty(n_hidden, n, width, device=DEV)
    b0 = torch.empty(width, device=DEV)
    stream = _lib.stream_ptr(DEV)
    _lib.check(L.gs_mlp_forward(ctypes.byref(a), y.data_ptr(), acts.data_ptr(), b0.data_ptr(), 4 * width, stream))
    _close(y, ref.forward(x, weights, biases, cond)[0], "y through the C ABI")
    POISON, GAP = -7.25, 64
    sizes = dict(dx=n * din, dcond=C)
    for l in range(n_hidden + 1):
        sizes["dW%d" % l], sizes["db%d" % l] = weights[l].size, biases[l].size
    offs, total = {}, GAP
    for k, s in sizes.items():
        offs[k] = total
        total += (s + 3) // 4 * 4 + GAP
    want = ref.flat(ref.forward_backward(x, weights, biases, cond, g))
    for wanted in (list(sizes), [k for k in sizes if k not in ("dx", "dcond", "dW1", "db1")]):
        arena = torch.full((total,), POISON, device=DEV)
        addr = lambda k: arena.data_ptr() + 4 * offs[k] if k in wanted else None
        a.dx, a.dcond = addr("dx"), addr("dcond")
        for l in range(n_hidden + 1):
            a.dW[l], a.db[l] = addr("dW%d" % l), addr("db%d" % l)
        ws = torch.empty(_lib.nbytes(L.gs_mlp_workspace_bytes, ctypes.byref(a), 1) // 4, device=DEV)
        _lib.check(L.gs_mlp_backward(ctypes.byref(a), acts.data_ptr(), gt.data_ptr(), ws.data_ptr(), 4 * ws.numel(), stream))
        host = arena.cpu().numpy()
        untouched = np.ones(total, bool)
        for k in wanted:
            untouched[offs[k]:offs[k] + sizes[k]] = False
            _close(host[offs[k]:offs[k] + sizes[k]], want[k].reshape(-1), "%s through the C ABI (%d wanted)" % (k, len(wanted)))
        assert (host[untouched] == POISON).all(), "a float outside the wanted gradients was written"


def test_condition_forms_give_the_same_bits():
    weights, biases, x, cond, g = _inputs(NONRIGID, T + 3, 560)
    n = x.shape[0]
    results = []
    for form in (lambda c: c, lambda c: c.reshape(1, -1), lambda c: c.reshape(1, -1).expand(n, -1), lambda c: c.expand(n, -1)):
        xt, base = _dev(x, True), _dev(cond, True)
        Wt, bt = [_dev(w, True) for w in weights], [_dev(b, True) for b in biases]
        y = _mlp().fused_mlp(xt, Wt, bt, cond=form(base))
        results.append([y.detach()] + list(torch.autograd.grad((y * _dev(g)).sum(), [xt, base] + Wt + bt)))
    for other in results[1:]:
        for p, q in zip(results[0], other):
            assert torch.equal(p, q)
    _close(results[0][2], ref.forward_backward(x, weights, biases, cond, g)["dcond"], "dcond")


class _Net(torch.nn.Module):
    """What VanillaCondMLP.__init__ leaves on the module, with mlp_forward as the forward."""

    def __init__(self, shape, weights, biases, dtype=torch.float32):
        super().__init__()
        din, C, width, n_hidden, dout = shape
        self.config = dict(multires=0, skip_in=[], cond_in=[0] if C else [], n_neurons=width, n_hidden_layers=n_hidden)
        self.num_layers, self.embed_fn = n_hidden + 2, None
        for l, (w, b) in enumerate(zip(weights, biases)):
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
            setattr(self, "lin%d" % l, lin)
        self.activation = torch.nn.LeakyReLU()
        self.to(device=DEV, dtype=dtype)

    def forward(self, coords, cond=None):
        return _mlp().mlp_forward(self, coords, cond=cond)

    def plain(self, coords, cond=None):
        """The same chain in plain torch, in the module's own dtype."""
        h = coords if cond is None else torch.cat([coords, cond.expand(coords.shape[0], -1)], 1)
        for l in range(self.num_layers - 1):
            h = getattr(self, "lin%d" % l)(h)
            if l < self.num_layers - 2:
                h = torch.nn.functional.leaky_relu(h, 0.01)
        return h


def _net_grads(net, out, leaves, g):
    params = [p for _, p in sorted(net.named_parameters())]
    return list(torch.autograd.grad((out * g).sum(), leaves + params))


def test_distinct_condition_rows_take_the_torch_path():
    shape = (7, 5, 32, 2, 4)
    weights, biases, x, _, g = _inputs(shape, 50, 570)
    conds = np.random.default_rng(571).normal(size=(50, 5)).astype(np.float32)
    net = _Net(shape, weights, biases)
    assert _mlp().mlp_supported(net)
    xt, ct = _dev(x, True), _dev(conds, True)
    got = net(xt, cond=ct)
    want = net.plain(xt, cond=ct)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    for p, q in zip(_net_grads(net, got, [xt, ct], _dev(g)), _net_grads(net, want, [xt, ct], _dev(g))):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7)


def test_strides_give_the_same_bits():
    weights, biases, x, cond, g = _inputs(TEXTURE, T + 3, 580)
    y0, g0 = _run(x, weights, biases, cond, g)
    n, din = x.shape
    wide = torch.zeros(n, 2 * din + 1, device=DEV)
    wide[:, 1::2] = _dev(x)
    xt = wide[:, 1::2].requires_grad_(True)                    # columns two apart
    Wt = [_dev(np.ascontiguousarray(w.T)).t().requires_grad_(True) for w in weights]  # transposed views
    assert not xt.is_contiguous() and not any(w.is_contiguous() for w in Wt)
    bt = [_dev(b, True) for b in biases]
    y = _mlp().fused_mlp(xt, Wt, bt)
    grads = torch.autograd.grad((y * _dev(g)).sum(), [xt] + Wt + bt)
    assert torch.equal(y.detach(), y0) and torch.equal(grads[0], g0["dx"])
    for l in range(len(Wt)):
        assert grads[1 + l].shape == Wt[l].shape
        assert torch.equal(grads[1 + l], g0["dW%d" % l]) and torch.equal(grads[1 + len(Wt) + l], g0["db%d" % l])
    # an x that starts off a 16-byte boundary is copied once, too
    shifted = torch.zeros(n * din + 1, device=DEV)[1:].view(n, din).copy_(_dev(x))
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(_mlp().fused_mlp(shifted, [_dev(w) for w in weights], [_dev(b) for b in biases]), y0)


def test_no_rows():
    weights, biases, _, cond, _ = _inputs(NONRIGID, 4, 590)
    x = np.zeros((0, NONRIGID[0]), np.float32)
    y, grads = _run(x, weights, biases, cond, np.zeros((0, NONRIGID[4]), np.float32))
    assert tuple(y.shape) == (0, NONRIGID[4]) and tuple(grads["dx"].shape) == x.shape
    for k, v in grads.items():
        assert not v.abs().sum().item(), k
    assert tuple(grads["dcond"].shape) == cond.shape and tuple(grads["dW0"].shape) == weights[0].shape


def test_bitwise_determinism():
    n = _cap_n()
    weights, biases, x, cond, g = _inputs(NONRIGID, n, 600)
    y0, g0 = _run(x, weights, biases, cond, g)
    junk = [torch.empty(1 << 20, device=DEV) for _ in range(3)]  # unrelated allocations move every buffer
    side = torch.cuda.Stream(DEV)
    for stream in (torch.cuda.current_stream(DEV), side):
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            y, grads = _run(x, weights, biases, cond, g)
        stream.synchronize()
        assert torch.equal(y, y0)
        for k, v in g0.items():
            assert torch.equal(v, grads[k]), k
    del junk
    _close(g0["db%d" % NONRIGID[3]], g.astype(np.float64).sum(0), "the last bias's gradient at N=%d" % n)


def _step_fn(shape=NONRIGID, n=5000, seed=610):
    weights, biases, x, cond, g = _inputs(shape, n, seed)
    gt = _dev(g)

    def fresh():
        return [_dev(x, True), _dev(cond, True)] + [_dev(w, True) for w in weights] + [_dev(b, True) for b in biases]

    def step(leaves):
        nl = len(weights)
        y = _mlp().fused_mlp(leaves[0], leaves[2:2 + nl], leaves[2 + nl:], cond=leaves[1].reshape(1, -1))
        return (y,) + tuple(torch.autograd.grad((y * gt).sum(), leaves))

    return fresh, step


def test_no_host_sync():
    fresh, step = _step_fn()
    leaves = fresh()
    step(leaves)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(leaves)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)


def test_graph_capture_replays_bit_identical():
    """torch's whole-network recipe (as tests/test_gpu_pose.py): fresh leaves first used on the side stream, then
    captured on it."""
    fresh, step = _step_fn()
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


def test_dtype_and_device_errors():
    weights, biases, x, cond, _ = _inputs((3, 5, 32, 2, 4), 9, 620)
    Wt, bt = [_dev(w) for w in weights], [_dev(b) for b in biases]
    with pytest.raises(RuntimeError, match="GPU"):
        _mlp().fused_mlp(torch.from_numpy(x), Wt, bt, cond=_dev(cond))
    with pytest.raises(RuntimeError, match="GPU"):
        _mlp().fused_mlp(_dev(x), Wt, bt, cond=torch.from_numpy(cond))
    with pytest.raises(TypeError):
        _mlp().fused_mlp(_dev(x).double(), Wt, bt, cond=_dev(cond))
    with pytest.raises(TypeError):
        _mlp().fused_mlp(_dev(x), [Wt[0].half()] + Wt[1:], bt, cond=_dev(cond))


@pytest.mark.parametrize("pattern", ["nonrigid", "texture"])
def test_mlp_forward_end_to_end(pattern):
    """A stand-in module with mlp_forward as its forward, called as nonrigid_forward calls its MLP (`self.mlp(feat,
    cond=pose_feat)`, pose_feat (1, C)) and as texture_forward calls its own (`self.mlp(inp)`), against the same chain
    in plain fp64 torch."""
    shape = NONRIGID if pattern == "nonrigid" else TEXTURE
    weights, biases, x, cond, g = _inputs(shape, R + T + 5, 630)
    net = _Net(shape, weights, biases)
    twin = _Net(shape, weights, biases, dtype=torch.float64)
    assert _mlp().mlp_supported(net)
    leaves = [_dev(x, True)] + ([_dev(cond.reshape(1, -1), True)] if cond is not None else [])
    leaves64 = [t.detach().double().requires_grad_(True) for t in leaves]
    out = net(leaves[0], cond=leaves[1]) if pattern == "nonrigid" else net(leaves[0])
    want = twin.plain(leaves64[0], cond=leaves64[1] if pattern == "nonrigid" else None)
    _close(out, want.detach().cpu().numpy(), "%s: output" % pattern)
    names = ["x"] + (["cond"] if cond is not None else []) + [k for k, _ in sorted(net.named_parameters())]
    for k, p, q in zip(names, _net_grads(net, out, leaves, _dev(g)), _net_grads(twin, want, leaves64, _dev(g).double())):
        assert p.shape == q.shape
        _close(p, q.cpu().numpy(), "%s: gradient of %s" % (pattern, k))
    state = net.state_dict()
    assert sorted(state) == sorted("lin%d.%s" % (l, k) for l in range(shape[3] + 1) for k in ("weight", "bias"))
