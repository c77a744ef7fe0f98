"""The wide fused MLP (gsplat_mi355.wide_mlp -> csrc/mlp_wide.hip) on the GPU: parity with the reference's own fp32 and fp64
results (tests/golden/wide_mlp.npz) and with the float64 restatement tests/wide_mlp_ref.py on the reference's three networks
at full shape, across tile and partial edges, widths, depths, skip layouts, first-layer widths, encodings and output
sizes; partial gradients, the forms of the condition, no rows, bitwise determinism, no host synchronisation, graph
capture, and `mlp_forward`, `hannw_mlp_forward` and `nonrigid.hannw_forward` end to end against the same chain in plain
fp64 torch.

Tolerance: the project's bar: no element beyond 1e-5 of its tensor's largest magnitude, all values finite.  Gradients are
compared on rows that keep clear of the activation's kink (wide_mlp_ref.random_inputs); the forward, which is continuous
there, also on unfiltered rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nonrigid_ref
import wide_mlp_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
FX = ref.load_fixture(os.path.join(ROOT, "tests", "golden", "wide_mlp.npz"))
R, CAP = 256, 128  # least rows per gradient partial, most partials (include/gsplat_mi355_wmlp.h)


def _wm():
    from gsplat_mi355 import wide_mlp
    return wide_mlp


def _tile():
    return _wm().TILE_ROWS  # the forward's row tile, as the library exports it


def _close(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(got.reshape(want.shape) - want).max())
    err = err / scale if scale > 0 else err  # (an all-zero expectation is met exactly or not at all)
    print("%s: %.3g of the largest magnitude" % (what, err))
    assert np.isfinite(got).all() and err <= BAR, "%s: %.3g of the largest magnitude" % (what, err)


def _dev(a, grad=False):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _names(cfg):
    return [k for k in ref.result_names(cfg) if k != "y"]


def _call(cfg, xt, Wt, bt, ct, band):
    return _wm().fused_wide_mlp(xt, Wt, bt, cond=ct, multires=cfg["multires"], include_input=cfg["include_input"],
                                band_weights=band, skip_in=cfg["skip_in"], negative_slope=cfg["slope"])


def _run(cfg, x, weights, biases, cond, g, band=None, need=None):
    """(y, {name: gradient}) of fused_wide_mlp for the upstream gradient g; `need` = the names that require one (None = all)."""
    want = lambda name: need is None or name in need
    xt, ct = _dev(x, want("dx")), _dev(cond, want("dcond"))
    Wt = [_dev(w, want("dW%d" % l)) for l, w in enumerate(weights)]
    bt = [_dev(b, want("db%d" % l)) for l, b in enumerate(biases)]
    y = _call(cfg, xt, Wt, bt, ct, band)
    names = ["dx"] + (["dcond"] if cond is not None else []) + ["dW%d" % l for l in range(len(Wt))] + ["db%d" % l for l in range(len(bt))]
    leaves = [xt] + ([ct] if cond is not None else []) + Wt + bt
    picked = [(k, t) for k, t in zip(names, leaves) if t.requires_grad]
    grads = torch.autograd.grad((y * _dev(g)).sum(), [t for _, t in picked]) if picked else ()
    return y.detach(), {k: v for (k, _), v in zip(picked, grads)}


_drawn = {}


def _inputs(cfg, n, seed, band=None):
    """(weights, biases, x, cond, g, the restatement's results): drawn and restated once per (network, n, seed)."""
    key = (tuple(sorted(cfg.items())), n, seed, band)
    if key not in _drawn:
        weights, biases = ref.random_params(cfg, seed)
        x, cond, g = ref.random_inputs(n, weights, biases, cfg, seed + 1, band=band)
        _drawn[key] = (weights, biases, x, cond, g, ref.flat(ref.forward_backward(x, weights, biases, cfg, cond, g, band)))
    return _drawn[key]


def _check(cfg, n, seed, what, band=None):
    """Parity with the restatement at N = n: every gradient on filtered rows, the forward on unfiltered rows too."""
    weights, biases, x, cond, g, want = _inputs(cfg, n, seed, band)
    y, grads = _run(cfg, x, weights, biases, cond, g, band)
    assert tuple(y.shape) == (n, cfg["dout"]) and sorted(grads) == sorted(_names(cfg))
    _close(y, want["y"], "%s y" % what)
    for k, v in grads.items():
        assert tuple(v.shape) == want[k].shape, k
        _close(v, want[k], "%s %s" % (what, k))
    xu, _, _ = ref.random_inputs(n, weights, biases, cfg, seed + 2, filtered=False)
    yu, _ = _run(cfg, xu, weights, biases, cond, g, band, need=())
    _close(yu, ref.forward(xu, weights, biases, cfg, cond, band)[0], "%s y (unfiltered rows)" % what)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_fixture_parity(case):
    cfg = ref.CASES[case]
    x, weights, biases, cond, g, band = ref.case_call(FX, case)
    y, grads = _run(cfg, x, weights, biases, cond, g, None if band is None else tuple(band.tolist()))
    grads["y"] = y
    assert sorted(grads) == sorted(ref.result_names(cfg))
    for name in ref.result_names(cfg):
        for tag in ("f32", "f64"):
            _close(grads[name], FX["%s/%s_%s" % (case, name, tag)], "%s %s vs the reference's %s" % (case, name, tag))


@pytest.mark.parametrize("name", ["nonrigid", "hannw", "texture"])
def test_reference_networks_at_full_shape(name):
    cfg = dict(nonrigid=ref.NONRIGID, hannw=ref.HANNW, texture=ref.TEXTURE)[name]
    band = (1.0, 1.0, 0.3454917, 0.0, 0.0, 0.0) if name == "hannw" else None
    _check(cfg, _tile() + R + 5, 700 + 10 * len(name), name, band)


EDGE = ref.net(3, 6, 0, 256, 2, (1,), 5)  # E = 39, the layer in front of the skip has 217 outputs


def _cap_n():
    """An N past CAP partials of R rows: rows per partial are then derived from N."""
    n = CAP * R + 232
    rows = _wm().rows_per_partial(n)
    assert rows > R and -(-n // rows) <= CAP
    return n


@pytest.mark.parametrize("n", ["1", "T-1", "T", "T+1", "2T+7", "cap"])
def test_row_edges(n):
    T = _tile()
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+7": 2 * T + 7, "cap": _cap_n()}[n]
    _check(EDGE, n, 720, "N=%d" % n)


NETWORKS = {
    "w32": ref.net(3, 2, 4, 32, 2, (2,), 5),
    "w160": ref.net(3, 6, 4, 160, 3, (2,), 5),
    "w224": ref.net(3, 6, 0, 224, 2, (1,), 5),
    "w256": ref.net(3, 6, 4, 256, 3, (2,), 5),
    "one_hidden": ref.net(3, 4, 3, 64, 1, (1,), 4),
    "eight_hidden": ref.net(3, 6, 3, 64, 8, (4,), 4),
    "skip_at_1": ref.net(3, 6, 3, 96, 3, (1,), 4),
    "skip_into_the_last_linear": ref.net(3, 6, 3, 96, 3, (3,), 4),
    "two_skips": ref.net(3, 6, 3, 96, 6, (2, 5), 4),
    "e271_no_encoding": ref.net(271, 0, 0, 64, 2, (), 3),
    "e512_c512": ref.net(512, 0, 512, 64, 2, (), 3),
    "d1_m10": ref.net(1, 10, 0, 64, 2, (1,), 3),
    "d4_m1": ref.net(4, 1, 0, 64, 2, (2,), 3),
    "no_raw_input": ref.net(3, 6, 0, 64, 2, (1,), 3, include_input=False),
    "dout1": ref.net(3, 3, 2, 64, 2, (2,), 1),
    "dout64": ref.net(3, 3, 2, 64, 2, (2,), 64),
}


@pytest.mark.parametrize("name", list(NETWORKS))
def test_networks(name):
    _check(NETWORKS[name], _tile() + R + 5, 740 + 7 * list(NETWORKS).index(name), name)


def test_zeroed_upper_bands():
    cfg = ref.net(3, 6, 3, 64, 3, (2,), 4, include_input=False, slope=0.0)
    _check(cfg, _tile() + 37, 900, "bands (1, 0.35, 0, 0, 0, 0)", band=(1.0, 0.35, 0.0, 0.0, 0.0, 0.0))


def test_relu_dead_units_pass_exactly_nothing():
    """Slope 0: a hidden unit that is exactly 0 in fp64 and fp32 alike (its weights 0, its bias -3) lets exactly nothing
    through: its own parameters' gradients and the next layer's column for it are 0.0, not small."""
    cfg = ref.net(3, 4, 3, 64, 2, (2,), 4, slope=0.0)
    n = _tile() + 9
    weights, biases = ref.random_params(cfg, 910)
    weights[0][5, :], biases[0][5] = 0.0, -3.0
    x, cond, g = ref.random_inputs(n, weights, biases, cfg, 911)
    want = ref.flat(ref.forward_backward(x, weights, biases, cfg, cond, g))
    y, grads = _run(cfg, x, weights, biases, cond, g)
    _close(y, want["y"], "relu y")
    for k, v in grads.items():
        _close(v, want[k], "relu %s" % k)
    assert not want["dW0"][5].any() and want["db0"][5] == 0 and not want["dW1"][:, 5].any()
    assert not grads["dW0"][5].any() and grads["db0"][5] == 0 and not grads["dW1"][:, 5].any()


PARTIAL = ref.net(3, 6, 5, 64, 3, (2,), 4)


@pytest.mark.parametrize("need", [("dcond", "dW0", "db0", "dW1", "db1", "dW3", "db3"), ("dx", "dW0", "db0", "dW3"), ("dW2",), ("dx",),
                                  ("dcond",), ("db3",)])
def test_partial_requires_grad(need):
    """x, cond or layers without a gradient: what is wanted has the bits of the full run, nothing else comes back."""
    weights, biases, x, cond, g, _ = _inputs(PARTIAL, R + 9, 920)
    y_full, full = _run(PARTIAL, x, weights, biases, cond, g)
    y, got = _run(PARTIAL, x, weights, biases, cond, g, need=need)
    assert torch.equal(y, y_full) and sorted(got) == sorted(need)
    for k, v in got.items():
        assert torch.equal(v, full[k]), k


def test_unwanted_gradients_are_not_written():
    """Through the C ABI: every gradient output carved from one poisoned arena with gaps; with dx (and a frozen layer, and
    dcond) NULL, every float outside the wanted outputs keeps the poison."""
    from gsplat_mi355 import _lib, _wide_lib
    L = _wide_lib.load()
    cfg = ref.net(3, 2, 9, 32, 2, (2,), 3)
    n = _tile() + R + 5
    weights, biases, x, cond, g, want = _inputs(cfg, n, 930)
    xt, ct, gt = _dev(x), _dev(cond), _dev(g)
    Wt, bt = [_dev(w) for w in weights], [_dev(b) for b in biases]
    a = _wm()._args(n, 3, 2, True, 9, 32, 2, 3, 1 << 2, 0.01, (1.0, 1.0), xt, ct, Wt, bt)
    y = torch.empty(n, 3, device=DEV)
    saved = torch.empty(_lib.nbytes(L.gs_wmlp_saved_bytes, ctypes.byref(a)) // 4, device=DEV)
    b0 = torch.empty(_lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), 0) // 4, device=DEV)
    stream = _lib.stream_ptr(DEV)
    _lib.check(L.gs_wmlp_forward(ctypes.byref(a), y.data_ptr(), saved.data_ptr(), b0.data_ptr(), 4 * b0.numel(), stream))
    _close(y, want["y"], "y through the C ABI")
    POISON, GAP = -7.25, 64
    sizes = dict(dx=x.size, dcond=cond.size)
    for l in range(3):
        sizes["dW%d" % l], sizes["db%d" % l] = weights[l].size, biases[l].size
    offs, total = {}, GAP
    for k, s in sizes.items():
        offs[k] = total
        total += (s + 3) // 4 * 4 + GAP
    for wanted in (list(sizes), [k for k in sizes if k not in ("dx", "dcond", "dW1", "db1")]):
        arena = torch.full((total,), POISON, device=DEV)
        addr = lambda k: arena.data_ptr() + 4 * offs[k] if k in wanted else None
        a.dx, a.dcond = addr("dx"), addr("dcond")
        for l in range(3):
            a.dW[l], a.db[l] = addr("dW%d" % l), addr("db%d" % l)
        ws = torch.empty(_lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), 1) // 4, device=DEV)
        _lib.check(L.gs_wmlp_backward(ctypes.byref(a), saved.data_ptr(), gt.data_ptr(), ws.data_ptr(), 4 * ws.numel(), stream))
        host = arena.cpu().numpy()
        untouched = np.ones(total, bool)
        for k in wanted:
            untouched[offs[k]:offs[k] + sizes[k]] = False
            _close(host[offs[k]:offs[k] + sizes[k]], want[k].reshape(-1), "%s through the C ABI (%d wanted)" % (k, len(wanted)))
        assert (host[untouched] == POISON).all(), "a float outside the wanted gradients was written"


def test_condition_forms_give_the_same_bits():
    weights, biases, x, cond, g, want = _inputs(PARTIAL, _tile() + 3, 940)
    n = x.shape[0]
    results = []
    for form in (lambda c: c, lambda c: c.reshape(1, -1), lambda c: c.reshape(1, -1).expand(n, -1), lambda c: c.expand(n, -1)):
        xt, base = _dev(x, True), _dev(cond, True)
        Wt, bt = [_dev(w, True) for w in weights], [_dev(b, True) for b in biases]
        y = _call(PARTIAL, xt, Wt, bt, form(base), None)
        results.append([y.detach()] + list(torch.autograd.grad((y * _dev(g)).sum(), [xt, base] + Wt + bt)))
    for other in results[1:]:
        for p, q in zip(results[0], other):
            assert torch.equal(p, q)
    _close(results[0][2], want["dcond"], "dcond")


def test_no_rows():
    weights, biases = ref.random_params(PARTIAL, 950)
    cond = np.ones(5, np.float32)
    x = np.zeros((0, 3), np.float32)
    y, grads = _run(PARTIAL, x, weights, biases, cond, np.zeros((0, 4), np.float32))
    assert tuple(y.shape) == (0, 4) and tuple(grads["dx"].shape) == x.shape
    for k, v in grads.items():
        assert not v.abs().sum().item(), k
    assert tuple(grads["dcond"].shape) == cond.shape and tuple(grads["dW0"].shape) == weights[0].shape


def test_bitwise_determinism():
    n = _cap_n()
    cfg = ref.net(3, 6, 5, 64, 2, (1,), 4)
    weights, biases, x, cond, g, want = _inputs(cfg, n, 960)
    y0, g0 = _run(cfg, x, weights, biases, cond, g)
    junk = [torch.empty(1 << 20, device=DEV) for _ in range(3)]  # unrelated allocations move every buffer
    side = torch.cuda.Stream(DEV)
    for stream in (torch.cuda.current_stream(DEV), side):
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            y, grads = _run(cfg, x, weights, biases, cond, g)
        stream.synchronize()
        assert torch.equal(y, y0)
        for k, v in g0.items():
            assert torch.equal(v, grads[k]), k
    del junk
    _close(g0["db2"], want["db2"], "the last bias's gradient at N=%d" % n)


def _step_fn(cfg=PARTIAL, n=3000, seed=970, band=None):
    weights, biases, x, cond, g, _ = _inputs(cfg, n, seed)
    gt = _dev(g)

    def fresh(x_values=x):
        return [_dev(x_values, True), _dev(cond, True)] + [_dev(w, True) for w in weights] + [_dev(b, True) for b in biases]

    def step(leaves):
        nl = len(weights)
        y = _call(cfg, leaves[0], leaves[2:2 + nl], leaves[2 + nl:], leaves[1].reshape(1, -1), band)
        return (y,) + tuple(torch.autograd.grad((y * gt).sum(), leaves))

    return fresh, step, x


def test_no_host_sync():
    fresh, step, _ = _step_fn()
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


def test_graph_capture_replays_bit_identical_with_new_inputs():
    """torch's whole-network recipe (as tests/test_gpu_mlp.py): fresh leaves first used on the side stream, then captured
    on it; the replay then reads new values of x from the captured leaf and must give eager's bits for them."""
    fresh, step, x = _step_fn()
    other = np.ascontiguousarray(x[::-1] * np.float32(0.5))
    eager = [[t.detach().clone() for t in step(fresh(v))] for v in (x, other)]
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
    for values, want in ((x, eager[0]), (other, eager[1])):
        with torch.no_grad():
            leaves[0].copy_(_dev(values))
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, want):
            assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_dtype_and_device_errors():
    weights, biases, x, cond, _, _ = _inputs(PARTIAL, 9, 980)
    Wt, bt = [_dev(w) for w in weights], [_dev(b) for b in biases]
    with pytest.raises(RuntimeError, match="GPU"):
        _call(PARTIAL, torch.from_numpy(x), Wt, bt, _dev(cond), None)
    with pytest.raises(RuntimeError, match="GPU"):
        _call(PARTIAL, _dev(x), Wt, bt, torch.from_numpy(cond), None)
    with pytest.raises(TypeError):
        _call(PARTIAL, _dev(x).double(), Wt, bt, _dev(cond), None)
    with pytest.raises(TypeError):
        _call(PARTIAL, _dev(x), [Wt[0].half()] + Wt[1:], bt, _dev(cond), None)


# ---- end to end: the module forwards against the same chain in plain fp64 torch
@pytest.fixture
def wide_on(monkeypatch):
    """Every class of network handed to the wide kernels, whatever the measured default says."""
    monkeypatch.setattr(_wm(), "DISPATCH", {"coordinate": True, "hannw": True, "plain": True})


class _Net(torch.nn.Module):
    """What VanillaCondMLP.__init__ / HannwCondMLP.__init__ leave on the module, with the fused forwards as the forward."""

    def __init__(self, cfg, weights, biases, dtype=torch.float32, hannw=False):
        super().__init__()
        self.cfg, self.hannw = cfg, hannw
        self.config = dict(multires=cfg["multires"], skip_in=list(cfg["skip_in"]), cond_in=[0] if cfg["C"] else [],
                           n_neurons=cfg["width"], n_hidden_layers=cfg["n_hidden"])
        if hannw:
            self.config["embedder"] = dict(ref.HANNW_EMBEDDER)
        self.num_layers = cfg["n_hidden"] + 2
        self.embed_fn = (lambda x: self.encode(x, None)) if (cfg["multires"] > 0 and not hannw) else None
        for l, (w, b) in enumerate(zip(weights, biases)):
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
            setattr(self, "lin%d" % l, lin)
        self.activation = torch.nn.ReLU() if hannw else torch.nn.LeakyReLU()
        self.to(device=DEV, dtype=dtype)

    def encode(self, x, band):
        m = self.cfg["multires"]
        if m == 0:
            return x
        band = [1.0] * m if band is None else band
        blocks = [x] if self.cfg["include_input"] else []
        for k in range(m):
            blocks += [band[k] * torch.sin(x * 2.0 ** k), band[k] * torch.cos(x * 2.0 ** k)]
        return torch.cat(blocks, 1)

    def forward(self, coords, *args, cond=None):
        if self.hannw:
            return _wm().hannw_mlp_forward(self, coords, args[0], cond=cond)
        from gsplat_mi355 import mlp
        return mlp.mlp_forward(self, coords, cond=cond)

    def plain(self, coords, cond=None, band=None):
        """The same chain in plain torch, in the module's own dtype."""
        e = self.encode(coords, band)
        h = e
        for l in range(self.num_layers - 1):
            if l == 0 and cond is not None:
                h = torch.cat([h, cond.expand(coords.shape[0], -1)], 1)
            if l in self.cfg["skip_in"]:
                h = torch.cat([h, e], 1) / np.sqrt(2.0)
            h = getattr(self, "lin%d" % l)(h)
            if l < self.num_layers - 2:
                h = self.activation(h)
        return h


def _is_fused(out):
    """Whether `out` came from the wide kernels' autograd node (directly, or through the view that restores the shape)."""
    return "FusedWide" in type(out.grad_fn).__name__ or "FusedWide" in str(out.grad_fn.next_functions)


def _net_grads(net, out, leaves, g):
    params = [p for _, p in sorted(net.named_parameters())]
    return list(torch.autograd.grad((out * g).sum(), leaves + params))


def _end_to_end(cfg, what, hannw=False, iteration=None):
    n = _tile() + R + 5
    band = _wm().hann_band_weights(ref.HANNW_EMBEDDER, cfg["multires"], iteration) if hannw else None
    weights, biases, x, cond, g, _ = _inputs(cfg, n, 1000, band)
    net, twin = _Net(cfg, weights, biases, hannw=hannw), _Net(cfg, weights, biases, dtype=torch.float64, hannw=hannw)
    assert _wm().wide_mlp_supported(net)
    leaves = [_dev(x, True)] + ([_dev(cond.reshape(1, -1), True)] if cond is not None else [])
    leaves64 = [t.detach().double().requires_grad_(True) for t in leaves]
    kw = dict(cond=leaves[1]) if cond is not None else {}
    out = net(leaves[0], iteration, **kw) if hannw else net(leaves[0], **kw)
    assert _is_fused(out), out.grad_fn
    want = twin.plain(leaves64[0], cond=leaves64[1] if cond is not None else None, band=band)
    _close(out, want.detach().cpu().numpy(), "%s: output" % what)
    names = ["x"] + (["cond"] if cond is not None else []) + [k for k, _ in sorted(net.named_parameters())]
    for k, p, q in zip(names, _net_grads(net, out, leaves, _dev(g)), _net_grads(twin, want, leaves64, _dev(g).double())):
        assert p.shape == q.shape
        _close(p, q.cpu().numpy(), "%s: gradient of %s" % (what, k))


@pytest.mark.parametrize("pattern", ["nonrigid", "texture"])
def test_mlp_forward_end_to_end(wide_on, pattern):
    """A stand-in for non_rigid/mlp.yaml's and texture/mlp.yaml's VanillaCondMLP with mlp_forward as its forward, called as
    nonrigid_forward (`self.mlp(xyz_norm, cond=pose_feat)`) and texture_forward (`self.mlp(inp)`) call theirs."""
    _end_to_end(ref.NONRIGID if pattern == "nonrigid" else ref.TEXTURE, pattern)


@pytest.mark.parametrize("iteration", sorted(ref.HANNW_ITERATIONS.values()))
def test_hannw_mlp_forward_end_to_end(wide_on, iteration):
    _end_to_end(ref.HANNW, "hannw at %d" % iteration, hannw=True, iteration=iteration)


def test_the_default_dispatch_is_what_the_module_says():
    """Without the fixture the measured default decides; a class that is off takes the torch path, bit for bit."""
    cfg = ref.net(3, 6, 5, 64, 3, (2,), 4)
    weights, biases, x, cond, g, _ = _inputs(cfg, 50, 1010)
    net = _Net(cfg, weights, biases)
    out = net(_dev(x), cond=_dev(cond.reshape(1, -1)))
    fused = _is_fused(out)
    assert fused == _wm().DISPATCH["coordinate"]
    if not fused:
        assert torch.equal(out, net.plain(_dev(x), cond=_dev(cond.reshape(1, -1))))


def test_a_network_both_paths_take_stays_narrow(wide_on):
    from gsplat_mi355 import mlp
    cfg = ref.net(32, 0, 144, 128, 3, (), 26)
    weights, biases, x, cond, g, _ = _inputs(cfg, _tile() + 3, 1020)
    net = _Net(cfg, weights, biases)
    assert mlp.mlp_supported(net) and _wm().wide_mlp_supported(net)
    xt, ct = _dev(x), _dev(cond.reshape(1, -1))
    out = net(xt, cond=ct)
    direct = mlp.fused_mlp(xt, [getattr(net, "lin%d" % l).weight for l in range(4)], [getattr(net, "lin%d" % l).bias for l in range(4)],
                           cond=ct)
    assert torch.equal(out, direct) and not _is_fused(out)
    wide = _call(cfg, xt, [_dev(w) for w in weights], [_dev(b) for b in biases], ct, None)
    _close(wide, direct.detach().double().cpu().numpy(), "the wide kernels on the narrow network")


class _AABB(torch.nn.Module):  # utils/dataset_utils.py AABB.normalize, restated
    def __init__(self, cmax, cmin, dtype):
        super().__init__()
        self.register_buffer("coord_max", torch.tensor(cmax, dtype=dtype))
        self.register_buffer("coord_min", torch.tensor(cmin, dtype=dtype))

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1.0 if sym else x


class _Gaussians(object):
    def __init__(self, xyz, scaling, rotation):
        self._xyz, self._scaling, self._rotation = xyz, scaling, rotation

    @property
    def get_xyz(self):
        return self._xyz

    def clone(self):
        return _Gaussians(self._xyz, self._scaling, self._rotation)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _HannwDeformer(torch.nn.Module):
    """A stand-in for HannwMLP with the reference's attribute names."""

    def __init__(self, cfg, net_cfg, weights, biases, dtype):
        super().__init__()
        self.cfg = cfg
        self.pose_encoder = nonrigid_ref.PoseEncoder(dim_per_joint=6, seed=51, dtype=dtype)
        self.mlp = _Net(net_cfg, weights, biases, dtype=dtype, hannw=True)
        self.aabb = _AABB([0.5, 1.0, 0.75], [-0.5, -1.0, -0.25], dtype)  # power-of-two extents: exact in fp32


@pytest.mark.parametrize("ro", ["add", "mult"])
def test_hannw_forward_end_to_end(wide_on, ro):
    from gsplat_mi355 import nonrigid
    n = 100
    net_cfg = ref.net(3, 6, 144, 64, 3, (2,), 10, include_input=False, slope=0.0)
    rng = np.random.default_rng(1030)
    xyz0 = (rng.integers(0, 1024, (n, 3)) / 1024.0 * np.array([1.0, 2.0, 1.0]) + np.array([-0.5, -1.0, -0.25])).astype(np.float32)
    inp, ups = nonrigid_ref.apply_inputs(n, 10, seed=1031)
    rots, Jtrs = nonrigid_ref.random_pose(1032)
    weights, biases = ref.random_params(net_cfg, 1033)
    weights[-1] *= np.float32(0.1)  # offsets of order 0.1
    cfg = _Cfg(scale_offset="logit", rot_offset=ro, mlp=_Cfg(embedder=_Cfg(ref.HANNW_EMBEDDER)))
    model = _HannwDeformer(cfg, net_cfg, weights, biases, torch.float32).to(DEV)
    twin = _HannwDeformer(cfg, net_cfg, weights, biases, torch.float64).to(DEV)
    camera = type("Camera", (), {})()

    def run(fused, iteration):
        dt = torch.float32 if fused else torch.float64
        t = lambda a: _dev(a).to(dt)
        gs = _Gaussians(t(xyz0).requires_grad_(True), t(inp["scaling"]).requires_grad_(True), t(inp["rotation"]).requires_grad_(True))
        camera.rots, camera.Jtrs = t(rots).requires_grad_(True), t(Jtrs).requires_grad_(True)
        if fused:
            mod = model
            d, losses = nonrigid.hannw_forward(model, gs, iteration, camera)
            assert sorted(losses) == ["nr_rot", "nr_scale", "nr_xyz"]
            assert nonrigid.hannw_forward(model, gs, iteration, camera, compute_loss=False)[1] == {}
            out = dict(xyz=d._xyz, scaling=d._scaling, rotation=d._rotation, **losses)
        else:  # the same chain in plain torch
            mod = twin
            pose_feat = twin.pose_encoder(camera.rots, camera.Jtrs)
            band = _wm().hann_band_weights(ref.HANNW_EMBEDDER, 6, iteration)
            deltas = twin.mlp.plain(twin.aabb.normalize(gs.get_xyz, sym=True), cond=pose_feat, band=band)
            if iteration < ref.HANNW_EMBEDDER["kick_in_iter"]:
                deltas = deltas * torch.zeros_like(deltas)
            x, s, q, _, nr3 = nonrigid_ref.apply(deltas, gs._xyz, gs._scaling, gs._rotation, "logit", ro)
            out = dict(xyz=x, scaling=s, rotation=q, nr_xyz=nr3[0], nr_scale=nr3[1], nr_rot=nr3[2])
        w = ups["g_nr"]
        ((out["xyz"] * t(ups["g_xyz"])).sum() + (out["scaling"] * t(ups["g_scal"])).sum() + (out["rotation"] * t(ups["g_rot"])).sum()
         + float(w[0]) * out["nr_xyz"] + float(w[1]) * out["nr_scale"] + float(w[2]) * out["nr_rot"]).backward()
        res = dict(out)
        res.update(dxyz=gs._xyz.grad, dscaling=gs._scaling.grad, drotation=gs._rotation.grad)
        res.update({"p." + name: p.grad for name, p in mod.named_parameters()})
        for p in mod.parameters():
            p.grad = None
        return res

    for iteration in (1000, 5800):
        got, want = run(True, iteration), run(False, iteration)
        assert sorted(got) == sorted(want)
        for name in want:
            assert got[name] is not None, name  # zero gradients before kick-in, never None: Adam's step count depends on it
            _close(got[name], want[name].detach().double().cpu().numpy(), "hannw_forward at %d: %s" % (iteration, name))
        if iteration < ref.HANNW_EMBEDDER["kick_in_iter"]:
            assert torch.equal(got["xyz"], _dev(xyz0)) and all(not got[k].any() for k in got if k.startswith("p.mlp."))
        else:
            assert all(got[k].any() for k in got if k.startswith("p.mlp.lin"))
