"""The fused MLP's C ABI, Python entry points and fixture on the CPU (no GPU needed): the new symbols are declared,
exported and bound, the struct mirrors the header's field for field, argument validation works with never-dereferenced
pointers (each limit and one past it), the Python functions reject what they must before touching a device,
`mlp_supported` takes the three default networks and turns down what the kernels do not cover, `mlp_forward`'s torch
path evaluates those, and the float64 restatement tests/mlp_ref.py reproduces the reference's own fp64 autograd results
(tests/golden/mlp.npz) to 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import mlp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_mlp_workspace_bytes", "gs_mlp_forward", "gs_mlp_backward")
DEFINES = (("GS_MLP_MAX_WIDTH", 128), ("GS_MLP_MAX_HIDDEN", 6), ("GS_MLP_MAX_LAYERS", 7), ("GS_MLP_MAX_IN", 512),
           ("GS_MLP_MAX_COND", 512), ("GS_MLP_MAX_OUT", 64), ("GS_MLP_TILE_ROWS", 128), ("GS_MLP_PARTIAL_MIN_ROWS", 256),
           ("GS_MLP_MAX_PARTIALS", 128))


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "mlp.npz"))


def test_symbols_declared_exported_and_bound(lib):
    header = abi_header.text()
    lib.load()
    for name, value in DEFINES:
        assert getattr(lib, name) == value
    assert lib.GS_MLP_MAX_LAYERS == lib.GS_MLP_MAX_HIDDEN + 1
    # six ints and the slope (28 bytes, padded to 32), then 2 + 4 x 7 + 2 addresses
    assert ctypes.sizeof(lib.GsMlpArgs) == 32 + 32 * ctypes.sizeof(ctypes.c_void_p)
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in NEW[1:]:
        assert name in capture_safe, name
    build_py = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "build.py")).read()
    assert build_py.count('"mlp.hip"') == 2  # SOURCES and STRICT


P, ODD4, ODD16 = 0x1000, 0x1002, 0x1004  # never dereferenced: validation fails first


def _args(lib, N=300, din=3, C=0, width=128, n_hidden=4, dout=25, grads=True, **over):
    a = lib.GsMlpArgs()
    a.N, a.dim_in, a.dim_cond, a.width, a.n_hidden, a.dim_out, a.slope = N, din, C, width, n_hidden, dout, 0.01
    a.x = P
    a.cond = P if C else None
    for l in range(min(max(n_hidden, 0), 6) + 1):
        a.W[l] = a.b[l] = P
        if grads:
            a.dW[l] = a.db[l] = P
    if grads:
        a.dx = P
        a.dcond = P if C else None
    for k, v in over.items():
        if k in ("W", "b", "dW", "db"):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _part_floats(din, width, n_hidden, dout):
    return width * (din + 1) + (n_hidden - 1) * width * (width + 1) + dout * (width + 1)


def test_workspace_sizes(lib):
    from gsplat_mi355 import mlp
    L = lib.load()
    ws = lambda a, bwd: lib.nbytes(L.gs_mlp_workspace_bytes, ctypes.byref(a), bwd)
    # rows per partial: 256 until 128 partials of them no longer cover N, then ceil(N / 128) rounded up to 32
    for n, rows in ((1, 256), (256, 256), (32768, 256), (32769, 288), (33000, 288), (200000, 1568)):
        assert mlp.rows_per_partial(n) == rows
        assert -(-n // rows) <= lib.GS_MLP_MAX_PARTIALS
    for shape in ((3, 0, 128, 4, 25), (32, 144, 128, 3, 26), (79, 0, 64, 2, 3), (512, 512, 32, 1, 64)):
        din, C, width, n_hidden, dout = shape
        for n in (1, 256, 257, 389, 33000):
            a = _args(lib, n, *shape)
            assert ws(a, 0) == (4 * width if C else 0)
            parts = -(-n // mlp.rows_per_partial(n))
            assert ws(a, 1) == 4 * (n_hidden * n * width + parts * _part_floats(din, width, n_hidden, dout)), (shape, n)
    assert ws(_args(lib, 0), 0) == 0 and ws(_args(lib, 0), 1) == 0
    out = ctypes.c_size_t(0)
    assert L.gs_mlp_workspace_bytes(None, 1, ctypes.byref(out)) == -1
    assert L.gs_mlp_workspace_bytes(ctypes.byref(_args(lib)), 1, None) == -1
    assert L.gs_mlp_workspace_bytes(ctypes.byref(_args(lib, width=160)), 1, ctypes.byref(out)) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    BIG = 1 << 40

    def fwd(a, y=P, acts=P, ws=P, nbytes=BIG):
        return L.gs_mlp_forward(ctypes.byref(a) if a is not None else None, y, acts, ws, nbytes, None)

    def bwd(a, acts=P, g=P, ws=P, nbytes=BIG):
        return L.gs_mlp_backward(ctypes.byref(a) if a is not None else None, acts, g, ws, nbytes, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        assert call(_args(lib, N=-1)) == -1
        assert call(_args(lib, N=0)) == 0 and call(_args(lib, N=0, x=None)) == 0  # no rows: nothing to do
        for kw in (dict(width=0), dict(width=16), dict(width=48), dict(width=160), dict(n_hidden=0), dict(n_hidden=7),
                   dict(din=0), dict(din=513), dict(C=-1), dict(C=513), dict(dout=0), dict(dout=65),
                   dict(slope=float("nan"))):
            assert call(_args(lib, **kw)) == -1, kw
        assert call(_args(lib, x=None)) == -1 and call(_args(lib, x=ODD16)) == -1
        assert call(_args(lib, C=5, cond=None)) == -1 and call(_args(lib, C=5, cond=ODD4)) == -1
        for l in (0, 2, 4):
            assert call(_args(lib, W=(l, None))) == -1 and call(_args(lib, b=(l, None))) == -1, l
            assert call(_args(lib, W=(l, ODD4))) == -1 and call(_args(lib, b=(l, ODD4))) == -1, l
    # every limit itself passes the shape checks: the workspace check answers the backward
    for kw in (dict(width=32), dict(width=128), dict(n_hidden=1), dict(n_hidden=6), dict(din=1), dict(din=512),
               dict(C=512), dict(dout=1), dict(dout=64)):
        assert bwd(_args(lib, **kw), nbytes=0) == -5, kw
    assert fwd(_args(lib, C=1), nbytes=4 * 128 - 1) == -5 and fwd(_args(lib, C=512), ws=None) == -1
    assert fwd(_args(lib, C=5), ws=ODD4) == -1
    assert fwd(_args(lib), y=None) == -1 and fwd(_args(lib), y=ODD4) == -1 and fwd(_args(lib), acts=ODD16) == -1
    assert bwd(_args(lib), acts=None) == -1 and bwd(_args(lib), acts=ODD16) == -1
    assert bwd(_args(lib), g=None) == -1 and bwd(_args(lib), g=ODD16) == -1
    assert bwd(_args(lib), ws=None) == -1 and bwd(_args(lib), ws=ODD16) == -1
    assert bwd(_args(lib, dx=ODD4)) == -1 and bwd(_args(lib, C=5, dcond=ODD4)) == -1
    assert bwd(_args(lib, dW=(1, ODD4))) == -1 and bwd(_args(lib, db=(4, ODD4))) == -1
    assert bwd(_args(lib, dcond=P)) == -1  # no condition: no dL_dcond
    a = _args(lib)
    need = lib.nbytes(L.gs_mlp_workspace_bytes, ctypes.byref(a), 1)
    assert bwd(a, nbytes=need - 1) == -5
    # nothing wanted: nothing to do (and nothing launched)
    assert bwd(_args(lib, grads=False), ws=None, nbytes=0) == 0


def _lin(i, o):
    return torch.nn.Linear(i, o)


def _module(din, C, width, n_hidden, dout, cond_in=None, skip_in=(), multires=0, widths=None):
    """What VanillaCondMLP.__init__ leaves on the module, as far as the forward and mlp_supported read it."""
    from gsplat_mi355 import mlp
    cond_in = ([0] if C else []) if cond_in is None else cond_in
    widths = widths or [width] * n_hidden
    dims = [din] + list(widths) + [dout]
    m = torch.nn.Module()
    m.config = dict(multires=multires, skip_in=list(skip_in), cond_in=list(cond_in), n_neurons=width, n_hidden_layers=n_hidden)
    m.num_layers = len(dims)
    m.embed_fn = None
    for l in range(len(dims) - 1):
        out = dims[l + 1] - dims[0] if l + 1 in skip_in else dims[l + 1]
        setattr(m, "lin%d" % l, _lin(dims[l] + (C if l in cond_in else 0), out))
    m.activation = torch.nn.LeakyReLU()
    m.forward = lambda coords, cond=None: mlp.mlp_forward(m, coords, cond)
    return m


def test_mlp_supported():
    from gsplat_mi355 import mlp
    # the three networks of the default config: skinning field, non-rigid deformer, colour MLP
    for shape in ((3, 0, 128, 4, 25), (32, 144, 128, 3, 26), (79, 0, 64, 2, 3)):
        assert mlp.mlp_supported(_module(*shape)), shape
    ok = (3, 0, 64, 2, 3)
    assert mlp.mlp_supported(_module(*ok))
    assert not mlp.mlp_supported(_module(*ok, multires=6))
    assert not mlp.mlp_supported(_module(*ok, skip_in=(2,)))
    assert not mlp.mlp_supported(_module(3, 5, 64, 2, 3, cond_in=[1]))
    assert not mlp.mlp_supported(_module(3, 5, 64, 2, 3, cond_in=[0, 1]))
    assert not mlp.mlp_supported(_module(3, 0, 256, 2, 3))                      # texture/mlp.yaml's width
    assert not mlp.mlp_supported(_module(3, 0, 64, 2, 3, widths=[64, 32]))
    assert not mlp.mlp_supported(_module(3, 0, 48, 2, 3)) and not mlp.mlp_supported(_module(3, 0, 16, 2, 3))
    assert not mlp.mlp_supported(_module(3, 0, 64, 7, 3)) and mlp.mlp_supported(_module(3, 0, 64, 6, 3))
    assert not mlp.mlp_supported(_module(513, 0, 64, 2, 3)) and mlp.mlp_supported(_module(512, 512, 64, 2, 64))
    assert not mlp.mlp_supported(_module(513, 512, 64, 2, 3)) and not mlp.mlp_supported(_module(3, 0, 64, 2, 65))
    m = _module(*ok)
    m.activation = torch.nn.ReLU()
    assert not mlp.mlp_supported(m)


def _plain_chain(m, x, cond):
    """The same network written out with torch.nn.functional, for the configurations the fallback evaluates."""
    F = torch.nn.functional
    cfg, h = m.config, x
    for l in range(m.num_layers - 1):
        lin = getattr(m, "lin%d" % l)
        if l in cfg["cond_in"]:
            h = torch.cat([h, cond.expand(x.shape[0], -1)], 1)
        if l in cfg["skip_in"]:
            h = torch.cat([h, x], 1) * (1.0 / np.sqrt(2))
        h = F.linear(h, lin.weight, lin.bias)
        if l < m.num_layers - 2:
            h = F.leaky_relu(h, 0.01)
    return h


def test_unsupported_configurations_take_the_torch_path_on_the_cpu():
    torch.manual_seed(5)
    x = torch.rand(9, 3)
    for m, cond in ((_module(3, 0, 256, 2, 3), None), (_module(3, 0, 64, 4, 10, skip_in=(2,)), None),
                    (_module(3, 5, 64, 2, 3, cond_in=[1]), torch.rand(1, 5)), (_module(3, 5, 32, 2, 4), torch.rand(9, 5)),
                    (_module(3, 513, 32, 2, 4), torch.rand(1, 513))):  # (lin0's 516 columns could be 512 + 4: the call knows)
        got, want = m.forward(x, cond=cond), _plain_chain(m, x, cond)
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    # a supported network has no CPU path: the fused kernels are the only implementation
    with pytest.raises(RuntimeError, match="GPU"):
        _module(3, 0, 64, 2, 3).forward(x)
    with pytest.raises(RuntimeError, match="GPU"):
        _module(3, 5, 32, 2, 4).forward(x, cond=torch.rand(1, 5).expand(9, -1))


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import mlp
    n = 5
    W = [torch.zeros(32, 3 + 5), torch.zeros(32, 32), torch.zeros(4, 32)]
    b = [torch.zeros(32), torch.zeros(32), torch.zeros(4)]
    ok = dict(x=torch.zeros(n, 3), weights=W, biases=b, cond=torch.zeros(5))
    call = lambda **over: mlp.fused_mlp(**dict(ok, **over))
    for bad in (dict(x=torch.zeros(n)), dict(x=torch.zeros(n, 4)), dict(cond=None), dict(cond=torch.zeros(6)),
                dict(cond=torch.zeros(2, 5)), dict(cond=torch.zeros(n, 5)), dict(cond=torch.zeros(1, 1, 5)),
                dict(biases=b[:2]), dict(weights=W[:1], biases=b[:1]), dict(biases=[b[0], torch.zeros(31), b[2]]),
                dict(weights=[W[0], torch.zeros(32, 31), W[2]]), dict(weights=[W[0], W[1], torch.zeros(4, 31)]),
                dict(weights=[torch.zeros(48, 8), torch.zeros(48, 48), torch.zeros(4, 48)], biases=[torch.zeros(48), torch.zeros(48), b[2]]),
                dict(weights=[W[0], W[1], torch.zeros(65, 32)], biases=[b[0], b[1], torch.zeros(65)]),
                dict(x=torch.zeros(n, 513), weights=[torch.zeros(32, 513), W[1], W[2]], cond=None),
                dict(weights=[torch.zeros(32, 3), W[1], W[2]])):
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (dict(x=torch.zeros(n, 3, dtype=torch.float64)), dict(cond=torch.zeros(5, dtype=torch.float16)),
                dict(weights=[W[0].double(), W[1], W[2]]), dict(biases=[b[0], b[1].half(), b[2]]), dict(x=[[0.0] * 3] * n)):
        with pytest.raises(TypeError):
            call(**bad)
    for good in ({}, dict(cond=torch.zeros(1, 5)), dict(cond=torch.zeros(1, 5).expand(n, -1)), dict(cond=torch.zeros(5).expand(n, -1))):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**good)


def _err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got).reshape(want.shape) - want).max()) / max(float(np.abs(want).max()), 1e-300)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_restatement_matches_reference_fp64(fx, case):
    x, weights, biases, cond, g = ref.case_call(fx, case)
    got = ref.flat(ref.forward_backward(x, weights, biases, cond, g))
    assert sorted(got) == sorted(ref.result_names(case))
    for name in ref.result_names(case):
        want = fx["%s/%s_f64" % (case, name)]
        assert np.abs(want).max() > 0 and _err(got[name], want) <= 1e-12, (case, name, _err(got[name], want))


def test_fixture_cases_hold_what_they_claim(fx):
    assert sorted(ref.CASES) == ["cond", "in3", "in7"]
    for case, (din, C, width, n_hidden, dout, n) in ref.CASES.items():
        x, weights, biases, cond, g = ref.case_call(fx, case)
        assert x.shape == (n, din) and g.shape == (n, dout) and (cond is None) == (C == 0)
        assert [w.shape for w in weights] == [(width, din + C)] + [(width, width)] * (n_hidden - 1) + [(dout, width)]
        zs = ref.forward(x, weights, biases, cond)[1]
        assert len(zs) == n_hidden and min(np.abs(z).min() for z in zs) > 1e-4
        assert all((z > 0).any() and (z < 0).any() for z in zs)  # both branches of the LeakyReLU are taken
        for name in ref.result_names(case):
            f32, f64 = fx["%s/%s_f32" % (case, name)], fx["%s/%s_f64" % (case, name)]
            assert f32.dtype == np.float32 and f64.dtype == np.float64 and np.isfinite(f64).all()
            assert np.abs(f32 - f64).max() <= 1e-6 * np.abs(f64).max(), (case, name)
    # the filter of random_inputs: what it keeps stays clear of the kink, and it refuses to drop too much
    weights, biases = ref.random_params(3, 0, 128, 4, 25, seed=1)
    x, _, _ = ref.random_inputs(2000, weights, biases, 0, seed=2)
    zs = ref.forward(x, weights, biases)[1]
    assert x.shape == (2000, 3) and min(np.abs(z).min() for z in zs) >= ref.KINK
