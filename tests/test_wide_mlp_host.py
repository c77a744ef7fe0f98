"""The wide fused MLP's C ABI, Python entry points and fixture on the CPU (no GPU needed): the module's own header
(include/gsplat_mi355_wmlp.h) and its own binding (gsplat_mi355/_wide_lib.py) agree, argument validation works with never-dereferenced pointers (each limit and one past it), the byte
counts come from the library, the Python functions reject what they must before touching a device, `wide_mlp_supported`
takes the reference's three networks and turns down what the kernels do not cover while `mlp_supported` keeps its
answers, CPU tensors keep taking the torch path, `hann_band_weights` gives the reference's window, and the float64
restatement tests/wide_mlp_ref.py reproduces the reference's own fp64 autograd results (tests/golden/wide_mlp.npz) to
1e-12 and its fp32 ones to the fixture generator's own fp32-against-fp64 bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_header
import wide_mlp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_wmlp_workspace_bytes", "gs_wmlp_saved_bytes", "gs_wmlp_forward", "gs_wmlp_backward")
DEFINES = (("GS_WMLP_MAX_WIDTH", 256), ("GS_WMLP_MAX_HIDDEN", 8), ("GS_WMLP_MAX_LAYERS", 9), ("GS_WMLP_MAX_FREQS", 10),
           ("GS_WMLP_MAX_ENC", 512), ("GS_WMLP_MAX_COND", 512), ("GS_WMLP_MAX_OUT", 64), ("GS_WMLP_TILE_ROWS", 128),
           ("GS_WMLP_PARTIAL_MIN_ROWS", 256), ("GS_WMLP_MAX_PARTIALS", 128))
F32_BOUND = 1e-6  # tests/golden/make_wide_mlp_golden.py: the reference's fp32 against its fp64


WIDE_HEADER = os.path.join(ROOT, "include", "gsplat_mi355_wmlp.h")


@pytest.fixture(scope="module")
def lib():
    """gsplat_mi355._wide_lib, the binding of include/gsplat_mi355_wmlp.h (the library is built first when it is missing)."""
    abi_header.lib()
    from gsplat_mi355 import _wide_lib
    return _wide_lib


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "wide_mlp.npz"))


def test_the_binding_is_what_the_header_declares(lib, tmp_path):
    """The wide MLP's own header against its own table, as tests/test_cabi_host.py holds gsplat_mi355.h against _lib.py:
    every function's arguments, the struct's fields and layout (the compiler's), every constant."""
    from test_cabi_host import abi_mismatch
    text = open(WIDE_HEADER).read()
    header = abi_header.parse(text)
    L = lib.load()
    assert list(header.functions) == list(lib.SIGNATURES) == list(NEW)
    wrong = []
    for name, fn in header.functions.items():
        restype, argtypes = lib.SIGNATURES[name]
        assert tuple(fn.restype) == ("int", False, 0) and restype is ctypes.c_int and len(argtypes) == len(fn.params), name
        wrong += ["%s(%s): %s" % (name, pname, abi_mismatch(ct, t)) for ct, (pname, t) in zip(argtypes, fn.params) if abi_mismatch(ct, t)]
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name
    assert list(header.structs) == ["GsWideMlpArgs"]
    fields = header.structs["GsWideMlpArgs"]
    assert [f[0] for f in lib.GsWideMlpArgs._fields_] == [f.name for f in fields]
    wrong += ["GsWideMlpArgs.%s: %s" % (f.name, abi_mismatch(ct, f.type, f.length))
              for (_, ct), f in zip(lib.GsWideMlpArgs._fields_, fields) if abi_mismatch(ct, f.type, f.length)]
    assert wrong == []
    bound = {n: v for n, v in vars(lib).items() if n.startswith("GS_") and isinstance(v, int)}
    assert bound == dict(header.constants) == dict(DEFINES)
    assert lib.GS_WMLP_MAX_LAYERS == lib.GS_WMLP_MAX_HIDDEN + 1
    # the layout, from the compiler
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gsplat_mi355_wmlp.h"', "int main() {",
             '    printf("size %zu\\n", sizeof(GsWideMlpArgs));']
    lines += ['    printf("%s %%zu\\n", offsetof(GsWideMlpArgs, %s));' % (f.name, f.name) for f in fields]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    cc = abi_header.build_module().hipcc()
    r = subprocess.run([cc, "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {"size": str(ctypes.sizeof(lib.GsWideMlpArgs))}
    want.update({n: str(getattr(lib.GsWideMlpArgs, n).offset) for n, _ in lib.GsWideMlpArgs._fields_})
    assert got == want
    # eight ints, the mask, the slope and ten band weights (80 bytes), then 2 + 4 x 9 + 2 addresses
    assert ctypes.sizeof(lib.GsWideMlpArgs) == 80 + 40 * ctypes.sizeof(ctypes.c_void_p)
    assert "Capture-safe" in text and all(name in text[text.index("Capture-safe"):] for name in NEW[2:])


def test_the_module_is_built_strict_and_leaves_the_narrow_path_s_abi_alone():
    from gsplat_mi355 import _lib
    build_py = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "build.py")).read()
    assert build_py.count('"mlp_wide.hip"') == 2  # SOURCES and STRICT
    assert "gsplat_mi355_wmlp.h" in build_py      # a change of the header rebuilds the library
    # the narrow path's constants stay what tests/test_mlp_host.py pins, and gsplat_mi355.h's table is the frame's and the
    # narrow modules' alone (tests/test_aux_boundary_host.py pins every one of its entry points)
    assert (_lib.GS_MLP_MAX_WIDTH, _lib.GS_MLP_MAX_HIDDEN, _lib.GS_MLP_TILE_ROWS) == (128, 6, 128)
    assert not any(name.startswith("gs_wmlp") for name in _lib.SIGNATURES) and "gs_wmlp" not in abi_header.text()


P, ODD4, ODD16 = 0x1000, 0x1002, 0x1004  # never dereferenced: validation fails first


def _args(lib, N=300, d=3, multires=6, include_input=1, C=5, width=256, n_hidden=8, dout=26, skip_mask=1 << 4, slope=0.01,
          grads=True, **over):
    a = lib.GsWideMlpArgs()
    a.N, a.dim_x, a.multires, a.include_input, a.dim_cond = N, d, multires, include_input, C
    a.width, a.n_hidden, a.dim_out, a.skip_mask, a.slope = width, n_hidden, dout, skip_mask, slope
    for k in range(10):
        a.band_w[k] = 1.0
    a.x = P
    a.cond = P if C else None
    for l in range(min(max(n_hidden, 0), 8) + 1):
        a.W[l] = a.b[l] = P
        if grads:
            a.dW[l] = a.db[l] = P
    if grads:
        a.dx = P
        a.dcond = P if C else None
    for k, v in over.items():
        if k in ("W", "b", "dW", "db", "band_w"):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_byte_counts_come_from_the_library(lib):
    from gsplat_mi355 import wide_mlp
    L = lib.load()
    ws = lambda a, bwd: lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), bwd)
    saved = lambda a: lib.nbytes(L.gs_wmlp_saved_bytes, ctypes.byref(a))
    for n, rows in ((1, 256), (256, 256), (32768, 256), (32769, 288), (200000, 1568)):
        assert wide_mlp.rows_per_partial(n) == rows and -(-n // rows) <= lib.GS_WMLP_MAX_PARTIALS
    # (d, multires, include_input, C, width, n_hidden, dout, skips)
    for d, m, inc, C, W, nh, dout, skips in ((3, 6, 1, 144, 256, 8, 26, (4,)), (3, 6, 0, 144, 256, 8, 10, (4,)),
                                              (271, 0, 1, 0, 256, 4, 3, ()), (7, 0, 1, 0, 64, 2, 4, (1, 2))):
        E = d * (inc + 2 * m) if m else d
        outs = [dout if l == nh else (W - E if l + 1 in skips else W) for l in range(nh + 1)]
        part = sum(o * ((E if l == 0 else W) + 1) for l, o in enumerate(outs))
        for n in (1, 257, 33000):
            a = _args(lib, n, d, m, inc, C, W, nh, dout, sum(1 << l for l in skips))
            assert saved(a) == 4 * nh * n * W
            assert ws(a, 0) == (4 * W if C else 0)
            parts = -(-n // wide_mlp.rows_per_partial(n))
            assert ws(a, 1) == 4 * (nh * n * W + (n * E if m else 0) + parts * part), (d, m, n)
    # at 200k rows the 8 x 256 network saves 1.6 GB (what torch's autograd keeps of it, too)
    assert saved(_args(lib, 200000)) == 8 * 200000 * 256 * 4
    assert ws(_args(lib, 0), 0) == 0 and ws(_args(lib, 0), 1) == 0 and saved(_args(lib, 0)) == 0
    out = ctypes.c_size_t(0)
    assert L.gs_wmlp_workspace_bytes(None, 1, ctypes.byref(out)) == -1 and L.gs_wmlp_saved_bytes(None, ctypes.byref(out)) == -1
    assert L.gs_wmlp_workspace_bytes(ctypes.byref(_args(lib)), 1, None) == -1
    assert L.gs_wmlp_saved_bytes(ctypes.byref(_args(lib)), None) == -1
    assert L.gs_wmlp_saved_bytes(ctypes.byref(_args(lib, width=288)), ctypes.byref(out)) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    BIG = 1 << 40

    def fwd(a, y=P, saved=P, ws=P, nbytes=BIG):
        return L.gs_wmlp_forward(ctypes.byref(a) if a is not None else None, y, saved, ws, nbytes, None)

    def bwd(a, saved=P, g=P, ws=P, nbytes=BIG):
        return L.gs_wmlp_backward(ctypes.byref(a) if a is not None else None, saved, g, ws, nbytes, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        assert call(_args(lib, N=-1)) == -1
        assert call(_args(lib, N=0)) == 0 and call(_args(lib, N=0, x=None)) == 0  # no rows: nothing to do
        for kw in (dict(width=0), dict(width=16), dict(width=48), dict(width=288), dict(n_hidden=0), dict(n_hidden=9, skip_mask=0),
                   dict(d=0), dict(multires=-1), dict(multires=11), dict(include_input=2), dict(C=-1), dict(C=513),
                   dict(dout=0), dict(dout=65), dict(slope=float("nan")), dict(slope=-0.1), dict(slope=float("inf")),
                   dict(skip_mask=1), dict(skip_mask=1 | 1 << 4), dict(skip_mask=1 << 9), dict(n_hidden=3, skip_mask=1 << 4),
                   dict(d=20, skip_mask=1 << 4),                 # E = 260 >= W with a skip
                   dict(d=64, multires=0, width=64, skip_mask=2),  # E == W with a skip
                   dict(d=25, multires=10, skip_mask=0),          # E = 525 > 512
                   dict(d=513, multires=0, skip_mask=0), dict(band_w=(2, float("nan")))):
            assert call(_args(lib, **kw)) == -1, kw
        assert call(_args(lib, x=None)) == -1 and call(_args(lib, x=ODD4)) == -1
        assert call(_args(lib, cond=None)) == -1 and call(_args(lib, cond=ODD4)) == -1
        for l in (0, 4, 8):
            assert call(_args(lib, W=(l, None))) == -1 and call(_args(lib, b=(l, None))) == -1, l
            assert call(_args(lib, W=(l, ODD4))) == -1 and call(_args(lib, b=(l, ODD4))) == -1, l
    # every limit itself passes the shape checks: the workspace check answers the backward
    for kw in (dict(width=32, d=1, multires=2), dict(width=256), dict(n_hidden=1, skip_mask=2), dict(n_hidden=8, skip_mask=1 << 8),
               dict(multires=10, include_input=0), dict(d=512, multires=0, skip_mask=0), dict(d=32, multires=8, include_input=0, skip_mask=0),
               dict(C=512), dict(C=0), dict(dout=1), dict(dout=64), dict(slope=0.0), dict(skip_mask=0b111111110),
               dict(band_w=(9, float("nan")))):  # (a band past multires is not read)
        assert bwd(_args(lib, **kw), nbytes=0) == -5, kw
    assert fwd(_args(lib, C=1), nbytes=4 * 256 - 1) == -5 and fwd(_args(lib, C=512), ws=None) == -1
    assert fwd(_args(lib), ws=ODD4) == -1
    assert fwd(_args(lib), y=None) == -1 and fwd(_args(lib), y=ODD4) == -1 and fwd(_args(lib), saved=ODD16) == -1
    assert bwd(_args(lib), saved=None) == -1 and bwd(_args(lib), saved=ODD16) == -1
    assert bwd(_args(lib), g=None) == -1 and bwd(_args(lib), g=ODD16) == -1
    assert bwd(_args(lib), ws=None) == -1 and bwd(_args(lib), ws=ODD16) == -1
    assert bwd(_args(lib, dx=ODD4)) == -1 and bwd(_args(lib, dcond=ODD4)) == -1
    assert bwd(_args(lib, dW=(1, ODD4))) == -1 and bwd(_args(lib, db=(8, ODD4))) == -1
    assert bwd(_args(lib, C=0, dcond=P)) == -1  # no condition: no dL_dcond
    a = _args(lib)
    need = lib.nbytes(L.gs_wmlp_workspace_bytes, ctypes.byref(a), 1)
    assert bwd(a, nbytes=need - 1) == -5
    # nothing wanted: nothing to do (and nothing launched)
    assert bwd(_args(lib, grads=False), ws=None, nbytes=0) == 0


def _module(cfg, cond_in=None, activation=None, hannw=False):
    """What VanillaCondMLP.__init__ / HannwCondMLP.__init__ leave on the module, as far as the forwards and
    wide_mlp_supported read it."""
    from gsplat_mi355 import mlp, wide_mlp
    C = cfg["C"]
    cond_in = ([0] if C else []) if cond_in is None else cond_in
    m = torch.nn.Module()
    m.config = dict(multires=cfg["multires"], skip_in=list(cfg["skip_in"]), cond_in=list(cond_in), n_neurons=cfg["width"],
                    n_hidden_layers=cfg["n_hidden"])
    if hannw:
        m.config["embedder"] = dict(ref.HANNW_EMBEDDER)
    m.num_layers = cfg["n_hidden"] + 2
    m.embed_fn = None
    if cfg["multires"] > 0 and not hannw:
        m.embed_fn = lambda x: torch.cat([x] + [f(x * 2.0 ** k) for k in range(cfg["multires"]) for f in (torch.sin, torch.cos)], -1)
    E = ref.enc_dim(cfg)
    for l, (out, fan_in) in enumerate(ref.layer_shapes(cfg)):
        fan_in = (E if l == 0 else fan_in) + (C if l in cond_in else 0)
        setattr(m, "lin%d" % l, torch.nn.Linear(fan_in, max(out, 0)))
    m.activation = activation or (torch.nn.ReLU() if hannw else torch.nn.LeakyReLU())
    if hannw:
        m.forward = lambda coords, iteration, cond=None: wide_mlp.hannw_mlp_forward(m, coords, iteration, cond)
    else:
        m.forward = lambda coords, cond=None: mlp.mlp_forward(m, coords, cond)
    return m


def test_wide_mlp_supported():
    from gsplat_mi355 import mlp, wide_mlp
    ok = wide_mlp.wide_mlp_supported
    assert ok(_module(ref.NONRIGID)) and ok(_module(ref.HANNW, hannw=True)) and ok(_module(ref.TEXTURE))
    for m in (_module(ref.NONRIGID), _module(ref.HANNW, hannw=True), _module(ref.TEXTURE)):
        assert not mlp.mlp_supported(m)
    small = ref.net(3, 6, 5, 64, 3, (2,), 4)
    assert ok(_module(small)) and ok(_module(dict(small, width=160))) and ok(_module(dict(small, width=224)))
    assert ok(_module(dict(small, n_hidden=8))) and ok(_module(dict(small, multires=10, width=96)))
    assert ok(_module(dict(small, dout=64))) and ok(_module(dict(small, skip_in=(1, 3)))) and ok(_module(dict(small, skip_in=(3,))))
    assert not ok(_module(small, cond_in=[1]))
    assert not ok(_module(small, cond_in=[0, 1]))
    assert not ok(_module(dict(small, skip_in=(0,))))
    assert not ok(_module(dict(small, skip_in=(4,))))                          # past the last linear
    assert not ok(_module(ref.net(64, 0, 0, 64, 2, (1,), 4)))                  # E == W with a skip
    assert not ok(_module(ref.net(3, 10, 0, 32, 2, (1,), 4)))                  # E = 63 >= W = 32 with a skip
    assert not ok(_module(dict(small, width=288))) and not ok(_module(dict(small, width=48)))
    assert not ok(_module(dict(small, n_hidden=9)))
    assert not ok(_module(dict(small, multires=11, width=128)))
    assert not ok(_module(dict(small, dout=65)))
    assert not ok(_module(small, activation=torch.nn.Tanh()))
    assert not ok(_module(ref.net(513, 0, 0, 64, 2, (), 4)))
    bent = _module(small)
    bent.lin1 = torch.nn.Linear(64, 64)  # the layer before the skip keeps all W outputs: not the reference's construction
    assert not ok(bent)


def test_the_narrow_path_keeps_its_answers():
    """mlp_supported's answers as tests/test_mlp_host.py lists them, and networks both paths could take stay narrow."""
    from gsplat_mi355 import mlp, wide_mlp
    for shape in ((3, 0, 128, 4, 25), (32, 144, 128, 3, 26), (79, 0, 64, 2, 3)):  # the default config's networks
        d, C, width, nh, dout = shape
        m = _module(ref.net(d, 0, C, width, nh, (), dout))
        assert mlp.mlp_supported(m) and wide_mlp.wide_mlp_supported(m)
    assert not mlp.mlp_supported(_module(ref.net(3, 0, 0, 256, 2, (), 3)))
    assert not mlp.mlp_supported(_module(ref.net(3, 6, 0, 64, 2, (), 3)))
    assert not mlp.mlp_supported(_module(ref.net(3, 0, 0, 64, 2, (2,), 3)))
    relu = _module(ref.net(3, 0, 0, 64, 2, (), 3), activation=torch.nn.ReLU())
    assert not mlp.mlp_supported(relu) and wide_mlp.wide_mlp_supported(relu)
    assert sorted(wide_mlp.DISPATCH) == ["coordinate", "hannw", "plain"]


def _plain_chain(m, x, cond, first):
    F = torch.nn.functional
    cfg, h = m.config, first
    for l in range(m.num_layers - 1):
        lin = getattr(m, "lin%d" % l)
        if l in cfg["cond_in"]:
            h = torch.cat([h, cond.expand(x.shape[0], -1)], 1)
        if l in cfg["skip_in"]:
            h = torch.cat([h, first], 1) * (1.0 / np.sqrt(2))
        h = F.linear(h, lin.weight, lin.bias)
        if l < m.num_layers - 2:
            h = m.activation(h)
    return h


def test_cpu_tensors_take_the_torch_path(monkeypatch):
    """Whatever DISPATCH says: the wide kernels are for device tensors, and mlp_forward's CPU behaviour is pinned."""
    from gsplat_mi355 import wide_mlp
    monkeypatch.setattr(wide_mlp, "DISPATCH", {"coordinate": True, "hannw": True, "plain": True})
    torch.manual_seed(7)
    x, cond = torch.rand(9, 3), torch.rand(1, 5)
    small = ref.net(3, 6, 5, 64, 3, (2,), 4)
    m = _module(small)
    got = m.forward(x, cond=cond)
    assert torch.allclose(got, _plain_chain(m, x, cond, m.embed_fn(x)), rtol=1e-6, atol=1e-7)
    wide = _module(ref.net(3, 0, 0, 256, 2, (), 3))
    assert torch.allclose(wide.forward(x), _plain_chain(wide, x, None, x), rtol=1e-6, atol=1e-7)
    h = _module(dict(small, include_input=False, slope=0.0, dout=10), hannw=True)
    band = wide_mlp.hann_band_weights(ref.HANNW_EMBEDDER, 6, 5800)
    first = torch.cat([w * f(x * 2.0 ** k) for k, w in enumerate(band) for f in (torch.sin, torch.cos)], -1)
    assert torch.allclose(h.forward(x, 5800, cond=cond), _plain_chain(h, x, cond, first), rtol=1e-6, atol=1e-7)


def test_hann_band_weights(fx):
    from gsplat_mi355 import wide_mlp
    for case, iteration in ref.HANNW_ITERATIONS.items():
        got = np.array(wide_mlp.hann_band_weights(ref.HANNW_EMBEDDER, 6, iteration), np.float32)
        want = fx[case + "/band"]
        assert want.dtype == np.float32 and got.shape == want.shape
        assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))).all(), (case, got, want)
        assert np.allclose(got, ref.hann_weights(6, iteration, **ref.HANNW_EMBEDDER), atol=1e-6)
    assert fx["hannw_before/band"].tolist() == [0.0] * 6 and fx["hannw_full/band"].tolist() == [1.0] * 6
    assert fx["hannw_mid/band"][:2].tolist() == [1.0, 1.0] and 0.3 < fx["hannw_mid/band"][2] < 0.4
    for cfg in (dict(kick_in_iter=3000, full_band_iter=0), dict(kick_in_iter=3000, full_band_iter=-1),
                dict(kick_in_iter=3000, full_band_iter=3000), dict(kick_in_iter=5000, full_band_iter=3000)):
        for iteration in (0, 1000, 100000):
            assert wide_mlp.hann_band_weights(cfg, 6, iteration) == (1.0,) * 6
    assert wide_mlp.hann_band_weights(ref.HANNW_EMBEDDER, 10, 10 ** 6) == (1.0,) * 10
    assert all(isinstance(w, float) for w in wide_mlp.hann_band_weights(ref.HANNW_EMBEDDER, 6, 5800))


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import wide_mlp
    n, cfg = 5, ref.net(3, 2, 5, 32, 2, (2,), 4)  # E = 15
    shapes = ref.layer_shapes(cfg)
    assert shapes == [(32, 20), (17, 32), (4, 32)]
    W = [torch.zeros(*s) for s in shapes]
    b = [torch.zeros(s[0]) for s in shapes]
    ok = dict(x=torch.zeros(n, 3), weights=W, biases=b, cond=torch.zeros(5), multires=2, skip_in=(2,))
    call = lambda **over: wide_mlp.fused_wide_mlp(**dict(ok, **over))
    for bad in (dict(x=torch.zeros(n)), dict(x=torch.zeros(n, 4)), dict(cond=None), dict(cond=torch.zeros(6)),
                dict(cond=torch.zeros(2, 5)), dict(cond=torch.zeros(n, 5)), dict(cond=torch.zeros(1, 1, 5)),
                dict(biases=b[:2]), dict(weights=W[:1], biases=b[:1]), dict(biases=[b[0], torch.zeros(16), b[2]]),
                dict(weights=[W[0], torch.zeros(32, 32), W[2]]),      # the layer before the skip must have W - E outputs
                dict(weights=[W[0], torch.zeros(17, 31), W[2]]), dict(skip_in=(0,)), dict(skip_in=(3,)), dict(skip_in=(1,)),
                dict(multires=11), dict(multires=-1), dict(multires=3), dict(include_input=False),
                dict(band_weights=(1.0,)), dict(band_weights=(1.0, float("nan"))), dict(negative_slope=-0.5),
                dict(negative_slope=float("nan")),
                dict(weights=[W[0], W[1], torch.zeros(65, 32)], biases=[b[0], b[1], torch.zeros(65)]),
                dict(x=torch.zeros(n, 11), multires=1, cond=None)):   # E = 33 >= W with a skip
        with pytest.raises(ValueError):
            call(**bad)
    wide = [torch.zeros(288, 3), torch.zeros(288, 288), torch.zeros(4, 288)]
    with pytest.raises(ValueError):
        wide_mlp.fused_wide_mlp(torch.zeros(n, 3), wide, [torch.zeros(288), torch.zeros(288), torch.zeros(4)])
    for bad in (dict(x=torch.zeros(n, 3, dtype=torch.float64)), dict(cond=torch.zeros(5, dtype=torch.float16)),
                dict(weights=[W[0].double(), W[1], W[2]]), dict(biases=[b[0], b[1].half(), b[2]]), dict(x=[[0.0] * 3] * n)):
        with pytest.raises(TypeError):
            call(**bad)
    for good in ({}, dict(cond=torch.zeros(1, 5)), dict(cond=torch.zeros(1, 5).expand(n, -1)), dict(cond=torch.zeros(5).expand(n, -1)),
                 dict(band_weights=(1.0, 0.25)), dict(negative_slope=0.0)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**good)


def _err(got, want):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max())
    return err / scale if scale > 0 else err


@pytest.mark.parametrize("case", list(ref.CASES))
def test_restatement_matches_reference(fx, case):
    cfg = ref.CASES[case]
    x, weights, biases, cond, g, band = ref.case_call(fx, case)
    got = ref.flat(ref.forward_backward(x, weights, biases, cfg, cond, g, band))
    assert sorted(got) == sorted(ref.result_names(cfg))
    for name in ref.result_names(cfg):
        f32, f64 = fx["%s/%s_f32" % (case, name)], fx["%s/%s_f64" % (case, name)]
        assert f32.dtype == np.float32 and f64.dtype == np.float64 and np.isfinite(f64).all()
        # (before kick-in every band weight is 0: dx and the encoding's columns of dW0 are exactly 0)
        assert np.abs(f64).max() > 0 or (case == "hannw_before" and name == "dx"), (case, name)
        assert _err(got[name], f64) <= 1e-12, (case, name, _err(got[name], f64))
        assert _err(got[name], f32) <= F32_BOUND, (case, name, _err(got[name], f32))


def test_fixture_cases_hold_what_they_claim(fx):
    assert list(ref.CASES) == ["enc_skip", "enc_only", "skip_plain", "hannw_before", "hannw_mid", "hannw_full"]
    for case, cfg in ref.CASES.items():
        x, weights, biases, cond, g, band = ref.case_call(fx, case)
        assert x.shape == (ref.ROWS, cfg["d"]) and g.shape == (ref.ROWS, cfg["dout"]) and (cond is None) == (cfg["C"] == 0)
        assert [w.shape for w in weights] == ref.layer_shapes(cfg) and cfg["width"] == 64
        zs = ref.forward(x, weights, biases, cfg, cond, band)[1]
        assert len(zs) == cfg["n_hidden"] and min(np.abs(z).min() for z in zs) > 1e-4
        assert all((z > 0).any() and (z < 0).any() for z in zs)  # both branches of the activation are taken
    # the filter of random_inputs on the three full networks: what it keeps stays clear of the kink, within its cap
    for k, cfg in enumerate((ref.NONRIGID, ref.HANNW, ref.TEXTURE)):
        weights, biases = ref.random_params(cfg, seed=10 + k)
        x, cond, _ = ref.random_inputs(300, weights, biases, cfg, seed=20 + k)
        _, zs, _ = ref.forward(x, weights, biases, cfg, cond)
        assert x.shape == (300, cfg["d"]) and min(np.abs(z).min() for z in zs) >= ref.KINK
        assert all(0.3 < z.std() < 2.5 for z in zs), [z.std() for z in zs]
