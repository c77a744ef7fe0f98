"""The LPIPS-VGG op's C ABI, Python surface and fixture on the CPU (no GPU needed): the new symbols are declared, exported
and bound, the struct mirrors the header's field for field, lpips.hip is built strictly, argument validation works with
never-dereferenced pointers (each limit and one past it), `import lpips` resolves from this tree and rejects what it must
before touching a device, state dicts round-trip in the three accepted spellings, `foreground_box` is train.py:130-133,
and the float64 restatement tests/lpips_ref.py reproduces the fixture tests/golden/lpips.npz to 1e-12."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_header
import lpips_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_lpips_packed_bytes", "gs_lpips_pack_weights", "gs_lpips_workspace_bytes", "gs_lpips_forward", "gs_lpips_backward",
       "gs_lpips_conv", "gs_lpips_pool")
DEFINES = (("GS_LPIPS_LAYERS", 13), ("GS_LPIPS_TAPS", 5), ("GS_LPIPS_MIN_SIZE", 16), ("GS_LPIPS_MAX_SIZE", 2048),
           ("GS_LPIPS_WS_FORWARD", 0), ("GS_LPIPS_WS_SAVED", 1), ("GS_LPIPS_WS_BACKWARD", 2))


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


def test_symbols_declared_exported_and_bound(lib):
    header = abi_header.text()
    capi = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "csrc", "lpips.hip")).read()  # (the module's own boundary)
    lib.load()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, capi, flags=re.M), name
    for name, value in DEFINES:
        assert getattr(lib, name) == value
    # five ints (padded to 24 bytes), four 64-bit strides, then 3 + 13 + 13 + 5 + 2 addresses
    assert ctypes.sizeof(lib.GsLpipsArgs) == 24 + 32 + 36 * ctypes.sizeof(ctypes.c_void_p)
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in ("gs_lpips_forward", "gs_lpips_backward", "gs_lpips_conv"):
        assert name in capture_safe, name
    build_py = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "build.py")).read()
    assert build_py.count('"lpips.hip"') == 2  # SOURCES and STRICT
    strict = build_py[build_py.index("STRICT = {"):build_py.index("}", build_py.index("STRICT = {"))]
    assert '"lpips.hip"' in strict


P, ODD4, ODD16 = 0x1000, 0x1002, 0x1004  # never dereferenced: validation fails first
BIG = 1 << 50


def _args(lib, H=37, W=29, g0=1, g1=0, **over):
    a = lib.GsLpipsArgs()
    a.H, a.W, a.normalize, a.need_grad0, a.need_grad1 = H, W, 1, g0, g1
    a.cs0 = a.cs1 = H * W
    a.rs0 = a.rs1 = W
    a.in0 = a.in1 = a.packed = P
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _saved_floats(H, W):
    px = [(H >> v) * (W >> v) for v in range(5)]
    level = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
    acts = sum(ref.CHANNELS[l + 1] * px[level[l]] for l in range(13))
    return acts + sum(ref.CHANNELS[l + 1] * px[k] for k, l in enumerate(ref.TAP_LAYERS))


def test_workspace_sizes(lib):
    from gsplat_mi355 import lpips as gl
    L = lib.load()
    assert lib.nbytes(L.gs_lpips_packed_bytes) == 4 * (16 + sum(2 * 9 * ref.CHANNELS[l] * ref.CHANNELS[l + 1] + ref.CHANNELS[l + 1]
                                                               for l in range(13)) + 64 + 128 + 256 + 512 + 512)
    for H, W in ((16, 16), (37, 29), (250, 400), (2048, 2048)):
        blocks = sum(-(-((H >> v) * (W >> v)) // 64) for v in range(5))
        full, half = 64 * H * W, 64 * (H >> 1) * (W >> 1)
        for g0, g1 in ((0, 0), (1, 0), (0, 1), (1, 1)):
            ng = g0 + g1
            assert gl.workspace_bytes(H, W, g0, g1, lib.GS_LPIPS_WS_FORWARD) == 4 * (ng * half + (2 - ng) * 2 * full + blocks)
            assert gl.workspace_bytes(H, W, g0, g1, lib.GS_LPIPS_WS_SAVED) == 4 * ng * _saved_floats(H, W)
            assert gl.workspace_bytes(H, W, g0, g1, lib.GS_LPIPS_WS_BACKWARD) == 4 * ng * 2 * full
    # an image without a gradient saves nothing
    assert gl.workspace_bytes(37, 29, 0, 0, lib.GS_LPIPS_WS_SAVED) == 0
    out = ctypes.c_size_t(0)
    for H, W, which in ((15, 16, 0), (16, 15, 0), (2049, 16, 0), (16, 2049, 0), (16, 16, 3), (16, 16, -1)):
        assert L.gs_lpips_workspace_bytes(H, W, 1, 0, which, ctypes.byref(out)) == -1, (H, W, which)
    assert L.gs_lpips_workspace_bytes(16, 16, 1, 0, 0, None) == -1
    assert L.gs_lpips_packed_bytes(None) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()

    def fwd(a, loss=P, taps=P, saved=P, sb=BIG, ws=P, wb=BIG):
        return L.gs_lpips_forward(ctypes.byref(a) if a is not None else None, loss, taps, saved, sb, ws, wb, None)

    def bwd(a, g=P, d0=P, d1=None, saved=P, sb=BIG, ws=P, wb=BIG):
        return L.gs_lpips_backward(ctypes.byref(a) if a is not None else None, g, d0, d1, saved, sb, ws, wb, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        for kw in (dict(H=15), dict(W=15), dict(H=2049), dict(W=2049), dict(in0=None), dict(in1=None), dict(in0=ODD4),
                   dict(packed=None), dict(packed=ODD16), dict(cs0=0), dict(cs1=0), dict(rs0=28), dict(rs1=28)):
            assert call(_args(lib, **kw)) == -1, kw
        assert call(_args(lib), saved=ODD16) == -1 and call(_args(lib), ws=ODD16) == -1 and call(_args(lib), ws=None) == -1
    # the limits themselves pass the shape checks: the workspace check answers
    for kw in (dict(H=16, W=16), dict(H=2048, W=2048), dict(H=16, W=2048)):
        assert fwd(_args(lib, **kw), wb=0) == -5 and bwd(_args(lib, **kw), wb=0) == -5, kw
    a = _args(lib)
    need = lambda which: lib.nbytes(L.gs_lpips_workspace_bytes, 37, 29, 1, 0, which)
    assert fwd(a, sb=need(1) - 1) == -5 and fwd(a, wb=need(0) - 1) == -5
    assert bwd(a, sb=need(1) - 1) == -5 and bwd(a, wb=need(2) - 1) == -5
    assert fwd(a, loss=None) == -1 and fwd(a, loss=ODD4) == -1 and fwd(a, taps=ODD4) == -1 and fwd(a, saved=None) == -1
    assert bwd(a, g=ODD4) == -1 and bwd(a, d0=ODD4) == -1
    assert bwd(a, d1=P) == -1                       # in1 saved nothing: no gradient for it
    assert bwd(_args(lib, g0=0), d0=P) == -1
    assert bwd(a, d0=None, saved=None, ws=None, sb=0, wb=0) == 0  # nothing wanted: nothing to do
    # one layer, and the pools
    conv = lambda layer=1, backward=0, H=3, W=5, packed=P, inp=P, cs=15, rs=5, mask=P, out=P: L.gs_lpips_conv(
        packed, layer, backward, 1, H, W, inp, cs, rs, mask, out, None)
    for kw in (dict(layer=-1), dict(layer=13), dict(H=0), dict(W=0), dict(H=2049), dict(packed=None), dict(packed=ODD16),
               dict(inp=None), dict(inp=ODD16), dict(out=None), dict(out=ODD16), dict(backward=1, mask=None),
               dict(backward=1, mask=ODD16), dict(layer=0, rs=4), dict(layer=0, cs=0), dict(layer=0, inp=ODD4),
               dict(layer=0, backward=1, out=ODD4)):
        assert conv(**kw) == -1, kw
    pool = lambda backward=0, H=3, W=5, C=64, inp=P, g=P, dp=P, out=P: L.gs_lpips_pool(backward, H, W, C, inp, g, dp, out, None)
    for kw in (dict(H=0), dict(W=0), dict(C=0), dict(C=6), dict(C=516), dict(inp=None), dict(out=ODD16), dict(backward=1, g=None),
               dict(backward=1, dp=None)):
        assert pool(**kw) == -1, kw
    pack = lambda a, packed=P, nb=BIG: L.gs_lpips_pack_weights(ctypes.byref(a) if a is not None else None, packed, nb, None)
    full = _args(lib)
    for l in range(13):
        full.weight[l] = full.bias[l] = P
    for k in range(5):
        full.lin[k] = P
    assert pack(None) == -1 and pack(full, packed=None) == -1 and pack(full, packed=ODD16) == -1
    assert pack(full, nb=lib.nbytes(L.gs_lpips_packed_bytes) - 1) == -5
    full.weight[7] = None
    assert pack(full) == -1
    full.weight[7], full.lin[4] = P, ODD4
    assert pack(full) == -1


def test_the_lpips_package_and_what_it_rejects(monkeypatch, tmp_path):
    import lpips
    from gsplat_mi355 import lpips as gl
    assert lpips.LPIPS is gl.LPIPS and lpips.__file__.startswith(os.path.join(ROOT, "3dgs-avatar-release_amd"))
    with pytest.raises(NotImplementedError, match="alex"):
        lpips.LPIPS(pretrained=False)  # upstream's default net
    for kw, word in ((dict(net="squeeze"), "net"), (dict(version="0.0"), "version"), (dict(lpips=False), "lpips"),
                     (dict(spatial=True), "spatial"), (dict(pnet_tune=True), "pnet_tune")):
        with pytest.raises(NotImplementedError, match=word):
            lpips.LPIPS(**dict(dict(net="vgg", pretrained=False), **kw))
    monkeypatch.delenv(gl.WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match=r"torch\.save\(lpips\.LPIPS\(net='vgg'\)\.state_dict\(\), path\)"):
        lpips.LPIPS(net="vgg")
    with pytest.raises(FileNotFoundError):
        lpips.LPIPS(net="vgg", model_path=str(tmp_path / "absent.pth"))
    m = lpips.LPIPS(net="vgg", pretrained=False, verbose=False)
    assert isinstance(m, torch.nn.Module) and not m.training
    assert not m.train().training and not m.train(True).training  # eval mode stays
    x = torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x[None], x[None], normalize=True)
    for bad in (torch.rand(16, 16), torch.rand(1, 16, 16), torch.rand(2, 2, 3, 16, 16)):
        with pytest.raises(ValueError):
            m(bad, bad)
    with pytest.raises(ValueError):
        m(x, torch.rand(3, 16, 17))
    for small in (torch.rand(3, 15, 16), torch.rand(3, 16, 15), torch.rand(3, 16, 2049)):
        with pytest.raises(ValueError, match="16..2048"):
            m(small, small)
    with pytest.raises(TypeError):
        m(x.to(torch.int32), x.to(torch.int32))
    # the weights file: model_path, then the environment variable
    sd = ref.weights()
    path = str(tmp_path / "vgg.pth")
    torch.save(sd, path)
    a = lpips.LPIPS(net="vgg", model_path=path)
    monkeypatch.setenv(gl.WEIGHTS_ENV, path)
    b = lpips.LPIPS(net="vgg")
    for got in (a.state_dict(), b.state_dict()):
        assert list(got) == gl.state_dict_keys() and all(torch.equal(got[k], sd[k]) for k in sd)


def test_state_dict_spellings_and_errors():
    import lpips
    from gsplat_mi355 import lpips as gl
    sd = ref.weights()
    m = lpips.LPIPS(net="vgg", pretrained=False)
    keys = gl.state_dict_keys()
    assert keys[:2] == ["scaling_layer.shift", "scaling_layer.scale"] and keys[2] == "net.slice1.0.weight"
    assert keys[-1] == "lin4.model.1.weight" and "net.slice5.28.bias" in keys and len(keys) == 2 + 26 + 5
    m.load_state_dict(sd)
    got = m.state_dict()
    assert list(got) == keys and all(torch.equal(got[k], sd[k]) for k in keys)  # round trip
    # lins.{k} instead of lin{k}; a torchvision trunk (features.N) without the scaling layer
    lins = collections.OrderedDict((re.sub(r"^lin(\d)\.", r"lins.\1.", k), v) for k, v in sd.items())
    tv = collections.OrderedDict()
    for k, v in sd.items():
        mm = re.match(r"net\.slice\d\.(\d+)\.(weight|bias)", k)
        if mm:
            tv["features.%s.%s" % mm.groups()] = v
        elif k.startswith("lin"):
            tv[k] = v
    both = collections.OrderedDict(sd)
    both.update((k, v) for k, v in lins.items() if k.startswith("lins."))  # (upstream lists the lin layers under both names)
    for spelled in (lins, tv, both):
        m2 = lpips.LPIPS(net="vgg", pretrained=False)
        m2.load_state_dict(spelled)
        got = m2.state_dict()
        assert list(got) == keys and all(torch.equal(got[k], sd[k]) for k in keys if not k.startswith("scaling"))
        assert torch.allclose(got["scaling_layer.shift"].flatten(), torch.tensor(ref.SHIFT))
    custom = collections.OrderedDict(sd)
    custom["scaling_layer.shift"] = torch.tensor([0.1, 0.2, 0.3])
    m.load_state_dict(custom)
    assert torch.equal(m.state_dict()["scaling_layer.shift"].flatten(), custom["scaling_layer.shift"])
    # every missing or mis-shaped entry is named
    broken = collections.OrderedDict(sd)
    del broken["lin3.model.1.weight"], broken["net.slice2.7.bias"]
    broken["net.slice4.19.weight"] = torch.zeros(512, 256, 3, 3)
    broken["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    with pytest.raises(ValueError) as e:
        m.load_state_dict(broken)
    for word in ("lin3.model.1.weight", "net.slice2.7.bias", "net.slice4.19.weight", "lin0.model.1.weight"):
        assert word in str(e.value), word
    short = collections.OrderedDict((k, v) for k, v in sd.items() if "slice5" not in k)
    with pytest.raises(ValueError, match="found 10"):
        m.load_state_dict(short)
    # pretrained=False: seeded, He-scaled
    r0, r1 = gl.random_state_dict(0), gl.random_state_dict(0)
    assert all(torch.equal(r0[k], r1[k]) for k in keys)
    w = r0["net.slice3.12.weight"]
    assert abs(float(w.std()) / np.sqrt(2.0 / (9 * 256)) - 1) < 0.01 and float(r0["lin2.model.1.weight"].min()) >= 0


def test_foreground_box_and_its_cache():
    from gsplat_mi355 import lpips as gl
    rng = np.random.default_rng(3)
    masks = [np.zeros((1, 12, 9), bool) for _ in range(6)]
    masks[0][0, 4, 7] = True                       # one pixel
    masks[1][0, 0, :] = True                       # the top row, border to border
    masks[2][0, :, 8] = True                       # the right column
    masks[3][0] = True                             # everything
    masks[4][0, 11, 0] = masks[4][0, 0, 8] = True  # two corners
    masks[5][0, 3:9, 2:5] = rng.random((6, 3)) > 0.4
    for m in masks:
        w = np.where(m)
        want = (w[1].min(), w[1].max() + 1, w[2].min(), w[2].max() + 1)  # train.py:131-133
        for given in (torch.from_numpy(m), torch.from_numpy(m).float(), torch.from_numpy(m[0]), m):
            got = gl.foreground_box(given)
            assert got == tuple(int(v) for v in want) and all(type(v) is int for v in got)
    assert gl.foreground_box(torch.from_numpy(masks[0])) == (4, 5, 7, 8)
    with pytest.raises(ValueError):
        gl.foreground_box(torch.zeros(1, 4, 4))

    class Camera(object):
        pass

    cam = Camera()
    cam.original_mask = torch.from_numpy(masks[5])
    calls = []
    out = gl.perceptual_loss(lambda a, b, normalize: calls.append((a, b, normalize)) or torch.ones(1, 1, 1, 1),
                             torch.rand(3, 12, 9), torch.rand(3, 12, 9), cam)
    box = cam._gsplat_foreground_box
    assert box == gl.foreground_box(cam.original_mask) and float(out) == 1.0
    a, b, normalize = calls[0]
    assert normalize is True and tuple(a.shape) == (3, box[1] - box[0], box[3] - box[2]) and a.shape == b.shape
    cam.original_mask = None  # a second call does not look at the mask again
    gl.perceptual_loss(lambda a, b, normalize: torch.ones(1), torch.rand(3, 12, 9), torch.rand(3, 12, 9), cam)
    assert cam._gsplat_foreground_box is box


def test_weights_are_the_fixtures(fx):
    assert int(fx["weight_seed"][0]) == ref.WEIGHT_SEED
    got, want = ref.checksums(ref.weights()), fx["weight_checksums"]
    assert got.shape == want.shape == (18, 2)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), "the weight generator changed: regenerate the fixture"


@pytest.mark.parametrize("case", list(ref.CASES))
def test_restatement_reproduces_the_fixture(fx, case):
    h, w, normalize = ref.CASES[case]
    a, b = torch.from_numpy(fx[case + "/in0"]), torch.from_numpy(fx[case + "/in1"])
    assert tuple(a.shape) == (3, h, w) and a.dtype == torch.float32
    sa, sb = ref.images(h, w, int(fx[case + "/seed"][0]))
    assert torch.equal(a, sa) and torch.equal(b, sb)
    got, margin = ref.forward_backward(a, b, ref.weights(), normalize)
    assert margin >= ref.MARGIN and abs(margin - float(fx[case + "/margin"][0])) <= 1e-6 * margin
    for q in ref.QUANTITIES:
        want = fx["%s/%s_f64" % (case, q)]
        assert want.dtype == np.float64 and np.abs(want).max() > 0
        assert ref.rel_err(got[q], want) <= 1e-12, (case, q, ref.rel_err(got[q], want))
        assert 0 < float(fx["%s/%s_err_f32" % (case, q)][0]) < 1e-5
    assert abs(float(got["taps"].sum()) - float(got["loss"][0])) <= 1e-15
