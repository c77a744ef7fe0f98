"""The skinning regulariser's C ABI, Python entry points, fixture and restatement on the CPU (no GPU needed): the new symbols
are declared and exported, the workspace size and the argument validation work without a device, the Python functions
reject what they must before touching one, MeshSampler's cumulative areas are what the kernel's face pick needs, and the
float64 restatement tests/skinning_loss_ref.py reproduces the reference's own fp64 autograd results
(tests/golden/skinning_loss.npz) to 1e-12."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import abi_header
import skinning_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_mesh_sample", "gs_skin_loss_workspace_bytes", "gs_skin_loss_forward", "gs_skin_loss_backward")


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "skinning_loss.npz"))


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    header = abi_header.text()
    capture = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in ("gs_mesh_sample", "gs_skin_loss_forward", "gs_skin_loss_backward"):
        assert name in capture, name


def test_workspace_size(lib):
    L = lib.load()
    ws = lambda n: lib.nbytes(L.gs_skin_loss_workspace_bytes, n)
    for n, blocks in ((0, 0), (1, 1), (256, 1), (257, 2), (1024, 4), (1025, 5)):  # one double per block of 256 rows
        assert ws(n) == blocks * 8, n
    out = ctypes.c_size_t(0)
    assert L.gs_skin_loss_workspace_bytes(-1, ctypes.byref(out)) == -1
    assert L.gs_skin_loss_workspace_bytes(10, None) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    a, mis = 0x1000, 0x1004  # never dereferenced: validation fails first (0x1004: 4-byte but not 16-byte aligned)

    def sample(n=10, V=5, F=4, verts=a, faces=a, cdf=a, vw=a, lo=a, inv=a, draws=a, pn=a, tg=a, face=a, bary=a, pts=a):
        return L.gs_mesh_sample(n, V, F, verts, faces, cdf, vw, lo, inv, draws, pn, tg, face, bary, pts, None)

    assert sample(n=-1) == -1 and sample(V=0) == -1 and sample(F=0) == -1 and sample(F=-3) == -1
    for arg in ("verts", "faces", "cdf", "vw", "lo", "inv", "draws", "pn", "tg"):
        assert sample(**{arg: None}) == -1, arg
    for arg in ("vw", "pn", "tg", "bary", "pts"):  # 16-byte accesses
        assert sample(**{arg: mis}) == -1, arg
    for arg in ("verts", "faces", "cdf", "lo", "inv", "draws", "face"):
        assert sample(**{arg: 0x1002}) == -1, arg
    assert sample(n=0, draws=None, pn=None, tg=None, face=None, bary=None, pts=None) == 0  # n = 0 enqueues nothing
    assert sample(n=0, F=0, draws=None, pn=None, tg=None) == -1                          # but the mesh is still checked

    nb = lib.nbytes(L.gs_skin_loss_workspace_bytes, 600)

    def fwd(n=600, kind=0, x=a, tg=a, loss=a, ws=a, b=nb):
        return L.gs_skin_loss_forward(n, kind, x, tg, loss, ws, b, None)

    def bwd(n=600, kind=0, x=a, tg=a, g=a, dx=a):
        return L.gs_skin_loss_backward(n, kind, x, tg, g, dx, None)

    for call in (fwd, bwd):
        assert call(n=-1) == -1
        for kind in (-1, 2, 3):  # the given-weights kind has no logits to differentiate
            assert call(kind=kind) == -1, kind
        for arg in ("x", "tg"):
            assert call(**{arg: None}) == -1 and call(**{arg: mis}) == -1, arg
    assert fwd(n=0, x=None, tg=None, loss=None, ws=None, b=0) == 0
    assert bwd(n=0, x=None, tg=None, g=None, dx=None) == 0
    assert fwd(loss=None) == -1 and fwd(loss=0x1002) == -1
    assert fwd(ws=None) == -1 and fwd(ws=mis) == -1
    assert fwd(b=nb - 1) == -5 and fwd(b=0) == -5  # a short workspace
    assert bwd(g=None) == -1 and bwd(g=0x1002) == -1 and bwd(dx=None) == -1 and bwd(dx=mis) == -1


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import skinning
    with pytest.raises(ValueError):
        skinning.skinning_mse_loss(torch.zeros(8, 26), torch.zeros(8, 24))
    with pytest.raises(ValueError):
        skinning.skinning_mse_loss(torch.zeros(8, 25), torch.zeros(7, 24))
    with pytest.raises(ValueError):
        skinning.skinning_mse_loss(torch.zeros(8, 24), torch.zeros(8, 25))
    with pytest.raises(RuntimeError, match="GPU"):
        skinning.skinning_mse_loss(torch.zeros(8, 25), torch.zeros(8, 24))
    v, f, w = ref.triangle()
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    with pytest.raises(ValueError):
        skinning.MeshSampler(v, np.array([[0, 1, 3]]), w, lo, hi, "cpu")   # a vertex that does not exist
    with pytest.raises(ValueError):
        skinning.MeshSampler(v, f, w[:2], lo, hi, "cpu")
    with pytest.raises(ValueError):
        skinning.MeshSampler(v, np.array([[1, 1, 2]]), w, lo, hi, "cpu")   # no area at all
    with pytest.raises(ValueError):
        skinning.MeshSampler(v, f, w, hi, lo, "cpu")
    s = skinning.MeshSampler(v, f, w, lo, hi, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        s.sample(4)

    class Field(object):
        distill = True

    with pytest.raises(NotImplementedError):
        skinning.skinning_loss(Field())


@pytest.mark.parametrize("mesh", ["triangle", "tetrahedron_with_degenerate_face", "sphere", "two_triangles"])
def test_mesh_sampler_cdf(mesh):
    """cdf: fp32, non-decreasing, the float64 running sum of the float64 areas rounded once -- also with a zero-area face,
    which repeats its predecessor's value so that the left-sided search never lands on it."""
    from gsplat_mi355 import skinning
    v, f, w = getattr(ref, mesh)()
    s = skinning.MeshSampler(torch.from_numpy(v), f, w, np.zeros(3), np.ones(3), "cpu")
    cdf = s.cdf.numpy()
    area = ref.face_areas(v, f)
    assert cdf.dtype == np.float32 and cdf.shape == (len(f),) and s.faces.dtype == torch.int32
    assert (np.diff(cdf) >= 0).all() and cdf[0] >= 0
    assert np.array_equal(cdf, np.cumsum(area).astype(np.float32))
    assert abs(float(cdf[-1]) - math.fsum(area)) <= float(np.spacing(cdf[-1]))  # the total, rounded once
    if mesh == "tetrahedron_with_degenerate_face":
        assert area[2] == 0.0 and cdf[2] == cdf[1] and cdf[1] > cdf[0] and cdf[3] > cdf[2]
    assert np.array_equal(s.aabb_inv_extent.numpy(), np.ones(3, np.float32))
    assert torch.equal(s.verts, torch.from_numpy(v)) and torch.equal(s.vertex_weights, torch.from_numpy(w))


@pytest.mark.parametrize("case", "abcd")
def test_restatement_matches_reference_fp64(fx, case):
    p = case + "/"
    loss, dx = ref.loss_and_grad(fx[p + "logits"], fx[p + "target"])
    want = float(fx[p + "loss_f64"])
    assert abs(loss - want) <= 1e-12 * abs(want), case
    want = fx[p + "dlogits_f64"]
    assert np.abs(dx - want).max() <= 1e-12 * np.abs(want).max(), case
    lo, hi = fx["aabb_min"].astype(np.float64), fx["aabb_max"].astype(np.float64)
    pn = 2.0 * (fx[p + "points"].astype(np.float64) - lo) / (hi - lo) - 1.0
    assert np.abs(pn - fx[p + "pnorm_f64"]).max() <= 1e-12


def test_restatement_barycentric_coordinates_agree_with_the_geometry():
    """(1 - a - b, a, b) are the barycentric coordinates of the sampled point: the sub-triangle areas say the same."""
    rng = np.random.default_rng(0)
    for mesh in (ref.triangle, ref.tetrahedron_with_degenerate_face, ref.sphere):
        v, f, w = mesh()
        cdf = np.cumsum(ref.face_areas(v, f)).astype(np.float32)
        r = ref.sample(v, f, cdf, w, np.zeros(3), np.ones(3), rng.random((4096, 3), dtype=np.float32))
        assert np.abs(r["bary"] - r["bary_geo"]).max() <= 1e-9
        assert r["bary"].min() >= -1e-7 and np.abs(r["bary"].sum(1) - 1).max() <= 1e-15
        assert np.abs(r["target"].sum(1) - 1).max() <= 1e-6  # blends of rows that sum to one


def test_fixture_cases_hold_what_they_claim(fx):
    assert [fx[c + "/logits"].shape for c in "abcd"] == [(96, 25), (64, 24), (48, 25), (1024, 25)]
    for c in "abcd":
        t = fx[c + "/target"]
        assert t.shape == (fx[c + "/logits"].shape[0], 24) and t.min() >= 0 and np.abs(t.sum(1) - 1).max() <= 1e-5
        assert fx[c + "/loss_f32"].shape == () and np.isfinite(fx[c + "/dlogits_f32"]).all()
    x = np.abs(fx["c/logits"])
    assert x.min() >= 20.0 and x.max() <= 1000.0
