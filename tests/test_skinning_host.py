"""Linear blend skinning's C ABI, Python entry points and fixture on the CPU (no GPU needed): the new symbols are declared
and exported, workspace sizes and argument validation work without a device, the Python functions reject what they
must before touching one, and the float64 restatement tests/skinning_ref.py reproduces the reference's own fp64
autograd results (tests/golden/skinning.npz) to 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import skinning_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_skin_weights_forward", "gs_skin_weights_backward", "gs_skinning_workspace_bytes", "gs_skinning_forward",
       "gs_skinning_backward")
OUTS = ("xbar", "Rbar", "T", "dw", "dtfs", "dxyz", "drot")


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return skinning_ref.load_fixture(os.path.join(ROOT, "tests", "golden", "skinning.npz"))


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert (lib.GS_SKIN_BONES, lib.GS_SKIN_HIERARCHICAL, lib.GS_SKIN_SOFTMAX, lib.GS_SKIN_WEIGHTS) == (24, 0, 1, 2)


def test_workspace_sizes(lib):
    L = lib.load()
    ws = lambda n: lib.nbytes(L.gs_skinning_workspace_bytes, n)
    # one 24 x 12 partial of doubles per block of 256 Gaussians
    for n, blocks in ((0, 0), (1, 1), (256, 1), (257, 2), (200000, 782), (1100000, 4297)):
        assert ws(n) == blocks * 24 * 12 * 8, n
    out = ctypes.c_size_t(0)
    assert L.gs_skinning_workspace_bytes(-1, ctypes.byref(out)) == -1
    assert L.gs_skinning_workspace_bytes(10, None) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    a, mis = 0x1000, 0x1004  # never dereferenced: validation fails first (0x1004: 4-byte but not 16-byte aligned)
    nb = lib.nbytes(L.gs_skinning_workspace_bytes, 10)

    def fwd(n=10, kind=0, w=a, tfs=a, xyz=a, rot=a, xo=a, ro=a, T=a):
        return L.gs_skinning_forward(n, kind, w, tfs, xyz, rot, xo, ro, T, None)

    def bwd(n=10, kind=0, w=a, tfs=a, xyz=a, rot=a, gx=a, gr=a, dw=a, dtfs=a, dx=a, dr=a, ws=a, b=nb):
        return L.gs_skinning_backward(n, kind, w, tfs, xyz, rot, gx, gr, dw, dtfs, dx, dr, ws, b, None)

    for call in (fwd, bwd):
        assert call(n=-1) == -1
        assert call(kind=3) == -1 and call(kind=-1) == -1
        assert call(n=0, w=None, tfs=None, xyz=None, rot=None) == 0  # N = 0 touches nothing
        for arg in ("w", "tfs", "xyz", "rot"):
            assert call(**{arg: None}) == -1, arg
        for arg in ("w", "tfs", "rot"):  # 16-byte loads
            assert call(**{arg: mis}) == -1, arg
    for arg in ("xo", "ro", "T"):
        assert fwd(**{arg: None}) == -1, arg
        assert fwd(**{arg: mis}) == -1, arg
    assert bwd(xyz=0x1002) == -1 and bwd(gx=0x1002) == -1 and bwd(dtfs=0x1002) == -1
    assert bwd(dw=mis) == -1 and bwd(dr=mis) == -1
    assert bwd(ws=None) == -1                                   # dtfs wanted: the workspace is required
    assert bwd(b=nb - 1) == -5                                  # too small
    assert bwd(ws=mis) == -1
    for kind in (0, 1):
        assert L.gs_skin_weights_forward(-1, kind, a, a, None) == -1
        assert L.gs_skin_weights_forward(0, kind, None, None, None) == 0
        assert L.gs_skin_weights_forward(10, kind, None, a, None) == -1
        assert L.gs_skin_weights_forward(10, kind, mis, a, None) == -1
        assert L.gs_skin_weights_forward(10, kind, a, mis, None) == -1
        assert L.gs_skin_weights_backward(10, kind, a, None, a, None) == -1
        assert L.gs_skin_weights_backward(10, kind, a, a, mis, None) == -1
    assert L.gs_skin_weights_forward(10, 2, a, a, None) == -1   # the given-weights kind has no activation
    assert L.gs_skin_weights_backward(10, 7, a, a, a, None) == -1


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import skinning
    x = torch.zeros(8, 25)
    with pytest.raises(RuntimeError, match="GPU"):
        skinning.hierarchical_softmax(x)
    with pytest.raises(ValueError):
        skinning.hierarchical_softmax(torch.zeros(8, 24))
    with pytest.raises(ValueError):
        skinning.skinning_softmax(torch.zeros(8, 23))
    with pytest.raises(RuntimeError, match="GPU"):
        skinning.skinning_softmax(torch.zeros(8, 24))
    tfs, xyz, rot = torch.zeros(24, 4, 4), torch.zeros(8, 3), torch.zeros(8, 4)
    with pytest.raises(ValueError):
        skinning.linear_blend_skinning(torch.zeros(8, 26), tfs, xyz, rot)
    with pytest.raises(ValueError):
        skinning.linear_blend_skinning(torch.zeros(8, 25), tfs, xyz, rot, weights=True)
    with pytest.raises(ValueError):
        skinning.linear_blend_skinning(x, torch.zeros(23, 4, 4), xyz, rot)
    with pytest.raises(ValueError):
        skinning.linear_blend_skinning(x, tfs, torch.zeros(7, 3), rot)
    with pytest.raises(RuntimeError, match="GPU"):
        skinning.linear_blend_skinning(x, tfs, xyz, rot)

    class Field(object):
        distill = True

    with pytest.raises(NotImplementedError):
        skinning.skinning_field_forward(Field(), None, 0, None)


@pytest.mark.parametrize("case", "abcde")
def test_restatement_matches_reference_fp64(fx, case):
    p = case + "/"
    got = skinning_ref.forward_backward(fx[p + "w"], fx[p + "tfs"], fx[p + "xyz"], fx[p + "rot"], str(fx[p + "kind"]),
                                        fx[p + "g"], fx[p + "G"])
    for name in OUTS:
        want = fx["%s%s_f64" % (p, name)]
        assert np.abs(got[name] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (case, name)


def test_restatement_matches_reference_fp64_weights_alone(fx):
    W, dx = skinning_ref.weights_forward_backward(fx["f/x"], "hierarchical", fx["f/gW"])
    for got, key in ((W, "f/W_f64"), (dx, "f/dx_f64")):
        want = fx[key]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), key


def test_fixture_cases_hold_what_they_claim(fx):
    assert [str(fx[c + "/kind"]) for c in "abcde"] == ["hierarchical", "softmax", "weights", "hierarchical", "hierarchical"]
    assert fx["a/w"].shape[1] == 25 and fx["b/w"].shape[1] == 24 and fx["f/x"].shape == (1024, 25)
    n = np.linalg.norm(fx["a/rot"], axis=1)
    assert n.min() >= 0.5 - 1e-6 and n.max() <= 2.0 + 1e-6 and n.std() > 0.1
    w = fx["c/w"]
    assert ((w == 1.0).sum(1) == 1).sum() >= 8 and ((w > 0).sum(1) > 1).sum() >= 8   # one-hot and blended rows
    x = np.abs(fx["d/w"])
    assert x.min() >= 20.0 and x.max() <= 1000.0
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-fx["d/w"].astype(np.float32)))
    assert (np.float32(1.0) - s.astype(np.float32) == 0).any()                        # 1 - s rounds to 0 in fp32
    assert np.abs(fx["e/tfs"][:, 3] - np.array([0, 0, 0, 1], np.float32)).max() > 0.1  # a general row 3
    assert np.abs(fx["a/tfs"][:, 3] - np.array([0, 0, 0, 1], np.float32)).max() == 0
    for c in "abcde":  # rows 3 of the bone-transform gradient are zero (T_fwd's row 3 feeds nothing differentiable)
        assert not fx[c + "/dtfs_f64"][:, 3].any()
