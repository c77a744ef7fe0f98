"""The fused ColorMLP input's C ABI, Python entry points and fixture on the CPU (no GPU needed): the new symbols are
declared, exported and bound, the struct mirrors the header's field for field, argument validation works with
never-dereferenced pointers, the Python functions reject what they must before touching a device, the float64
restatement tests/texture_ref.py reproduces the reference's own fp64 autograd results (tests/golden/texture.npz) to
1e-12, and the fixture holds the cases it claims."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import texture_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_texture_workspace_bytes", "gs_texture_input_forward", "gs_texture_input_backward")
DEFINES = (("GS_TEXTURE_MAX_D", 512), ("GS_TEXTURE_MAX_BEFORE", 6), ("GS_TEXTURE_MAX_AFTER", 2))


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "texture.npz"))


def test_symbols_declared_exported_and_bound(lib):
    header = abi_header.text()
    lib.load()
    for name, value in DEFINES:
        assert getattr(lib, name) == value
    # the largest shipped config (texture/mlp.yaml): 128 features, 15 bases, 64 non-rigid features, 64 latent values
    assert lib.GS_TEXTURE_MAX_D >= 128 + 15 + 64 + 64
    # 17 ints and the 9 floats of the noise matrix (104 bytes), then 12 addresses
    assert ctypes.sizeof(lib.GsTextureArgs) == 104 + 12 * ctypes.sizeof(ctypes.c_void_p)
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in NEW[1:]:
        assert name in capture_safe, name
    build_py = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "build.py")).read()
    assert build_py.count('"texture.hip"') == 2  # SOURCES and STRICT


def test_workspace_sizes(lib):
    from gsplat_mi355 import texture
    L = lib.load()
    ws = lambda n, D, lt: lib.nbytes(L.gs_texture_workspace_bytes, n, D, lt)
    # one float per latent column and block of min(256, floor(8192 / D) rounded down to a multiple of 4) rows
    for D, rows in ((1, 256), (32, 256), (33, 248), (79, 100), (88, 92), (223, 36), (256, 32), (271, 28), (512, 16)):
        assert texture.rows_per_block(D) == rows
        for n in (1, rows, rows + 1, 200000):
            assert ws(n, D, min(16, D)) == 4 * min(16, D) * ((n + rows - 1) // rows), (n, D)
    assert ws(0, 79, 16) == 0 and ws(1000, 79, 0) == 0
    out = ctypes.c_size_t(0)
    for n, D, lt in ((-1, 79, 16), (5, 0, 0), (5, 513, 16), (5, 79, -1), (5, 16, 17)):
        assert L.gs_texture_workspace_bytes(n, D, lt, ctypes.byref(out)) == -1, (n, D, lt)
    assert L.gs_texture_workspace_bytes(5, 79, 16, None) == -1


P, ODD4, ODD16 = 0x1000, 0x1002, 0x1004  # never dereferenced: validation fails first


def _args(lib, N=5, deg=3, before=(1, 31), after=(16,), lt=16, D=None, **over):
    a = lib.GsTextureArgs()
    a.N, a.sh_degree, a.latent_dim, a.n_before, a.n_after = N, deg, lt, len(before), len(after)
    for k, w in enumerate(before[:6]):
        a.before_w[k], a.before[k] = w, P
    for k, w in enumerate(after[:2]):
        a.after_w[k], a.after[k] = w, P
    a.D = sum(before) + sum(after) + (deg + 1) ** 2 - 1 + lt if D is None else D
    a.xyz = a.campos = a.fwd_transform = a.latent = P
    a.rot_stride, a.rot_row = 16, 4
    for k, v in over.items():
        if k in ("before_ptr", "after_ptr"):
            getattr(a, k[:-4])[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_argument_validation_without_a_device(lib):
    L = lib.load()

    def fwd(a, inp=P):
        return L.gs_texture_input_forward(ctypes.byref(a) if a is not None else None, inp, None)

    def bwd(a, g=P, db=(P,) * 6, da=(P,) * 2, dxyz=P, dlat=P, ws=P, nbytes=1 << 20):
        db = (ctypes.c_void_p * 6)(*db) if db is not None else None
        da = (ctypes.c_void_p * 2)(*da) if da is not None else None
        return L.gs_texture_input_backward(ctypes.byref(a) if a is not None else None, g, db, da, dxyz, dlat, ws, nbytes, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        assert call(_args(lib, N=-1)) == -1
        for deg in (-1, 5):
            assert call(_args(lib, deg=deg)) == -1, deg
        assert call(_args(lib, n_before=7)) == -1 and call(_args(lib, n_before=-1)) == -1
        assert call(_args(lib, n_after=3)) == -1 and call(_args(lib, n_after=-1)) == -1
        assert call(_args(lib, D=78)) == -1 and call(_args(lib, D=80)) == -1       # not the sum of the widths
        assert call(_args(lib, before=(1, 0))) == -1 and call(_args(lib, after=(-1,))) == -1
        assert call(_args(lib, lt=-1)) == -1
        assert call(_args(lib, before=(400,), after=(82,), lt=16, deg=3)) == -1   # D = 513: one over the cap
        assert call(_args(lib, N=0)) == 0 and call(_args(lib, N=0, xyz=None)) == 0  # no rows: nothing to do
    # D at the cap passes the shape checks: a later one (the workspace's size) answers
    assert bwd(_args(lib, before=(400,), after=(81,), lt=16, deg=3), nbytes=0) == -5
    assert fwd(_args(lib), inp=None) == -1 and fwd(_args(lib), inp=ODD16) == -1
    for k in range(2):
        assert fwd(_args(lib, before_ptr=(k, None))) == -1 and fwd(_args(lib, before_ptr=(k, ODD16))) == -1
    assert fwd(_args(lib, after_ptr=(0, None))) == -1 and fwd(_args(lib, after_ptr=(0, ODD16))) == -1
    for name in ("xyz", "campos", "latent"):
        assert fwd(_args(lib, **{name: None})) == -1 and fwd(_args(lib, **{name: ODD4})) == -1, name
    assert fwd(_args(lib, fwd_transform=ODD4)) == -1
    assert fwd(_args(lib, rot_row=2)) == -1 and fwd(_args(lib, rot_stride=10)) == -1
    assert bwd(_args(lib), g=None) == -1 and bwd(_args(lib), g=ODD16) == -1
    for k in range(2):
        db = [P] * 6
        db[k] = ODD16
        assert bwd(_args(lib), db=tuple(db)) == -1
    assert bwd(_args(lib), da=(ODD16, P)) == -1
    assert bwd(_args(lib), dxyz=ODD4) == -1 and bwd(_args(lib), dlat=ODD4) == -1
    assert bwd(_args(lib, xyz=None)) == -1 and bwd(_args(lib, campos=None)) == -1 and bwd(_args(lib, rot_row=2)) == -1
    assert bwd(_args(lib, deg=0)) == -1                    # no direction: no dL_dxyz
    assert bwd(_args(lib, lt=0)) == -1                     # no latent: no dL_dlatent
    assert bwd(_args(lib), ws=None) == -1 and bwd(_args(lib), ws=ODD4) == -1
    assert bwd(_args(lib), nbytes=63) == -5 and bwd(_args(lib, N=101), nbytes=64) == -5  # 16 floats per block of 100 rows
    # nothing wanted: nothing to do (and nothing launched), whatever the direction's pointers are
    nothing = dict(db=None, da=None, dxyz=None, dlat=None, ws=None, nbytes=0)
    assert bwd(_args(lib, xyz=None, campos=None), **nothing) == 0
    assert bwd(_args(lib), db=(None,) * 6, da=(None,) * 2, dxyz=None, dlat=None) == 0


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import texture
    n = 5
    ok = dict(before=[torch.zeros(n, 1, 1), torch.zeros(n, 31, 1)], xyz=torch.zeros(n, 3), camera_center=torch.zeros(3),
              sh_degree=3, fwd_transform=torch.zeros(n, 4, 4), after=[torch.zeros(n, 16)], latent=torch.zeros(1, 16))
    call = lambda **over: texture.color_mlp_input(**dict(ok, **over))
    for bad in (dict(xyz=torch.zeros(n, 4)), dict(xyz=torch.zeros(n)), dict(sh_degree=5), dict(sh_degree=-1),
                dict(before=[torch.zeros(n + 1, 32)]), dict(before=[torch.zeros(n, 1)] * 7), dict(after=[torch.zeros(n, 1)] * 3),
                dict(after=[torch.zeros(n, 0)]), dict(camera_center=torch.zeros(4)), dict(latent=torch.zeros(2, 16)),
                dict(latent=torch.zeros(1, 1, 16)), dict(fwd_transform=torch.zeros(n, 3, 4)), dict(fwd_transform=torch.zeros(n + 1, 4, 4)),
                dict(view_noise=torch.zeros(4, 4)), dict(before=[torch.zeros(n, 400)], after=[torch.zeros(n, 82)]),
                dict(before=[], after=[], latent=None, sh_degree=0)):
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (dict(xyz=torch.zeros(n, 3, dtype=torch.float64)), dict(before=[torch.zeros(n, 32, dtype=torch.float16)]),
                dict(latent=torch.zeros(16, dtype=torch.float64)), dict(camera_center=torch.zeros(3, dtype=torch.float64)),
                dict(fwd_transform=torch.zeros(n, 4, 4, dtype=torch.float64)), dict(xyz=[[0.0] * 3] * n)):
        with pytest.raises(TypeError):
            call(**bad)
    with pytest.raises(RuntimeError, match="GPU"):
        call()
    assert texture.MAX_D == 512 and texture.rows_per_block(79) == 100

    class Gaussians(object):
        get_xyz = torch.zeros(n, 3)
        _features_dc, _features_rest = torch.zeros(n, 1, 1), torch.zeros(n, 31, 3)

    module = type("Module", (), dict(use_xyz=False, use_cov=False, use_normal=False, sh_degree=0, cano_view_dir=False,
                                     non_rigid_dim=0, latent_dim=0, training=False))()
    with pytest.raises(ValueError, match="_features_rest"):
        texture.texture_forward(module, Gaussians(), None)
    Gaussians._features_rest = torch.zeros(n, 31, 1)
    camera = type("Camera", (), dict(camera_center=torch.zeros(3), frame_id=0))()
    with pytest.raises(RuntimeError, match="GPU"):
        texture.texture_forward(module, Gaussians(), camera)


def _err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got).reshape(want.shape) - want).max()) / max(float(np.abs(want).max()), 1e-300)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_restatement_matches_reference_fp64(fx, case):
    got = ref.case_results(fx, case)
    for name in ("inp",) + ref.GRADS:
        want = fx["%s/%s_f64" % (case, name)]
        if not np.abs(want).max():
            assert not np.abs(got[name]).max(), (case, name)
        else:
            assert _err(got[name], want) <= 1e-12, (case, name, _err(got[name], want))


def test_fixture_cases_hold_what_they_claim(fx):
    assert len(ref.CASES) == 7
    assert sorted((c["sh_degree"], c["cano"], c["use_xyz"], c["latent_dim"], c["known_frame"]) for c in ref.CASES.values()) == \
        sorted([(1, 1, 0, 16, 1), (3, 1, 0, 16, 1), (4, 1, 0, 16, 1), (3, 0, 0, 16, 1), (3, 1, 1, 16, 1), (0, 1, 0, 0, 1), (3, 1, 0, 16, 0)])
    for case, c in ref.CASES.items():
        p = case + "/"
        n = fx[p + "xyz"].shape[0]
        D = 32 + 3 * c["use_xyz"] + ref.n_sh(c["sh_degree"]) + 16 + c["latent_dim"]
        assert n == 40 and fx[p + "features_dc"].shape == (n, 1, 1) and fx[p + "features_rest"].shape == (n, 31, 1)
        assert fx[p + "non_rigid_feature"].shape == (n, 16) and fx[p + "T_fwd"].shape == (n, 4, 4) and fx[p + "noise"].shape == (3, 3)
        assert fx[p + "g"].shape == (n, D) == fx[p + "inp_f32"].shape == fx[p + "inp_f64"].shape
        assert np.abs(fx[p + "xyz"]).max() <= 1 and abs(np.linalg.norm(fx[p + "campos"]) - c["dist"]) < 1e-6
        R = fx[p + "T_fwd"][:, :3, :3].astype(np.float64)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.abs(fx[p + "T_fwd"][:, :3, 3]).max() > 0.1
        M = fx[p + "noise"].astype(np.float64)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-6 and np.abs(M - np.eye(3)).max() > 0.05
        for name in ("inp",) + ref.GRADS:
            f32, f64 = fx["%s%s_f32" % (p, name)], fx["%s%s_f64" % (p, name)]
            assert f32.dtype == np.float32 and f64.dtype == np.float64 and np.isfinite(f64).all()
            # what the generator asserted: the reference's fp32 within a tenth of the GPU tests' bar of its fp64
            assert np.abs(f32 - f64).max() <= 1e-6 * max(np.abs(f64).max(), 1e-300), (case, name)
        inp, g = fx[p + "inp_f64"], fx[p + "g"].astype(np.float64)
        assert np.array_equal(inp[:, :1], fx[p + "features_dc"].reshape(n, 1)) and np.array_equal(inp[:, 1:32], fx[p + "features_rest"].reshape(n, 31))
        assert np.array_equal(fx[p + "d_features_rest_f64"].reshape(n, 31), g[:, 1:32])
        row, dW = int(fx[p + "latent_row"]), fx[p + "d_latent_weight_f64"]
        assert row == (2 if c["known_frame"] else 4)
        if c["latent_dim"]:
            assert np.array_equal(inp[:, -16:], np.broadcast_to(fx[p + "latent_weight"][row], (n, 16)))
            assert dW[row].all() and not np.delete(dW, row, axis=0).any()
        else:
            assert not dW.any() and D == 48
        sh = inp[:, 32 + 3 * c["use_xyz"]:32 + 3 * c["use_xyz"] + ref.n_sh(c["sh_degree"])]
        if c["sh_degree"]:
            assert fx[p + "d_xyz_f64"].all()
            assert np.allclose((sh[:, :3] ** 2).sum(1), ref.C1 ** 2, rtol=1e-9)  # a unit direction
        else:
            assert not fx[p + "d_xyz_f64"].any()
    # the rotation and the noise matter where they are on, and only there
    kw, _ = ref.case_call(fx, "deg3")
    assert _err(ref.compose(**dict(kw, noise=None)), fx["deg3/inp_f64"]) > 1e-3
    assert _err(ref.compose(**dict(kw, fwd_transform=None)), fx["deg3/inp_f64"]) > 1e-3
    kw, _ = ref.case_call(fx, "deg3_world")
    assert kw["fwd_transform"] is None and kw["noise"] is None
    kw, _ = ref.case_call(fx, "deg1")
    assert kw["noise"] is None  # eval mode
