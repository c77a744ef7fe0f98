"""The fused non-rigid deformer's C ABI, Python entry points and fixture on the CPU (no GPU needed): the new symbols are
declared, exported and bound, struct sizes and #defines agree, argument validation (a bad kinematic tree, a bad width,
unknown modes included) works with never-dereferenced pointers, the Python functions reject what they must before
touching a device, the float64 restatement tests/nonrigid_ref.py reproduces the reference's own fp64 autograd results
(tests/golden/nonrigid.npz) to 1e-12, and the fixture holds the cases it claims."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import nonrigid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_pose_encoder_grad_floats", "gs_pose_encoder_forward", "gs_pose_encoder_backward", "gs_nonrigid_workspace_bytes",
       "gs_nonrigid_apply_forward", "gs_nonrigid_apply_backward")
DEFINES = (("GS_POSE_ENC_JOINTS", 24), ("GS_POSE_ENC_MAX_DIM", 16), ("GS_POSE_ENC_STATE_FLOATS", 1392), ("GS_NONRIGID_MAX_D", 2048),
           ("GS_NR_SCALE_LOGIT", 0), ("GS_NR_SCALE_EXP", 1), ("GS_NR_SCALE_ZERO", 2), ("GS_NR_ROT_ADD", 0), ("GS_NR_ROT_MULT", 1))


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(os.path.join(ROOT, "tests", "golden", "nonrigid.npz"))


def test_symbols_declared_exported_and_bound(lib):
    header = abi_header.text()
    lib.load()
    for name, value in DEFINES:
        assert getattr(lib, name) == value
    # d and the tree by value (25 ints, padded to a pointer), rots, Jtrs, W0, b0 and four tables of 24 addresses
    assert ctypes.sizeof(lib.GsPoseEncArgs) == 104 + (4 + 4 * 24) * ctypes.sizeof(ctypes.c_void_p) < 1024
    # the state holds in_j and h_j at the largest width
    assert lib.GS_POSE_ENC_STATE_FLOATS == 2 * 24 * (13 + lib.GS_POSE_ENC_MAX_DIM)
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in ("gs_pose_encoder_forward", "gs_pose_encoder_backward", "gs_nonrigid_apply_forward", "gs_nonrigid_apply_backward"):
        assert name in capture_safe, name
    build_py = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "build.py")).read()
    assert build_py.count('"nonrigid.hip"') == 2  # SOURCES and STRICT


def test_sizes(lib):
    L = lib.load()
    for d in (1, 6, 16):
        n = lib.nbytes(L.gs_pose_encoder_grad_floats, d)
        assert n == sum(int(np.prod(s)) for s in ref.param_shapes(d))
        from gsplat_mi355 import nonrigid
        layout, total = nonrigid.grad_layout(d)
        assert total == n and [s for _, s in layout] == ref.param_shapes(d)
    out = ctypes.c_size_t(0)
    for d in (0, 17, -1):
        assert L.gs_pose_encoder_grad_floats(d, ctypes.byref(out)) == -1
    assert L.gs_pose_encoder_grad_floats(6, None) == -1
    ws = lambda n, D: lib.nbytes(L.gs_nonrigid_workspace_bytes, n, D)
    # three floats per block of min(256, floor(8192 / D) rounded down to a multiple of 4) rows
    for n, D, rows in ((1, 10, 256), (256, 10, 256), (257, 26, 256), (1000, 74, 108), (200000, 26, 256), (7, 2048, 4), (100, 33, 248)):
        assert ws(n, D) == 12 * ((n + rows - 1) // rows), (n, D)
    assert ws(0, 10) == 0
    for n, D in ((-1, 10), (5, 9), (5, 2049)):
        assert L.gs_nonrigid_workspace_bytes(n, D, ctypes.byref(out)) == -1
    assert L.gs_nonrigid_workspace_bytes(5, 10, None) == -1


def _enc_args(lib, d=6, parents=None, **ptrs):
    a = lib.GsPoseEncArgs()
    a.d = d
    a.parents[:] = [int(p) for p in (ref.SMPL_PARENTS if parents is None else parents)]
    for name in ("rots", "Jtrs", "W0", "b0"):
        setattr(a, name, ptrs.get(name, 0x1000))
    for name in ("W1", "b1", "W2", "b2"):
        for j in range(24):
            getattr(a, name)[j] = 0x1000
        if name in ptrs:
            j, v = ptrs[name]
            getattr(a, name)[j] = v
    return a


def test_encoder_argument_validation_without_a_device(lib):
    L = lib.load()
    p, odd = 0x1000, 0x1002  # never dereferenced: validation fails first

    def fwd(a, out=p, state=p):
        return L.gs_pose_encoder_forward(ctypes.byref(a) if a is not None else None, out, state, None)

    def bwd(a, state=p, g=p, d=(p, p, p)):
        return L.gs_pose_encoder_backward(ctypes.byref(a) if a is not None else None, state, g, *d, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        for d in (0, -1, 17, 1 << 20):
            assert call(_enc_args(lib, d=d)) == -1, d
        for i, v in ((1, 1), (5, 5), (7, 12), (23, 23), (3, -1), (23, 24)):
            bad = ref.SMPL_PARENTS.copy()
            bad[i] = v
            assert call(_enc_args(lib, parents=bad)) == -1, (i, v)
        assert call(_enc_args(lib, W0=None)) == -1 and call(_enc_args(lib, W0=odd)) == -1
        for name in ("W1", "W2"):
            for j in (0, 11, 23):
                assert call(_enc_args(lib, **{name: (j, None)})) == -1, (name, j)
                assert call(_enc_args(lib, **{name: (j, odd)})) == -1, (name, j)
        assert call(_enc_args(lib), state=None) == -1 and call(_enc_args(lib), state=odd) == -1
    for name in ("rots", "Jtrs", "b0"):
        assert fwd(_enc_args(lib, **{name: None})) == -1, name
        assert fwd(_enc_args(lib, **{name: odd})) == -1, name
    for name in ("b1", "b2"):
        assert fwd(_enc_args(lib, **{name: (17, None)})) == -1 and fwd(_enc_args(lib, **{name: (17, odd)})) == -1
    assert fwd(_enc_args(lib), out=None) == -1 and fwd(_enc_args(lib), out=odd) == -1
    assert bwd(_enc_args(lib), g=None) == -1 and bwd(_enc_args(lib), g=odd) == -1
    for k in range(3):
        d = [p] * 3
        d[k] = odd
        assert bwd(_enc_args(lib), d=tuple(d)) == -1, k
    # nothing wanted: nothing to do (and nothing launched); entry 0 of the tree is ignored
    assert bwd(_enc_args(lib), d=(None,) * 3) == 0
    star = np.zeros(24, np.int32)
    star[0] = 77
    assert bwd(_enc_args(lib, parents=star), d=(None,) * 3) == 0
    assert bwd(_enc_args(lib, parents=np.arange(-1, 23), d=16), d=(None,) * 3) == 0


def test_apply_argument_validation_without_a_device(lib):
    L = lib.load()
    p, odd4, odd16 = 0x1000, 0x1002, 0x1004

    def fwd(N=5, D=26, so=0, ro=0, deltas=p, xyz=p, scaling=p, rotation=p, xyz_o=p, scal_o=p, rot_o=p, feat=p, losses=p, ws=p,
            nbytes=12):
        return L.gs_nonrigid_apply_forward(N, D, so, ro, deltas, xyz, scaling, rotation, xyz_o, scal_o, rot_o, feat, losses, ws,
                                           nbytes, None)

    def bwd(N=5, D=26, so=0, ro=0, deltas=p, scaling=p, rotation=p, g=(p,) * 7, d=(p, p, p)):
        return L.gs_nonrigid_apply_backward(N, D, so, ro, deltas, scaling, rotation, *g, *d, None)

    for call in (fwd, bwd):
        assert call(N=-1) == -1
        assert call(D=9) == -1 and call(D=0) == -1 and call(D=2049) == -1
        assert call(so=3) == -1 and call(so=-1) == -1 and call(ro=2) == -1 and call(ro=-1) == -1
        assert call(deltas=None) == -1 and call(deltas=odd16) == -1
        assert call(rotation=odd16) == -1 and call(scaling=odd4) == -1
        assert call(N=0) == 0 and call(N=0, deltas=None) == 0  # no rows: nothing to do
    for name in ("xyz", "rotation", "xyz_o", "rot_o", "feat", "scaling", "scal_o"):
        assert fwd(**{name: None}) == -1, name
    for name in ("xyz", "xyz_o", "scal_o", "losses", "ws"):
        assert fwd(**{name: odd4}) == -1, name
    for name in ("rot_o", "feat"):
        assert fwd(**{name: odd16}) == -1, name
    assert fwd(ws=None) == -1 and fwd(nbytes=11) == -5 and fwd(N=257, nbytes=12) == -5
    assert bwd(so=1, scaling=None) == -1 and bwd(ro=1, rotation=None) == -1
    for k in range(7):
        g = [p] * 7
        g[k] = odd4 if k in (0, 1, 4, 5, 6) else odd16
        assert bwd(g=tuple(g)) == -1, k
    for k, bad in enumerate((odd16, odd4, odd16)):
        d = [p] * 3
        d[k] = bad
        assert bwd(d=tuple(d)) == -1, k
    assert bwd(d=(None,) * 3) == 0  # nothing wanted
    assert bwd(so=2, scaling=None, d=(None,) * 3) == 0


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import nonrigid
    rots, Jtrs = torch.zeros(1, 24, 9), torch.zeros(1, 24, 3)
    with pytest.raises(NotImplementedError, match="rel_joints"):
        nonrigid.pose_encode(ref.PoseEncoder(rel_joints=True), rots, Jtrs)
    with pytest.raises(NotImplementedError, match="batch"):
        nonrigid.pose_encode(ref.PoseEncoder(), torch.zeros(2, 24, 9), torch.zeros(2, 24, 3))
    with pytest.raises(NotImplementedError, match="dim_per_joint"):
        nonrigid.pose_encode(ref.PoseEncoder(dim_per_joint=17), rots, Jtrs)
    with pytest.raises(ValueError):
        nonrigid.pose_encode(ref.PoseEncoder(), torch.zeros(1, 24, 3, 4), Jtrs)
    bad = ref.SMPL_PARENTS.copy()
    bad[6] = 6
    with pytest.raises(ValueError, match="parents"):
        nonrigid.pose_encode(ref.PoseEncoder(parents=bad), rots, Jtrs)
    with pytest.raises(RuntimeError, match="GPU"):
        nonrigid.pose_encode(ref.PoseEncoder(), rots, Jtrs)
    with pytest.raises(RuntimeError, match="GPU"):
        nonrigid.hierarchical_pose_encoder_forward(ref.PoseEncoder(out_dim=8), rots, Jtrs)

    ok = dict(deltas=torch.zeros(5, 26), xyz=torch.zeros(5, 3), scaling=torch.zeros(5, 3), rotation=torch.zeros(5, 4))
    for name, shape in (("deltas", (5, 9)), ("deltas", (5,)), ("deltas", (5, 2049)), ("xyz", (4, 3)), ("scaling", (5, 4)),
                        ("rotation", (5, 3))):
        with pytest.raises(ValueError):
            nonrigid.nonrigid_apply(**dict(ok, **{name: torch.zeros(*shape)}))
    with pytest.raises(ValueError, match="scale_offset"):
        nonrigid.nonrigid_apply(scale_offset="log", **ok)
    with pytest.raises(ValueError, match="rot_offset"):
        nonrigid.nonrigid_apply(rot_offset="times", **ok)
    with pytest.raises(RuntimeError, match="GPU"):
        nonrigid.nonrigid_apply(**ok)

    class Gaussians(object):
        get_xyz = torch.zeros(7, 3)

        def clone(self):
            return Gaussians()

    module = type("Module", (), dict(delay=10, feature_dim=4))()
    gs = Gaussians()
    out, losses = nonrigid.nonrigid_forward(module, gs, 9, None)  # below `delay`: a clone, zero features, no losses
    assert out is not gs and losses == {} and tuple(out.non_rigid_feature.shape) == (7, 4) and not out.non_rigid_feature.any()
    module.feature_dim = 0
    out, losses = nonrigid.nonrigid_forward(module, gs, 0, None)
    assert losses == {} and not hasattr(out, "non_rigid_feature")


def _err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got).reshape(want.shape) - want).max()) / max(float(np.abs(want).max()), 1e-300)


@pytest.mark.parametrize("case", ref.ENC_CASES)
def test_encoder_restatement_matches_reference_fp64(fx, case):
    p = case + "/"
    got = ref.encoder_forward_backward(fx[p + "params"], int(fx[p + "d"]), fx[p + "rots"], fx[p + "Jtrs"], ref.SMPL_PARENTS, fx[p + "g"])
    for name in ("out", "drots", "dJtrs", "dparams"):
        assert _err(got[name], fx["%s%s_f64" % (p, name)]) <= 1e-12, (case, name)
    assert _err(got["pre"], fx[p + "pre_f64"]) <= 1e-12


@pytest.mark.parametrize("case", ref.APPLY_CASES)
def test_apply_restatement_matches_reference_fp64(fx, case):
    p = case + "/"
    so, ro, F = case.split("_")
    ups = {k: fx.get(p + k) for k in ref.APPLY_UPS}
    got = ref.apply_forward_backward(fx[p + "deltas"], fx[p + "xyz"], fx[p + "scaling"], fx[p + "rotation"], so, ro, **ups)
    for name in ref.APPLY_OUTS + ref.APPLY_GRADS:
        want = fx["%s%s_f64" % (p, name)]
        if not np.abs(want).max():
            assert not np.abs(got[name]).max(), (case, name)
        else:
            assert _err(got[name], want) <= 1e-12, (case, name)


def test_fixture_cases_hold_what_they_claim(fx):
    assert [int(fx[c + "/d"]) for c in ref.ENC_CASES] == [1, 6, 16, 6, 6]
    for c in ref.ENC_CASES:
        d = int(fx[c + "/d"])
        n = sum(int(np.prod(s)) for s in ref.param_shapes(d))
        assert fx[c + "/params"].shape == (n,) == fx[c + "/dparams_f64"].shape
        assert fx[c + "/rots"].shape == (1, 24, 9) and fx[c + "/Jtrs"].shape == (1, 24, 3) and fx[c + "/g"].shape == (1, 24 * d)
        pre = fx[c + "/pre_f64"]
        assert pre.shape == (24, 13 + d)
        dead = (5, 16) if c == "k" else ()
        assert np.abs(np.delete(pre, dead, axis=0)).min() > 1e-4  # fp32 and fp64 agree on every ReLU decision
        for name in ("out", "drots", "dJtrs", "dparams"):
            assert np.isfinite(fx["%s/%s_f32" % (c, name)]).all() and np.isfinite(fx["%s/%s_f64" % (c, name)]).all()
    # z: two zero-length bones, finite gradients, the bone-length inputs' weights still take none from them
    J = fx["z/Jtrs"][0]
    assert np.array_equal(J[7], J[4]) and not J[0].any()
    bones = np.abs(J[1:] - J[ref.SMPL_PARENTS[1:]]).sum(1)
    assert bones[6] == 0 and np.delete(bones, 6).min() > 0
    dW1 = ref.unpack(fx["z/dparams_f64"], 6)
    for j in (0, 7):
        assert not dW1[2 + 4 * j][:, 12].any() and dW1[2 + 4 * j][:, :12].any()
    # k: every hidden unit of joints 5 and 16 dead: their first layers take no gradient, their second layers only a bias one
    assert fx["k/pre_f64"][[5, 16]].max() < -1.0
    dk, pk = ref.unpack(fx["k/dparams_f64"], 6), ref.unpack(fx["k/params"], 6)
    for j in (5, 16):
        assert (pk[2 + 4 * j + 1] == -10).all()
        assert not dk[2 + 4 * j].any() and not dk[2 + 4 * j + 1].any() and not dk[2 + 4 * j + 2].any() and dk[2 + 4 * j + 3].any()
    assert dk[2 + 4 * 4].any()

    assert len(ref.APPLY_CASES) == 12
    for c in ref.APPLY_CASES:
        so, ro, F = c.split("_")
        F = int(F[1:])
        deltas = fx[c + "/deltas"]
        n = deltas.shape[0]
        assert deltas.shape == (n, 10 + F) and n <= 96 and ((c + "/g_feat") in fx) == (F > 0)
        assert not deltas[3, :10].any()  # a zero offset row: the norm's gradient there is zero, and finite
        dd = fx[c + "/ddeltas_f64"]
        assert np.isfinite(dd).all() and np.isfinite(fx[c + "/ddeltas_f32"]).all()
        assert np.array_equal(dd[3, :3], fx[c + "/g_xyz"][3].astype(np.float64))
        if ro == "mult":
            assert not dd[:, 6].any() and dd[:, 7:10].any()
        if so == "zero":
            assert not dd[:, 3:6].any() and not fx[c + "/nr_f64"][1]
            assert np.array_equal(fx[c + "/scal_o_f32"], fx[c + "/scaling"])
        if so == "exp":  # the clamp rows: log(1e-6) and exactly zero gradients; the others far from the threshold
            e = np.exp(fx[c + "/scaling"].astype(np.float64))
            arg = e + deltas[:, 3:6].astype(np.float64)
            clamp = arg <= 0
            assert ((arg >= 0.1 * e) | clamp).all() and clamp.sum() >= 9 and (~clamp).sum() >= 60
            assert np.allclose(fx[c + "/scal_o_f64"][clamp], np.log(1e-6), rtol=0, atol=1e-12)
            assert not fx[c + "/dscaling_f64"][clamp].any() and fx[c + "/dscaling_f64"][~clamp].all()
            w = fx[c + "/g_nr"][1].astype(np.float64) / n
            assert np.allclose(dd[:, 3:6][clamp], w * np.sign(deltas[:, 3:6][clamp]), rtol=1e-12, atol=0)
        if F:
            assert np.array_equal(dd[:, 10:], fx[c + "/g_feat"].astype(np.float64))
