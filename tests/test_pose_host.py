"""The fused SMPL pose correction's C ABI, Python entry points and fixture on the CPU (no GPU needed): the new symbols are
declared and exported, workspace sizes and argument validation (a bad kinematic tree included) work without a device,
the Python functions reject what they must before touching one, the fixture tests/golden/pose.npz holds the cases it
claims, and the float64 restatement tests/pose_ref.py reproduces the reference's own fp64 autograd results to 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import pose_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_pose_workspace_bytes", "gs_pose_forward", "gs_pose_backward")
CASES = "abcde"
MODEL = ("v_template", "shapedirs", "J_regressor", "parents")
INPUTS = ("betas", "root_orient", "pose_body", "pose_hand", "trans")
UPS = ("g_rots", "g_Jtrs", "g_bone", "g_loss")


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return pose_ref.load_fixture(os.path.join(ROOT, "tests", "golden", "pose.npz"))


def _shaped(fx, c):
    return fx[c + "/v_template"].astype(np.float64) + fx[c + "/shapedirs"].astype(np.float64) @ fx[c + "/betas"][0].astype(np.float64)


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    for name, value in (("GS_POSE_BONES", 24), ("GS_POSE_MAX_BETAS", 16), ("GS_POSE_STATE_FLOATS", 512)):
        assert getattr(lib, name) == value
    # two ints, the tree by value, ten pointers
    assert ctypes.sizeof(lib.GsPoseArgs) == 8 + 4 * 24 + 10 * ctypes.sizeof(ctypes.c_void_p)
    header = abi_header.text()
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    assert "gs_pose_forward" in capture_safe and "gs_pose_backward" in capture_safe


def test_workspace_sizes(lib):
    L = lib.load()
    ws = lambda v: lib.nbytes(L.gs_pose_workspace_bytes, v)
    # nine doubles per block of 256 vertices, at most 32 blocks (they stride over the vertices beyond that)
    for v, blocks in ((1, 1), (256, 1), (257, 2), (6890, 27), (8192, 32), (8193, 32), (1 << 24, 32)):
        assert ws(v) == blocks * 9 * 8, v
    out = ctypes.c_size_t(0)
    assert L.gs_pose_workspace_bytes(0, ctypes.byref(out)) == -1
    assert L.gs_pose_workspace_bytes(-3, ctypes.byref(out)) == -1
    assert L.gs_pose_workspace_bytes(10, None) == -1


def _args(lib, V=300, NB=10, parents=None, **ptrs):
    a = lib.GsPoseArgs()
    a.V, a.NB = V, NB
    a.parents[:] = [int(p) for p in (pose_ref.SMPL_PARENTS if parents is None else parents)]
    for name in ("v_template", "shapedirs", "J_template", "J_shapedirs", "betas", "root_orient", "pose_body", "pose_hand", "trans"):
        setattr(a, name, ptrs.get(name, 0x1000))
    a.rots_gt = ptrs.get("rots_gt", None)
    return a


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    p, odd = 0x1000, 0x1002  # never dereferenced: validation fails first (0x1002 is not fp32-aligned)
    nb = lib.nbytes(L.gs_pose_workspace_bytes, 300)

    def fwd(a, rots=p, Jtrs=p, bone=p, loss=p, state=p, ws=p, b=nb):
        return L.gs_pose_forward(ctypes.byref(a) if a is not None else None, rots, Jtrs, bone, loss, state, ws, b, None)

    def bwd(a, state=p, g=(p, p, p, p), d=(p, p, p, p, p)):
        return L.gs_pose_backward(ctypes.byref(a) if a is not None else None, state, *g, *d, None)

    for call in (fwd, bwd):
        assert call(None) == -1
        assert call(_args(lib, V=0)) == -1 and call(_args(lib, V=-5)) == -1
        assert call(_args(lib, NB=0)) == -1 and call(_args(lib, NB=17)) == -1
        # the kinematic tree: parents[i] >= i, a negative parent; entry 0 is ignored
        for i, v in ((1, 1), (5, 5), (7, 12), (23, 23), (3, -1), (23, 24)):
            bad = pose_ref.SMPL_PARENTS.copy()
            bad[i] = v
            assert call(_args(lib, parents=bad)) == -1, (i, v)
        for name in ("J_shapedirs", "root_orient", "pose_body", "pose_hand"):
            assert call(_args(lib, **{name: None})) == -1, name
            assert call(_args(lib, **{name: odd})) == -1, name
        assert call(_args(lib, rots_gt=odd)) == -1
        assert call(_args(lib), state=None) == -1 and call(_args(lib), state=odd) == -1
    for name in ("v_template", "shapedirs", "J_template", "betas", "trans"):
        assert fwd(_args(lib, **{name: None})) == -1, name
        assert fwd(_args(lib, **{name: odd})) == -1, name
    for name in ("rots", "Jtrs", "bone"):
        assert fwd(_args(lib), **{name: None}) == -1, name
        assert fwd(_args(lib), **{name: odd}) == -1, name
    assert fwd(_args(lib, rots_gt=p), loss=None) == -1          # a loss needs somewhere to go
    assert fwd(_args(lib), loss=odd) == -1
    assert fwd(_args(lib), ws=None) == -1 and fwd(_args(lib), ws=0x1004) == -1  # doubles: 8-byte alignment
    assert fwd(_args(lib), b=nb - 1) == -5 and fwd(_args(lib, V=257), b=nb - 1) == -5
    for k in range(4):
        g = [p] * 4
        g[k] = odd
        assert bwd(_args(lib), g=tuple(g)) == -1, k
    for k in range(5):
        d = [p] * 5
        d[k] = odd
        assert bwd(_args(lib), d=tuple(d)) == -1, k
    # nothing wanted: nothing to do (and nothing launched)
    assert bwd(_args(lib), d=(None,) * 5) == 0
    star = np.zeros(24, np.int32)
    star[0] = 77  # ignored
    assert bwd(_args(lib, parents=star), d=(None,) * 5) == 0
    assert bwd(_args(lib, parents=np.arange(-1, 23)), d=(None,) * 5) == 0


def test_python_argument_errors_without_a_device():
    from gsplat_mi355 import pose
    v, sd, Jr = torch.zeros(50, 3), torch.zeros(50, 3, 10), torch.zeros(24, 50)
    par = torch.from_numpy(pose_ref.SMPL_PARENTS.copy())
    with pytest.raises(RuntimeError, match="GPU"):
        pose.PoseModel(v, sd, Jr, par)
    with pytest.raises(RuntimeError, match="GPU"):
        pose.PoseModel(v[None], sd, Jr, par)
    with pytest.raises(ValueError):
        pose.PoseModel(torch.zeros(50, 4), sd, Jr, par)
    with pytest.raises(ValueError):
        pose.PoseModel(v, torch.zeros(50, 3, 17), Jr, par)
    with pytest.raises(ValueError):
        pose.PoseModel(v, torch.zeros(49, 3, 10), Jr, par)
    with pytest.raises(ValueError):
        pose.PoseModel(v, sd, torch.zeros(23, 50), par)
    with pytest.raises(ValueError):
        pose.PoseModel(v, sd, Jr, par[:23])
    bad = par.clone()
    bad[6] = 6
    with pytest.raises(ValueError, match="parents"):
        pose.PoseModel(v, sd, Jr, bad)

    model = object.__new__(pose.PoseModel)  # (a real one needs a device)
    model.NB = 10
    ok = dict(betas=torch.zeros(1, 10), root_orient=torch.zeros(1, 3), pose_body=torch.zeros(1, 63), pose_hand=torch.zeros(1, 6),
              trans=torch.zeros(1, 3))
    with pytest.raises(TypeError):
        pose.smpl_pose_forward(None, **ok)
    for name, shape in (("betas", (1, 6)), ("root_orient", (3,)), ("pose_body", (1, 69)), ("pose_hand", (2, 3)), ("trans", (1, 4))):
        with pytest.raises(ValueError, match=name):
            pose.smpl_pose_forward(model, **dict(ok, **{name: torch.zeros(*shape)}))
    with pytest.raises(ValueError, match="rots_gt"):
        pose.smpl_pose_forward(model, rots_gt=torch.zeros(1, 24, 3, 3), **ok)
    with pytest.raises(RuntimeError, match="GPU"):
        pose.smpl_pose_forward(model, **ok)

    class Module(object):
        cfg = dict(delay=10)
        frame_dict = {3: 0}

    class Camera(object):
        frame_id = 3

    cam = Camera()
    assert pose.pose_correct(Module(), cam, 9) == (cam, {})  # below `delay`: nothing is touched
    cam.frame_id = 4
    assert pose.pose_correct(Module(), cam, 10) == (cam, {})  # a frame without a row


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_fp64(fx, case):
    p = case + "/"
    got = pose_ref.forward_backward({k: fx[p + k] for k in MODEL}, *[fx[p + k] for k in INPUTS], fx[p + "rots_gt"],
                                    *[fx[p + k] for k in UPS])
    for name in pose_ref.OUTS + pose_ref.GRADS:
        want = fx["%s%s_f64" % (p, name)]
        err = np.abs(np.asarray(got[name]).reshape(want.shape) - want).max()
        assert err <= 1e-12 * max(np.abs(want).max(), 1e-300), (case, name, err)


def test_fixture_cases_hold_what_they_claim(fx):
    for c in CASES:
        V = fx[c + "/v_template"].shape[0]
        NB = fx[c + "/betas"].shape[1]
        assert fx[c + "/shapedirs"].shape == (V, 3, NB) and fx[c + "/J_regressor"].shape == (24, V)
        Jr = fx[c + "/J_regressor"]
        assert (Jr >= 0).all() and np.abs(Jr.astype(np.float64).sum(1) - 1.0).max() < 1e-6
        assert np.array_equal(fx[c + "/parents"], pose_ref.SMPL_PARENTS)
        for name, shape in (("root_orient", (1, 3)), ("pose_body", (1, 63)), ("pose_hand", (1, 6)), ("trans", (1, 3)),
                            ("rots_gt", (1, 24, 9)), ("rots_f64", (1, 24, 9)), ("Jtrs_f64", (1, 24, 3)),
                            ("bone_transforms_f64", (24, 4, 4)), ("dbetas_f64", (1, NB)), ("dpose_body_f64", (1, 63))):
            assert fx["%s/%s" % (c, name)].shape == shape, (c, name)
        assert np.array_equal(fx[c + "/rots_f64"][0, 0], np.eye(3).reshape(9))
        # (the reference inverts the star-pose transforms numerically: its rows 3 are (0, 0, 0, 1) up to rounding)
        assert np.abs(fx[c + "/bone_transforms_f64"][:, 3] - np.array([0, 0, 0, 1.0])).max() < 1e-15
    assert [fx[c + "/betas"].shape[1] for c in CASES] == [10, 10, 10, 6, 10]
    assert [fx[c + "/v_template"].shape[0] for c in CASES] == [300, 300, 300, 257, 333]
    assert fx["d/v_template"].shape[0] % 64 and fx["e/v_template"].shape[0] % 64
    # a: angles up to about 1 rad
    a = np.linalg.norm(np.concatenate([fx["a/root_orient"], fx["a/pose_body"], fx["a/pose_hand"]], 1).reshape(24, 3), axis=1)
    assert 0.5 < a.max() <= 1.0 + 1e-6 and a.min() > 0
    # b: the hands exactly zero, one body row exactly zero, one of magnitude 1e-6; their gradients are finite
    body = fx["b/pose_body"].reshape(21, 3)
    assert not fx["b/pose_hand"].any() and not body[4].any()
    assert abs(np.linalg.norm(body[9].astype(np.float64)) - 1e-6) < 1e-9
    assert (np.linalg.norm(np.delete(body, (4, 9), axis=0), axis=1) > 1e-2).all()
    assert np.isfinite(fx["b/dpose_hand_f64"]).all() and np.abs(fx["b/dpose_hand_f64"]).max() > 1e-3
    assert np.isfinite(fx["b/dpose_body_f64"]).all() and np.isfinite(fx["b/dpose_body_f32"]).all()
    assert np.array_equal(fx["b/rots_f64"][0, 22:], np.tile(np.eye(3).reshape(9), (2, 1)))
    # c: rows near pi (the first three along an axis: one coordinate within 1e-3 of +-pi) and one near 3 pi
    pose_c = np.concatenate([fx["c/root_orient"], fx["c/pose_body"], fx["c/pose_hand"]], 1).reshape(24, 3).astype(np.float64)
    near_pi, near_3pi = fx["c/near_pi"], fx["c/near_3pi"]
    assert len(near_pi) == 6 and len(near_3pi) == 1
    assert (np.abs(np.linalg.norm(pose_c[near_pi], axis=1) - np.pi) < 1e-3).all()
    assert (np.abs(np.linalg.norm(pose_c[near_3pi], axis=1) - 3 * np.pi) < 1e-3).all()
    for k, j in enumerate(near_pi[:3]):
        assert abs(abs(pose_c[j, k]) - np.pi) < 1e-3, j
    assert pose_c[near_pi[1], 1] < 0 < pose_c[near_pi[0], 0]
    # d / e: every shaped coordinate positive / negative
    assert _shaped(fx, "d").min() > 0 and _shaped(fx, "e").max() < 0
    assert _shaped(fx, "a").min() < 0 < _shaped(fx, "a").max()
    # the fp32 reference's own error: no tensor is beyond a quarter of the project's bar, so none gets a widened one
    for name in pose_ref.OUTS + pose_ref.GRADS:
        bar = float(fx["bar/" + name])
        worst = max(np.abs(fx["%s/%s_f32" % (c, name)].astype(np.float64) - fx["%s/%s_f64" % (c, name)]).max()
                    / np.abs(fx["%s/%s_f64" % (c, name)]).max() for c in CASES)
        assert abs(bar - worst) <= 1e-3 * worst + 1e-12, name
