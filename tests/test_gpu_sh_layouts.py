"""The kernels that read spherical-harmonic coefficients, off the diagonal the rest of the suite stays on.  Each takes the
active degree `deg` and the stored coefficient count `M` separately ((deg+1)^2 <= M <= 16) and branches on M == 16, on
3 M being a multiple of four and on the block of coefficients starting on a 16-byte boundary; helpers.cloud_and_camera
only ever builds M == (deg+1)^2 in fresh storage.  The reference model stores 16 coefficients from the first iteration
and raises the degree every 1000 (scene/gaussian_model.py:159-163), so deg < 3 with M = 16 is three quarters of its
schedule.  Here: the rasterizer (preprocess.hip, gaussian_bwd.hip, the SH tiles of gs_math.h) at every such branch
against the oracle at the bars of test_random_small_scenes_against_oracle, the same scene in three layouts bit for bit,
and the two pre-pass kernels (prepass.hip) at every coefficient-count branch and block edge."""
import functools

import numpy as np
import pytest
import torch

import helpers
from test_gpu_parity import SMALL_TOL, _bulk_close, _conditioned_oracle, _inputs, _settings

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# ---- the rasterizer

P, W, H = 600, 64, 48  # two full workgroups of 256 and a tail of 88
BG = (0.2, 0.4, 0.1)
CULLED = torch.arange(P) % 15 == 3   # 40 Gaussians behind the near plane, in every workgroup (the tail's: 513, ..., 588)
PUSHED = torch.arange(P) % 20 == 7   # 30 beyond the 1.3 tanfov clamp
GRAD_NAMES = dict(shs="sh", scales="scales", rotations="rotations", cov3D_precomp="cov3D_precomp")


@functools.lru_cache(maxsize=None)
def _base():
    cloud, cam = helpers.cloud_and_camera(P, W, H, sh_degree=3, seed=71, scale_mul=1.3)
    cloud.xyz[CULLED, 2] = -3.5
    cloud.xyz[PUSHED, 0] *= 3.0
    cloud.shs[:, 0] -= 1.2 * (torch.arange(P) % 7 == 0).float()[:, None]  # clamp bits
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(17))
    return cloud, cam, gimg


def _scene(deg, M, above=None):
    """The base scene with its coefficients cut to [:, :M] and the active degree `deg`.  `above`: a seed; the coefficients
    above the degree are then replaced by random values ten times the size of the others."""
    from gsplat_mi355.scenes import GaussianCloud
    base, cam, gimg = _base()
    shs = base.shs[:, :M].clone()
    nb = (deg + 1) ** 2
    if above is not None:
        shs[:, nb:] = 0.5 * torch.randn(P, M - nb, 3, generator=torch.Generator().manual_seed(above))
    cloud = GaussianCloud(base.xyz.clone(), base.scales.clone(), base.rotations.clone(), base.opacity.clone(), shs.contiguous(), deg)
    return cloud, cam, gimg


def _sh_leaf(shs, offset):
    """A leaf whose contiguous (P, M, 3) view starts `offset` floats into its storage: (leaf, view)."""
    from gsplat_mi355 import _lib
    store = torch.zeros(shs.numel() + offset, device=DEV)
    store[offset:] = shs.reshape(-1).to(DEV)
    store.requires_grad_(True)
    view = store[offset:].view(shs.shape)
    assert view.is_contiguous() and _lib.is_aligned(view) == (offset == 0)
    return store, view


def _render(cloud, cam, gimg, offset, cov_mode):
    """One forward and one backward through GaussianRasterizer: (outputs as numpy, the tensors of the call)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    kw = {k: v.clone().requires_grad_(True) for k, v in _inputs(cloud, cam, "sh", cov_mode, DEV).items()}
    store, kw["shs"] = _sh_leaf(cloud.shs, offset)
    means3D = cloud.xyz.to(DEV).requires_grad_(True)
    means2D = torch.zeros(P, 3, device=DEV, requires_grad=True)
    opac = cloud.opacity.to(DEV).requires_grad_(True)
    settings = _settings(cam, cloud, BG, DEV)
    color, radii = GaussianRasterizer(settings)(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    (color * gimg.to(DEV)).sum().backward()
    assert not store.grad[:offset].any()
    out = dict(color=color.detach(), radii=radii, means3D=means3D.grad, means2D=means2D.grad, opacities=opac.grad,
               sh=store.grad[offset:].view(cloud.shs.shape))
    out.update({GRAD_NAMES[k]: v.grad for k, v in kw.items() if k != "shs"})
    return {k: v.cpu().numpy() for k, v in out.items()}, (settings, means3D, opac, kw)


CASES = [
    # deg, M, offset of the coefficients in their storage (floats), covariance input
    (0, 16, 0, "scale_rot"), (1, 16, 0, "scale_rot"), (2, 16, 0, "scale_rot"),  # float4 paths, rows above the degree
    (3, 16, 1, "scale_rot"),   # the scalar paths at full degree
    (1, 16, 1, "scale_rot"),   # scalar loads; float4 store of dL_dsh (the wrapper's fresh tensor is aligned)
    (0, 8, 0, "scale_rot"),    # float4 tile moves of 6 per row, scalar preprocess
    (1, 12, 0, "scale_rot"), (2, 12, 0, "scale_rot"),  # float4 tile moves of 9 per row
    (0, 5, 0, "scale_rot"), (1, 7, 0, "scale_rot"), (2, 11, 0, "scale_rot"),  # odd rows: scalar everywhere
    (1, 16, 0, "cov"),         # the other covariance input
]


@pytest.mark.parametrize("deg,M,offset,cov_mode", CASES,
                         ids=["deg%d-M%d-%s%s" % (d, m, "off4" if o else "aligned", "-cov3D" if c == "cov" else "") for d, m, o, c in CASES])
def test_degree_below_the_stored_coefficients_against_oracle(oracle, deg, M, offset, cov_mode):
    """One frame, forward and backward, per (deg, M, alignment) branch of preprocess.hip / gaussian_bwd.hip / the SH tile
    moves: radii exact, the image the bits of debug.forward_state, every forward difference from the oracle attributed
    to a threshold decision, every gradient element within SMALL_TOL of its tensor's maximum of the conditioned oracle,
    the clamp mask the oracle's, and the gradient of every coefficient above the degree exactly zero on every Gaussian
    (visible, culled, in the tail workgroup)."""
    cloud, cam, gimg = _scene(deg, M)
    sc = helpers.oracle_scene(cloud, cam, bg=BG, cov_mode=cov_mode)
    assert (sc.sh_degree, sc.M) == (deg, M)
    fw = oracle.forward(sc)
    got, (settings, means3D, opac, kw) = _render(cloud, cam, gimg, offset, cov_mode)
    tag = "deg %d M %d offset %d %s" % (deg, M, offset, cov_mode)
    vis = fw["radii"] > 0
    assert np.array_equal(got["radii"], fw["radii"]), tag
    # the scene reaches what it is meant to: culled and visible Gaussians in the tail workgroup, clamped colours
    assert not vis[CULLED.numpy()].any() and (~vis[512:]).any() and vis[512:].any() and vis[PUSHED.numpy()].any()
    assert fw["geom"]["clamped"][vis].sum() > 10
    st, fwc, ov = _conditioned_oracle(oracle, sc, fw, settings, means3D, opac, kw, "sh layouts " + tag)
    assert np.array_equal(got["color"], st["color"]), tag
    cl = st["geom"]["clamped"]
    bits = np.stack([(cl >> c) & 1 for c in range(3)], 1)
    assert np.array_equal(bits[vis], fw["geom"]["clamped"][vis]), tag
    want = oracle.backward(sc, fwc, gimg.numpy(), ov)
    names = ["means3D", "means2D", "opacities", "sh"] + (["scales", "rotations"] if cov_mode == "scale_rot" else ["cov3D_precomp"])
    for name in names:
        w = want[name].reshape(got[name].shape)
        assert np.abs(w).max() > 0, tag + " " + name
        _bulk_close(got[name], w, tol=SMALL_TOL, frac=0.0, name=tag + " " + name)
    nb = (deg + 1) ** 2
    assert got["sh"].shape == (P, M, 3)
    assert (got["sh"][:, nb:, :] == 0).all(), tag
    assert (got["sh"][~vis] == 0).all(), tag


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_layout_of_the_coefficients_changes_no_bit(deg):
    """The same scene with its coefficients stored three ways -- (a) M = (deg+1)^2, the layout the rest of the suite
    runs; (b) M = 16 with the same first (deg+1)^2 coefficients and random values above them; (c) as (b), starting 4 bytes
    off a 16-byte boundary -- and (b) once more with other values above the degree.  The layouts only change how the
    coefficients travel (dwordx4 or dword loads, through registers or LDS): the arithmetic is one expression per kernel
    and the coefficients above the degree enter no sum, so image, radii, every gradient and dL_dsh[:, :(deg+1)^2] agree
    bit for bit, and the rest of dL_dsh is zero."""
    nb = (deg + 1) ** 2
    runs = {}
    for name, M, above, offset in [("a", nb, None, 0), ("b", 16, 1, 0), ("b2", 16, 2, 0), ("c", 16, 1, 1)]:
        cloud, cam, gimg = _scene(deg, M, above)
        runs[name], _ = _render(cloud, cam, gimg, offset, "scale_rot")
    a = runs["a"]
    assert (a["radii"] > 0).sum() > 400 and np.abs(a["sh"]).max() > 0
    for name in ("b2", "b", "c"):  # (b2 first: coefficients above the degree that leak into a sum show here)
        r = runs[name]
        ref = runs["b"] if name == "b2" else a
        for k in ("color", "radii", "means3D", "means2D", "opacities", "scales", "rotations"):
            assert np.array_equal(r[k], ref[k]), (name, k, np.abs(r[k] - ref[k]).max())
        assert np.array_equal(r["sh"][:, :nb], ref["sh"][:, :nb]), (name, np.abs(r["sh"][:, :nb] - ref["sh"][:, :nb]).max())
        assert (r["sh"][:, nb:] == 0).all(), name


# ---- the pre-pass: sh2rgb

CAMPOS = np.array([0.3, -0.2, 4.0], np.float32)
SH2RGB_LAYOUTS = [(0, 1), (0, 16), (1, 4), (1, 7), (2, 9), (2, 16), (3, 16)]
SH2RGB_SIZES = [1, 255, 256, 257, 1000]


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                     1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                     1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3).astype(np.float32)


def _sh2rgb_inputs(deg, M, n, use_rot, seed=0):
    """(features (n, M, 3), xyz, bone transforms (n, 4, 4) or None, gradient of the colours), all coefficients random
    (those above the degree too)."""
    rng = np.random.default_rng(100000 * seed + 10000 * deg + 500 * M + 2 * n + int(use_rot))
    feats = (0.5 * rng.normal(size=(n, M, 3))).astype(np.float32)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    T = None
    if use_rot:
        T = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        T[:, :3, :3] = _rotations(rng, n)
        T[:, :3, 3] = rng.normal(size=(n, 3))
    gcol = rng.normal(size=(n, 3)).astype(np.float32)
    return feats, xyz, T, gcol


def _sh2rgb_keep(oracle, feats, xyz, deg, R):
    """Rows whose three pre-clamp values all lie further than 1e-5 from zero, from the oracle alone (a second run with
    +1 on every channel through the DC term, as test_sh2rgb_matches_oracle): a colour within rounding of the clamp may
    fall on the other side, and its gradient with it."""
    shifted = feats.copy()
    shifted[:, 0, :] += np.float32(1.0 / 0.28209479177387814)
    col1, _ = oracle.sh2rgb(shifted, xyz, CAMPOS, deg, R, None)
    r = col1.astype(np.float64) - 1.0  # exact where r > -1; anything below is safely clamped
    return (np.abs(r) > 1e-5).all(1)


def _check_sh2rgb(oracle, deg, feats, xyz, T, gcol, offset=0):
    from gsplat_mi355.prepass import sh2rgb
    n, M = feats.shape[:2]
    R = None if T is None else np.ascontiguousarray(T[:, :3, :3])
    want_col, want_cl, want_dsh, want_dp = oracle.sh2rgb(feats, xyz, CAMPOS, deg, R, None, gcol)
    col64, dsh64, dp64 = helpers.sh2rgb_float64(feats, xyz, CAMPOS, deg, R, None, gcol)
    keep = _sh2rgb_keep(oracle, feats, xyz, deg, R)
    assert (~keep).mean() <= 0.01 and (n >= 100 or keep.all())
    store, f = _sh_leaf(torch.from_numpy(feats), offset)
    p = torch.from_numpy(xyz).to(DEV).requires_grad_(True)
    col = sh2rgb(f, p, torch.from_numpy(CAMPOS).to(DEV), deg, fwd_transform=None if T is None else torch.from_numpy(T).to(DEV))
    (col * torch.from_numpy(gcol).to(DEV)).sum().backward()
    got = col.detach().cpu().numpy()
    assert got.shape == (n, 3)
    gd, gp = store.grad[offset:].view(n, M, 3).cpu().numpy(), p.grad.cpu().numpy()
    assert not store.grad[:offset].any()
    for ref_col, ref_dsh, ref_dp in ((want_col, want_dsh, want_dp), (col64, dsh64, dp64)):
        assert np.abs(got - ref_col).max() <= 2e-6
        assert np.abs(gd[keep] - ref_dsh[keep]).max() <= 1e-5 * np.abs(ref_dsh).max()
        assert np.abs(gp[keep] - ref_dp[keep]).max() <= 1e-5 * np.abs(ref_dp).max()
    assert np.abs(want_dsh).max() > 0 and (deg == 0 or np.abs(want_dp).max() > 0)
    nb = (deg + 1) ** 2
    assert (gd[:, nb:, :] == 0).all()  # coefficients above the active degree get exactly zero


@pytest.mark.parametrize("use_rot", [False, True], ids=["world-dir", "cano-dir"])
@pytest.mark.parametrize("n", SH2RGB_SIZES)
@pytest.mark.parametrize("deg,M", SH2RGB_LAYOUTS)
def test_sh2rgb_at_every_coefficient_count_branch_and_block_edge(oracle, deg, M, n, use_rot):
    """sh2rgb and its backward with M = 16 (dwordx4 loads and stores) and M < 16 (dword loads of the 3 M floats there
    are, zero above them), degree below and at what M holds, one Gaussian, one short of / exactly / one past a
    workgroup, several workgroups with a tail; with and without the bone rotation.  Against oracle.sh2rgb and
    helpers.sh2rgb_float64 at the bars of test_sh2rgb_matches_oracle: colours 2e-6, gradients 1e-5 of each tensor's
    maximum except on rows within 1e-5 of the clamp (at most 1 % of the rows, none below 100 rows; with these seeds
    no row of any case: the largest share is 0), gradients above the degree exactly zero."""
    _check_sh2rgb(oracle, deg, *_sh2rgb_inputs(deg, M, n, use_rot))


@pytest.mark.parametrize("deg", [1, 3])
def test_sh2rgb_of_coefficients_off_a_16_byte_boundary(oracle, deg):
    """An (N, 16, 3) view that starts 4 bytes past a boundary: the dword branch of the loads, and of the gradient store,
    at M = 16 (the gradient tensor itself is fresh and aligned: either operand off the boundary selects it)."""
    _check_sh2rgb(oracle, deg, *_sh2rgb_inputs(deg, 16, 257, True, seed=1), offset=1)


@pytest.mark.parametrize("use_rot", [False, True], ids=["world-dir", "cano-dir"])
def test_sh2rgb_of_a_point_at_the_camera_centre(oracle, use_rot):
    """The reference normalises the view direction as dir / (|dir| + 1e-12) (models/texture/texture.py:35): a point at
    the camera centre has the direction 0, the colour of its DC term alone, and a finite position gradient
    d colour / d dir / 1e-12 -- of order 1e12, so that row is compared on its own, relative to its own magnitude, and the
    other rows against a maximum taken without it.  torch's float64 autograd gives exactly that value (the subgradient
    of the norm at 0 is 0, which is the kernel's k2 = 0 branch); it is also written out below, ddir / 1e-12 with
    ddir = sum_c g_c C1 (-sh[3, c], -sh[1, c], sh[2, c]) for directions of length 0 (rotated back by R when the bone
    rotation is in), so the expectation does not rest on that convention."""
    from gsplat_mi355.prepass import sh2rgb
    n, row, deg = 300, 123, 3
    feats, xyz, T, gcol = _sh2rgb_inputs(deg, 16, n, use_rot, seed=2)
    xyz[row] = CAMPOS
    feats[row, 0] = (0.8, -0.3, 2.0)  # colours 0.73, 0.42, 1.06: none clamped
    R = None if T is None else np.ascontiguousarray(T[:, :3, :3])
    want_col, _, want_dsh, want_dp = oracle.sh2rgb(feats, xyz, CAMPOS, deg, R, None, gcol)
    col64, dsh64, dp64 = helpers.sh2rgb_float64(feats, xyz, CAMPOS, deg, R, None, gcol)
    C1 = 0.4886025119029199
    f64, g64 = feats[row].astype(np.float64), gcol[row].astype(np.float64)
    ddir = C1 * np.array([-(f64[3] * g64).sum(), -(f64[1] * g64).sum(), (f64[2] * g64).sum()])
    analytic = (R[row].astype(np.float64) @ ddir if use_rot else ddir) / 1e-12
    assert np.isfinite(dp64[row]).all() and np.abs(dp64[row] - analytic).max() <= 1e-9 * np.abs(analytic).max()
    assert np.abs(analytic).max() > 1e10
    keep = _sh2rgb_keep(oracle, feats, xyz, deg, R)
    assert keep[row] and (~keep).mean() <= 0.01
    others = keep.copy()
    others[row] = False
    f = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    p = torch.from_numpy(xyz).to(DEV).requires_grad_(True)
    col = sh2rgb(f, p, torch.from_numpy(CAMPOS).to(DEV), deg, fwd_transform=None if T is None else torch.from_numpy(T).to(DEV))
    (col * torch.from_numpy(gcol).to(DEV)).sum().backward()
    got, gd, gp = col.detach().cpu().numpy(), f.grad.cpu().numpy(), p.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(gd).all() and np.isfinite(gp).all()
    assert np.abs(got - want_col).max() <= 2e-6 and np.abs(got - col64).max() <= 2e-6
    assert np.abs(got[row] - (0.28209479177387814 * f64[0] + 0.5)).max() <= 2e-6
    assert np.abs(gp[row] - dp64[row]).max() <= 1e-5 * np.abs(dp64[row]).max()
    assert np.abs(gp[row] - analytic).max() <= 1e-5 * np.abs(analytic).max()
    assert np.abs(gd[row] - dsh64[row]).max() <= 1e-5 * np.abs(dsh64[row]).max()
    rest = np.arange(n) != row
    for ref_dsh, ref_dp in ((want_dsh, want_dp), (dsh64, dp64)):
        assert np.abs(gd[others] - ref_dsh[others]).max() <= 1e-5 * np.abs(ref_dsh[rest]).max()
        assert np.abs(gp[others] - ref_dp[others]).max() <= 1e-5 * np.abs(ref_dp[rest]).max()


# ---- the pre-pass: covariance from scaling and rotation

COV_SIZES = [1, 255, 256, 257]
COV_MODIFIER = 1.25  # (exact in fp32: the float64 restatement and the kernel see the same number)
COV_TENSORS = ("cov6", "d/dscaling", "d/drotation")


def _cov_inputs(n, matrix):
    """Scalings log-uniform over 1e-4 .. 10 (per component: needles among them), quaternions that are not unit or
    rotation matrices, a random upstream gradient."""
    rng = np.random.default_rng(7000 + 2 * n + int(matrix))
    scaling = (10.0 ** rng.uniform(-4.0, 1.0, (n, 3))).astype(np.float32)
    if matrix:
        rot = _rotations(rng, n)
    else:
        rot = (rng.normal(size=(n, 4)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    g6 = rng.normal(size=(n, 6)).astype(np.float32)
    return scaling, rot, g6


def _row_err(got, ref):
    """Per row: the largest error of the row over the largest reference magnitude of the row."""
    got = np.asarray(got, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    return np.abs(got - ref).max(1) / np.abs(ref).max(1)


# What an fp32 evaluation of this chain loses per row, measured on the CPU: the reference's own lines in torch float32
# (helpers.covariance_float64 with dtype=torch.float32) against the same lines in float64, largest _row_err over the
# rows of all of COV_SIZES' inputs.  (oracle.build_covariance is no such measure: it evaluates in double and rounds its
# outputs once, 6.0e-8 on these inputs.)  The kernel's bar is four times this; the factor allows for another association
# order and for FMA contraction.  tests/test_oracle.py re-measures these numbers on the host.  Keys: (rotation matrices?,
# tensor).
COV_ROW_ERR_OF_FP32 = {
    (False, "cov6"): 1.05e-6, (False, "d/dscaling"): 1.93e-4, (False, "d/drotation"): 3.61e-6,
    (True, "cov6"): 2.62e-7, (True, "d/dscaling"): 4.68e-6, (True, "d/drotation"): 3.30e-7,
}
# (d/dscaling of row b is 2 s_b (R^T (G + G^T) R)_bb: a quadratic form of an indefinite matrix, near zero on some rows,
# and a row's own magnitude is then a poor scale for its rounding errors -- the 1.9e-4 is one such row of the 769)


def measure_fp32_row_err(fn=None):
    """COV_ROW_ERR_OF_FP32, measured: `fn(scaling, modifier, rotation, g6)` (default: the float32 torch restatement)
    against the float64 one."""
    fn = fn or (lambda *a: helpers.covariance_float64(*a, dtype=torch.float32))
    out = {}
    for matrix in (False, True):
        for n in COV_SIZES:
            inputs = _cov_inputs(n, matrix)
            got = fn(inputs[0], COV_MODIFIER, *inputs[1:])
            ref = helpers.covariance_float64(inputs[0], COV_MODIFIER, *inputs[1:])
            for name, g, r in zip(COV_TENSORS, got, ref):
                out[(matrix, name)] = max(out.get((matrix, name), 0.0), float(_row_err(g, r).max()))
    return out


@pytest.mark.parametrize("n", COV_SIZES)
@pytest.mark.parametrize("matrix", [False, True], ids=["quaternions", "matrices"])
def test_build_covariance_per_row_over_five_decades_of_scale(oracle, matrix, n):
    """build_covariance_from_scaling_rotation at one Gaussian, one short of / exactly / one past a workgroup, scalings
    over 1e-4 .. 10 (the needle scenes, a trained avatar).  The bar of test_build_covariance_matches_oracle -- 1e-5 of
    each tensor's maximum against oracle.build_covariance -- is set by the largest Gaussians alone and would pass a
    kernel that is wrong on every small one, so also per row: the error of cov6, d/dscaling and d/drotation against
    helpers.covariance_float64 over that row's own largest reference magnitude, within four times what the same chain
    evaluated in fp32 on the CPU loses on the same inputs (COV_ROW_ERR_OF_FP32, measured: quaternions 1.05e-6 / 1.93e-4 /
    3.61e-6, matrices 2.62e-7 / 4.68e-6 / 3.30e-7, so the bars are 4.2e-6 / 7.7e-4 / 1.4e-5 and 1.0e-6 / 1.9e-5 / 1.3e-6;
    the kernel's own error is not the yardstick)."""
    from gsplat_mi355.prepass import build_covariance_from_scaling_rotation
    scaling, rot, g6 = _cov_inputs(n, matrix)
    want = oracle.build_covariance(scaling, COV_MODIFIER, rot, g6)
    ref = helpers.covariance_float64(scaling, COV_MODIFIER, rot, g6)
    s = torch.from_numpy(scaling).to(DEV).requires_grad_(True)
    r = torch.from_numpy(rot).to(DEV).requires_grad_(True)
    cov = build_covariance_from_scaling_rotation(s, COV_MODIFIER, r)
    (cov * torch.from_numpy(g6).to(DEV)).sum().backward()
    got = [t.cpu().numpy() for t in (cov.detach(), s.grad, r.grad)]
    for name, g, w, r64 in zip(COV_TENSORS, got, want, ref):
        assert g.shape == w.shape
        assert np.abs(g - w).max() <= 1e-5 * np.abs(w).max(), name
        err = float(_row_err(g, r64).max())
        bar = 4.0 * COV_ROW_ERR_OF_FP32[(matrix, name)]
        print("build_covariance %s n=%d %s: per-row error %.3g (bar %.3g)" % ("matrices" if matrix else "quaternions", n, name, err, bar))
        assert err <= bar, (name, err, bar)
