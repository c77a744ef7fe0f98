"""The rasterizer under general cameras and scale_modifier != 1.

Every scene of test_gpu_parity.py is seen through the orbit camera (helpers.cloud_and_camera): one focal length for both
axes, a pure yaw about y (mostly frame 0, the identity), the camera outside the cloud, scale_modifier 1.  A swap of fx / fy
or tanfovx / tanfovy in one term, a row / column mix-up in the view matrix's y row, a wrong y_grad_mul or a lost modifier
passes all of it.  Here the same HIP path runs under helpers.POSES -- `general` (every entry of the view rotation
non-zero, fx != fy, off-axis translation), `inside` (the camera in the cloud: near-plane culls, on-screen radii of
hundreds of pixels with clamped rectangles, the 1.3 tanfov Jacobian clamp active in x and in y), `roll90` (x and y
exchanged, fx != fy) -- with scale_modifier 0.6 / 1.7, against the CPU oracle (integers exact, floats conditioned on the
attributed threshold decisions) and, independently of it, against float64 autograd of oracle/dense_ref.py.  The oracle
itself is pinned under these cameras by test_oracle.py::test_backward_matches_float64_autograd_under_general_cameras.

Every test asserts the preconditions of its pose (test_oracle.assert_pose_preconditions) before it compares anything."""
import numpy as np
import pytest
import torch

import helpers
from test_gpu_parity import COMBOS, SMALL_TOL, _bulk_close, _conditioned_oracle, _inputs, _settings, tile_rect  # noqa: F401
from test_oracle import CAMERA_BG, CAMERA_COMBOS, assert_pose_preconditions, camera_case

pytestmark = pytest.mark.gpu

POSE_NAMES = ["general", "inside", "roll90"]
POSE_SEED = {"general": 51, "inside": 52, "roll90": 53}
GRAD_NAMES = dict(shs="sh", colors_precomp="colors_precomp", scales="scales", rotations="rotations",
                  cov3D_precomp="cov3D_precomp")


def _leaves(cloud, cam, color_mode, cov_mode, dev, mod):
    kw = {k: v.clone().requires_grad_(True) for k, v in _inputs(cloud, cam, color_mode, cov_mode, dev, mod).items()}
    means3D = cloud.xyz.to(dev).requires_grad_(True)
    means2D = torch.zeros(cloud.num, 3, device=dev, requires_grad=True)
    opac = cloud.opacity.to(dev).requires_grad_(True)
    return means3D, means2D, opac, kw


def _grads(means3D, means2D, opac, kw):
    got = dict(means3D=means3D.grad, means2D=means2D.grad, opacities=opac.grad)
    for k, v in kw.items():
        got[GRAD_NAMES[k]] = v.grad
    return got


@pytest.mark.parametrize("combo", range(len(COMBOS)), ids=["%s-%s-%d" % c for c in COMBOS])
@pytest.mark.parametrize("pose", POSE_NAMES)
def test_posed_cameras_against_the_oracle(oracle, tile_rect, pose, combo):
    """2500 Gaussians on a ragged 112x72 image (35 tiles, up to ~38 k pairs, lists of over a thousand entries), every
    input combination, both tile-rectangle modes, scale_modifier 0.6 (even combinations) / 1.7 (odd ones): radii,
    tiles_touched, the sorted lists, the tile ranges and the pair count bit-exact; every difference of the image attributed
    to decisions at a threshold; every gradient within 1e-5 of the maximum of the oracle conditioned on them, no exempt
    element; exact zeros for every Gaussian that reaches no tile.  Measured over the 30 cases on an MI355X: no threshold
    decision flipped, gradients within 5.9e-6 (means2D; cov3D_precomp 3.3e-6, means3D 2.0e-6, the others <= 1.4e-6)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    color_mode, cov_mode, deg = COMBOS[combo]
    mod = 0.6 if combo % 2 == 0 else 1.7
    n, W, H = 2500, 112, 72
    cloud, _ = helpers.cloud_and_camera(n, W, H, sh_degree=deg, seed=POSE_SEED[pose])
    cloud.shs[:, 0] -= 1.2 * (torch.arange(n) % 5 == 0).float()[:, None]  # some colours clamp at 0
    cam = helpers.posed_camera(pose, W, H)
    bg = (0.3, 0.6, 0.1)
    sc = helpers.oracle_scene(cloud, cam, bg=bg, color_mode=color_mode, cov_mode=cov_mode, scale_modifier=mod,
                              tile_rect=tile_rect)
    fw = oracle.forward(sc)
    vs = assert_pose_preconditions(pose, cloud, cam, fw["radii"])
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5))
    settings = _settings(cam, cloud, bg, dev, scale_modifier=mod)
    means3D, means2D, opac, kw = _leaves(cloud, cam, color_mode, cov_mode, dev, mod)
    color, radii = GaussianRasterizer(settings)(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    (color * gimg.to(dev)).sum().backward()
    tag = "cameras %s %s/%s deg %d mod %g tile_rect=%d" % (pose, color_mode, cov_mode, deg, mod, tile_rect)
    # --- integers: bit-exact (before any float is looked at)
    assert np.array_equal(radii.cpu().numpy(), fw["radii"]), tag
    from gsplat_mi355 import debug
    st = debug.forward_state(settings, means3D.detach(), opac.detach(), **{k: v.detach() for k, v in kw.items()})
    og, ob = fw["geom"], fw["binning"]
    assert np.array_equal(st["radii"], og["radii"]), tag
    assert np.array_equal(st["geom"]["tiles_touched"], og["tiles_touched"]), tag
    assert st["D"] == ob["D"] and ob["D"] > 3000, tag
    assert np.array_equal(st["binning"]["point_list"], ob["point_list"]), tag
    nz = ob["ranges"][:, 1] > ob["ranges"][:, 0]
    assert np.array_equal(st["image"]["ranges"][nz], ob["ranges"][nz]), tag
    assert (st["image"]["ranges"][~nz, 1] == st["image"]["ranges"][~nz, 0]).all(), tag
    # --- floats: the oracle conditioned on the attributed threshold decisions (asserts that no pixel is left unattributed)
    st, fwc, ov = _conditioned_oracle(oracle, sc, fw, settings, means3D, opac, kw, tag)
    assert np.array_equal(color.detach().cpu().numpy(), st["color"]), tag
    want = oracle.backward(sc, fwc, gimg.numpy(), ov)
    got = {k: v.cpu().numpy() for k, v in _grads(means3D, means2D, opac, kw).items()}
    for name, gt in got.items():
        w = want[name].reshape(gt.shape)
        if np.abs(w).max() == 0:
            assert np.abs(gt).max() == 0, tag + " " + name
            continue
        print("ERR3a %s | %s | %.3g | flips %d" % (tag, name, helpers.rel_to_max(gt, w), len(ov)))
        _bulk_close(gt, w, tol=SMALL_TOL, frac=0.0, name=tag + " " + name)
    for name in ("means3D", "opacities") + tuple(GRAD_NAMES[k] for k in kw):
        assert np.abs(want[name]).max() > 0, tag + " " + name
    # --- a Gaussian that reaches no tile (behind the near plane, off the screen) gets exact zeros
    nowhere = fw["radii"] == 0
    if pose == "inside":
        wv = cam.world_view_transform.numpy().astype(np.float64)
        behind = (cloud.xyz.numpy().astype(np.float64) @ wv[:3, :3] + wv[3, :3])[:, 2] <= 0.2
        assert behind.sum() == vs["culled"] > 0 and nowhere[behind].all(), tag
    for name, gt in got.items():
        assert (gt[nowhere] == 0).all(), tag + " " + name


@pytest.mark.parametrize("color_mode,cov_mode,deg,mod", CAMERA_COMBOS)
@pytest.mark.parametrize("pose", POSE_NAMES)
def test_posed_cameras_against_dense_float64_autograd_directly(pose, color_mode, cov_mode, deg, mod):
    """The independent path of test_hip_path_against_dense_float64_autograd_directly -- the HIP rasterizer against
    oracle/dense_ref.py with autograd, not through the C oracle -- under every pose, with the input combinations and
    modifiers of the oracle's own test (test_oracle.camera_case: n = 300, 48x32), at that test's bars: radii equal, image
    within 1e-5, every gradient within 2e-4 of its maximum.  Measured over the nine cases on an MI355X: image within
    8.2e-7, gradients within 4.1e-6 (means2D; means3D 2.4e-6, the others <= 1.3e-6)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    cloud, cam, sc, gimg, (color64, radii64, grads64) = camera_case(pose, color_mode, cov_mode, deg, mod)
    assert_pose_preconditions(pose, cloud, cam, radii64)
    means3D, means2D, opac, kw = _leaves(cloud, cam, color_mode, cov_mode, dev, mod)
    settings = _settings(cam, cloud, CAMERA_BG, dev, scale_modifier=mod)
    color, radii = GaussianRasterizer(settings)(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    (color * torch.from_numpy(gimg).to(dev)).sum().backward()
    tag = "%s %s/%s deg %d mod %g" % (pose, color_mode, cov_mode, deg, mod)
    assert np.array_equal(radii.cpu().numpy(), radii64), tag
    err = np.abs(color.detach().cpu().numpy() - color64).max()
    print("ERR3b %s | image | %.3g" % (tag, err))
    assert err < 1e-5, (tag, err)
    got = _grads(means3D, means2D, opac, kw)
    for name, ref in grads64.items():
        err = helpers.rel_to_max(got[name].cpu().numpy().reshape(ref.shape), ref)
        print("ERR3b %s | %s | %.3g" % (tag, name, err))
        assert err < 2e-4, (tag, name, err)


def test_scale_modifier_has_no_effect_on_precomputed_covariances():
    """Upstream applies scale_modifier where it builds the covariance from scales and rotations, and nowhere else: with
    cov3D_precomp the same tensors give the same bits -- colour, radii, every gradient -- under modifier 1.0 and 1.7 (the
    oracle behaves the same way)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    n, W, H = 2500, 112, 72
    cloud, _ = helpers.cloud_and_camera(n, W, H, sh_degree=2, seed=POSE_SEED["general"])
    cam = helpers.posed_camera("general", W, H)
    assert_pose_preconditions("general", cloud, cam)
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    cov = helpers.covariance6_cpu(cloud, 1.3).to(dev)
    out = []
    for mod in (1.0, 1.7):
        leaves = dict(means3D=cloud.xyz.to(dev).requires_grad_(True), means2D=torch.zeros(n, 3, device=dev, requires_grad=True),
                      opacities=cloud.opacity.to(dev).requires_grad_(True), shs=cloud.shs.to(dev).requires_grad_(True),
                      cov3D_precomp=cov.clone().requires_grad_(True))
        color, radii = GaussianRasterizer(_settings(cam, cloud, (0.3, 0.6, 0.1), dev, scale_modifier=mod))(**leaves)
        (color * gimg).sum().backward()
        out.append([color.detach(), radii] + [leaves[k].grad for k in sorted(leaves)])
    assert int((out[0][1] > 0).sum()) > n // 2 and float(out[0][0].std()) > 0
    for a, b in zip(*out):
        assert float(a.float().abs().max()) > 0
        assert torch.equal(a, b)


@pytest.mark.parametrize("pose", ["general", "inside"])
def test_mark_visible_under_posed_cameras(oracle, pose):
    """markVisible reads the view matrix's z column alone; the cloud is stretched so that under either pose part of it lies
    behind the 0.2 near plane."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    n = 5000
    cloud, _ = helpers.cloud_and_camera(n, 64, 64, sh_degree=0, seed=2)
    cloud.xyz = cloud.xyz * 3.0
    cam = helpers.posed_camera(pose, 64, 64)
    assert np.abs(cam.world_view_transform.numpy()[:3, :3]).min() > 0.05
    got = GaussianRasterizer(_settings(cam, cloud, (0, 0, 0), dev)).markVisible(cloud.xyz.to(dev)).cpu().numpy()
    want = oracle.mark_visible(cloud.xyz.numpy(), cam.world_view_transform.numpy())
    assert 0 < want.sum() < n and want.sum() == n - helpers.view_stats(cloud, cam)["culled"]
    assert got.dtype == np.bool_ and np.array_equal(got, want)


def _inside_scene(n, W, H):
    cloud, _ = helpers.cloud_and_camera(n, W, H, sh_degree=2, seed=POSE_SEED["inside"], scale_mul=1.2)
    cam = helpers.posed_camera("inside", W, H)
    return cloud, cam


def test_fused_opacity_render_inside_the_cloud(oracle):
    """test_fused_opacity_render_matches_the_second_rasterizer_call with the camera inside the cloud and scale_modifier
    0.6: rasterizer(..., with_opacity=True) against the two calls of the reference (the second one served from the first
    one's geometry) and against the oracle's render with colours = 1, at that test's bars."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    n, W, H = 3000, 150, 110
    bgval, mod = (0.3, 0.6, 0.1), 0.6
    cloud, cam = _inside_scene(n, W, H)
    gen = torch.Generator().manual_seed(8)
    gimg = torch.randn(3, H, W, generator=gen).to(dev)
    gop = torch.randn(1, H, W, generator=gen).to(dev)
    rast = GaussianRasterizer(_settings(cam, cloud, bgval, dev, scale_modifier=mod))

    def leaves():
        return dict(means3D=cloud.xyz.to(dev).clone().requires_grad_(True),
                    means2D=torch.zeros(n, 3, device=dev, requires_grad=True),
                    opacities=cloud.opacity.to(dev).clone().requires_grad_(True),
                    shs=cloud.shs.to(dev).clone().requires_grad_(True),
                    scales=cloud.scales.to(dev).clone().requires_grad_(True),
                    rotations=cloud.rotations.to(dev).clone().requires_grad_(True))

    a = leaves()
    color, radii, opa = rast(with_opacity=True, **a)
    assert_pose_preconditions("inside", cloud, cam, radii.cpu().numpy())
    ((color * gimg).sum() + (opa * gop).sum()).backward()
    b = leaves()
    dgr.release_shared_geometry()
    hits0 = dgr._geom_cache.hits
    color2, radii2 = rast(**b)
    opa2, _ = rast(means3D=b["means3D"], means2D=b["means2D"], opacities=b["opacities"], shs=None,
                   colors_precomp=torch.ones(n, 3, device=dev), scales=b["scales"], rotations=b["rotations"])
    assert dgr._geom_cache.hits - hits0 == 1  # the second call was served from the first one's geometry
    ((color2 * gimg).sum() + (opa2[:1] * gop).sum()).backward()
    assert torch.equal(color, color2) and torch.equal(radii, radii2)
    assert np.abs((opa - opa2[:1]).detach().cpu().numpy()).max() <= 2e-6
    sc = helpers.oracle_scene(cloud, cam, bg=bgval, color_mode="precomp", cov_mode="scale_rot", colors=torch.ones(n, 3),
                              scale_modifier=mod)
    want = oracle.forward(sc)
    assert np.array_equal(radii.cpu().numpy(), want["radii"])
    assert np.abs(opa[0].detach().cpu().numpy() - want["color"][0]).max() <= 1e-2
    _bulk_close(opa[0].detach().cpu().numpy(), want["color"][0], name="opacity render")
    for k in a:
        assert float(b[k].grad.abs().max()) > 0
        _bulk_close(a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy(), tol=2e-5, frac=1e-4, name="fused vs two calls: " + k)


def test_shared_geometry_second_render_inside_the_cloud():
    """test_shared_geometry_second_render_is_bitwise_identical (each call with its own backward) with the camera inside the
    cloud, scales and rotations as inputs and scale_modifier 0.6: the second render served from the first one's geometry
    gives the bits -- both images, radii, every gradient -- of an independent second call."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    from gsplat_mi355 import _lib
    dev = torch.device("cuda:0")
    n, W, H = 3000, 150, 110
    cloud, cam = _inside_scene(n, W, H)
    settings = _settings(cam, cloud, (0.3, 0.6, 0.1), dev, scale_modifier=0.6)
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
    saved = dgr._SHARE, dgr._FUSE_SECOND

    def run(share):
        dgr._SHARE = share
        dgr.release_shared_geometry()
        hits0 = dgr._geom_cache.hits
        xyz = cloud.xyz.to(dev).requires_grad_(True)
        m2d = torch.zeros(n, 3, device=dev, requires_grad=True)
        op = cloud.opacity.to(dev).requires_grad_(True)
        sca = cloud.scales.to(dev).requires_grad_(True)
        rot = cloud.rotations.to(dev).requires_grad_(True)
        cols = helpers.precomp_colors(cloud, cam).to(dev).requires_grad_(True)
        ones = torch.ones(n, 3, device=dev)
        rast = GaussianRasterizer(settings)
        img1, r1 = rast(means3D=xyz, means2D=m2d, opacities=op, colors_precomp=cols, scales=sca, rotations=rot)
        img2, r2 = rast(means3D=xyz, means2D=m2d, opacities=op, colors_precomp=ones, scales=sca, rotations=rot)
        hits = dgr._geom_cache.hits - hits0
        ((img1 * gimg).sum() + (img2[:1] * gimg[:1]).sum()).backward()
        return [img1.detach(), img2.detach(), r1, r2, xyz.grad, m2d.grad, op.grad, sca.grad, rot.grad, cols.grad], hits

    try:
        dgr._FUSE_SECOND = False
        _lib.tuning("ones_fast", 0)  # (the all-ones image composited, not 1 - T: equal only to fp32 rounding)
        shared, hits = run(True)
        alone, none = run(False)
        assert hits == 1 and none == 0
        assert_pose_preconditions("inside", cloud, cam, shared[2].cpu().numpy())
        for a, b in zip(shared, alone):
            assert float(a.float().abs().max()) > 0
            assert torch.equal(a, b)
    finally:
        dgr._SHARE, dgr._FUSE_SECOND = saved
        dgr.release_shared_geometry()
        _lib.tuning("ones_fast", 1)
