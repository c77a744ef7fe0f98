"""The rasterizer's `antialiasing` option on the device (GsFwdArgs.antialiasing; definition in include/gsplat_mi355.h).

Two clouds of 2048 Gaussians on a 96 x 80 image (six tiles by five, neither side a multiple of 16; 2051 Gaussians, not a
multiple of the 64-lane wave or of the 256-thread workgroup): helpers.cloud_and_camera with scale_mul 1.0 (footprints of a
few pixels, s near 1) and 0.05 (most footprints below a pixel, s << 1), each joined by three hand-placed Gaussians: one
of scale 1e-6 (the clamp on det0 / det1), one whose centre lies half a pixel inside the right image border, one behind
the 0.2 near plane.

The reference for everything the option shares with the default path is the default path itself, run on the effective
opacities o' read back from the device; for what it adds, the float64 restatement tests/antialias_ref.py.  Bounds that
were not known in advance are 4 x the error of the SAME restatement evaluated in fp32 on the CPU against float64 (the
device's operation order differs from the CPU's only in the backward, where FMA contraction is on), never below the
project's parity bar of 1e-5 max|g| per tensor (README).  Every test prints the figures it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

import antialias_ref as ref
import helpers
from helpers import _CallCounter

pytestmark = pytest.mark.gpu

N0, W, H = 2048, 96, 80
CLAMP, BORDER, BEHIND = N0, N0 + 1, N0 + 2  # rows of the hand-placed Gaussians
PARITY = 1e-5                               # |delta| <= 1e-5 max|g| per tensor: the project's parity bar (README)


@functools.lru_cache(maxsize=None)
def _scene(scale_mul):
    cloud, cam = helpers.cloud_and_camera(N0, W, H, sh_degree=3, seed=4, scale_mul=scale_mul)
    V = cam.world_view_transform.numpy().astype(np.float64)
    fx, fy = W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5))
    # (on the centre of pixel (50, 38): alpha = 0.9 * 0.005 G reaches 1/255 only where G > 0.87, within 0.29 px of the centre)
    view_pts = np.array([[(50.5 - W / 2) * 3.0 / fx, (38.5 - H / 2) * 3.0 / fy, 3.0],  # scale 1e-6: clamped
                         [(W / 2 - 0.5) * 3.0 / fx, 0.02, 3.0],     # centre half a pixel inside the right border
                         [0.0, 0.0, 0.1]])                          # behind the 0.2 near plane: culled
    world = (view_pts - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    g = torch.Generator().manual_seed(9)
    q = torch.randn(3, 4, generator=g)
    cloud.xyz = torch.cat([cloud.xyz, torch.from_numpy(world).float()]).contiguous()
    cloud.scales = torch.cat([cloud.scales, torch.tensor([[1e-6] * 3, [0.02, 0.05, 0.03], [0.02] * 3])]).contiguous()
    cloud.rotations = torch.cat([cloud.rotations, q / q.norm(dim=1, keepdim=True)]).contiguous()
    cloud.opacity = torch.cat([cloud.opacity, torch.tensor([[0.9], [0.8], [0.7]])]).contiguous()
    cloud.shs = torch.cat([cloud.shs, cloud.shs[:3]]).contiguous()
    return cloud, cam


def _settings(cam, dev, *tail, sh_degree=3):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
        cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), sh_degree, cam.camera_center.to(dev), False, False, *tail)


def _inputs(cloud, cam, dev, color_mode, cov_mode, opacity=None):
    """Keyword tensors of one rasterizer call in one of the four input combinations (fresh device tensors)."""
    kw = dict(means3D=cloud.xyz.to(dev), opacities=(cloud.opacity if opacity is None else opacity).to(dev))
    if color_mode == "sh":
        kw["shs"] = cloud.shs.to(dev)
    else:
        kw["colors_precomp"] = helpers.precomp_colors(cloud, cam).to(dev)
    if cov_mode == "scale_rot":
        kw["scales"], kw["rotations"] = cloud.scales.to(dev), cloud.rotations.to(dev)
    else:
        kw["cov3D_precomp"] = helpers.covariance6_cpu(cloud).to(dev)
    return kw


def _state(cloud, cam, dev, antialiasing, color_mode="sh", cov_mode="scale_rot", opacity=None):
    from gsplat_mi355 import debug
    kw = _inputs(cloud, cam, dev, color_mode, cov_mode, opacity)
    return debug.forward_state(_settings(cam, dev, antialiasing, sh_degree=cloud.sh_degree), kw.pop("means3D"),
                               kw.pop("opacities"), **kw)


def _effective(cloud, st):
    """o' [n, 1] as the device stored it (record word 5); culled Gaussians (no record) keep o."""
    o = cloud.opacity.numpy().copy()
    vis = st["radii"] > 0
    o[vis, 0] = st["geom"]["rec"][vis, 5]
    return torch.from_numpy(o)


def _ref_scene(cloud, cam, rows, cov_mode="scale_rot", dtype=torch.float64):
    kw = (dict(scales=cloud.scales.numpy(), rotations=cloud.rotations.numpy()) if cov_mode == "scale_rot"
          else dict(cov6=helpers.covariance6_cpu(cloud).numpy()))
    return ref.Scene(cloud.xyz.numpy(), cloud.opacity.numpy(), cam.world_view_transform.numpy(), W, H,
                     math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), rows=rows, dtype=dtype, **kw)


@pytest.fixture(params=[1, 0], ids=["snug-box", "square"])
def tile_rect(request):
    import diff_gaussian_rasterization as dgr
    saved = dgr._TILE_RECT
    dgr._TILE_RECT = request.param
    yield request.param
    dgr._TILE_RECT = saved


@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_effective_opacity_against_the_float64_restatement(scale_mul):
    """Record word 5 of every Gaussian with radii > 0 against o' of tests/antialias_ref.py in float64.  Bound: 4 x the
    largest error of the same restatement in fp32 on the CPU (preprocess.hip is built without contraction, in the
    restatement's operation order).  Measured (o' <= 1: absolute figures): scale_mul 1.0: 2050 visible, fp32 CPU error
    8.62e-8, bound 3.45e-7, device error 8.62e-8; scale_mul 0.05: 2041 visible, median s 0.108, fp32 CPU error 3.99e-8,
    bound 1.60e-7, device error 3.99e-8 -- the device reproduces the fp32 restatement.  The Gaussian of scale 1e-6 is
    clamped: exactly o * 0.005f."""
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    st = _state(cloud, cam, dev, True)
    vis = st["radii"] > 0
    assert vis[CLAMP] and vis[BORDER] and not vis[BEHIND] and vis.sum() > 1500
    got = st["geom"]["rec"][:, 5].astype(np.float64)
    o64, s64, free64 = _ref_scene(cloud, cam, vis).effective_opacity()
    o32, _, _ = _ref_scene(cloud, cam, vis, dtype=torch.float32).effective_opacity()
    cpu_err = np.abs(o32 - o64)[vis].max()
    bound = 4.0 * cpu_err
    err = np.abs(got - o64)[vis].max()
    print("effective opacity scale_mul=%g: visible %d, s in [%.3g, %.3g], median %.3g; fp32 CPU error %.3g, bound %.3g, device "
          "error %.3g" % (scale_mul, vis.sum(), s64[vis].min(), s64[vis].max(), np.median(s64[vis]), cpu_err, bound, err))
    assert not free64[CLAMP] and free64[vis].sum() == vis.sum() - 1
    if scale_mul == 0.05:
        assert np.median(s64[vis]) < 0.5  # most footprints below a pixel
    assert cpu_err > 0 and err <= bound
    assert st["geom"]["rec"][CLAMP, 5] == np.float32(0.9) * np.float32(0.005)
    assert not st["geom"]["rec"][BEHIND, :9].any()  # (words 0..8: the splat; 9..11 are the binning's bookkeeping)


@pytest.mark.parametrize("cov_mode", ["scale_rot", "cov3d"])
@pytest.mark.parametrize("color_mode", ["sh", "precomp"])
@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_forward_is_bitwise_the_default_path_on_the_effective_opacities(tile_rect, scale_mul, color_mode, cov_mode):
    """antialiasing=True against antialiasing=False given opacities = o' (culled Gaussians keep o): image, radii,
    num_rendered, final_T, n_contrib and every splat record bit for bit, in both tile_rect modes.  (Fails where the
    settings tuple has no such field.)"""
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    on = _state(cloud, cam, dev, True, color_mode, cov_mode)
    o_eff = _effective(cloud, on)
    assert not torch.equal(o_eff, cloud.opacity)
    off = _state(cloud, cam, dev, False, color_mode, cov_mode, opacity=o_eff)
    plain = _state(cloud, cam, dev, False, color_mode, cov_mode)
    print("forward tile_rect=%d scale_mul=%g %s %s: num_rendered %d with the option, %d without"
          % (tile_rect, scale_mul, color_mode, cov_mode, on["D"], plain["D"]))
    assert on["D"] == off["D"] and on["D"] > 0
    assert np.array_equal(on["radii"], off["radii"]) and np.array_equal(on["radii"], plain["radii"])
    assert np.array_equal(on["color"].view(np.uint32), off["color"].view(np.uint32))
    assert np.array_equal(on["image"]["final_T"].view(np.uint32), off["image"]["final_T"].view(np.uint32))
    assert np.array_equal(on["image"]["n_contrib"], off["image"]["n_contrib"])
    assert np.array_equal(on["geom"]["rec"].view(np.uint32), off["geom"]["rec"].view(np.uint32))
    assert np.array_equal(on["geom"]["tiles_touched"], off["geom"]["tiles_touched"])
    assert not np.array_equal(on["color"], plain["color"])  # the option does something
    if tile_rect == 0:
        assert on["D"] == plain["D"]  # the 3-sigma square does not depend on the opacity
    else:
        assert on["D"] < plain["D"]


_BACKWARD_OF = {"plain": "gs_backward", "with-opacity": "gs_backward_with_opacity", "two-call": "gs_backward_with_second"}


def _leaves(kw):
    for k, t in kw.items():
        t.requires_grad_(True)
    return kw


def _run_backward(cloud, cam, dev, mode, antialiasing, color_mode, cov_mode, opacity, g_img, g_opa, settings_tail=None):
    """One forward + backward through the public surface; returns (images, {name: gradient})."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355.render import Pipe, render
    from gsplat_mi355.scenes import GaussianCloud
    dgr.release_shared_geometry()
    if mode == "two-call":
        pc = GaussianCloud(cloud.xyz.to(dev), cloud.scales.to(dev), cloud.rotations.to(dev), opacity.to(dev),
                           cloud.shs.to(dev), cloud.sh_degree)
        names = dict(means3D=pc.xyz, opacities=pc.opacity, scales=pc.scales, rotations=pc.rotations, shs=pc.shs)
        _leaves(names)
        hits0 = dgr._geom_cache.hits
        pkg = render(cam.to(dev), pc, Pipe(antialiasing=antialiasing), torch.zeros(3, device=dev), return_opacity=True)
        cam.to("cpu")
        assert dgr._geom_cache.hits - hits0 == 1  # the opacity pass was served from the colour pass's geometry
        ((pkg.render * g_img.to(dev)).sum() + (pkg.opacity_render * g_opa.to(dev)).sum()).backward()
        names["means2D"] = pkg.viewspace_points
        images = (pkg.render.detach(), pkg.opacity_render.detach())
    else:
        tail = (antialiasing,) if settings_tail is None else settings_tail
        rast = dgr.GaussianRasterizer(_settings(cam, dev, *tail, sh_degree=cloud.sh_degree))
        names = _leaves(_inputs(cloud, cam, dev, color_mode, cov_mode, opacity))
        names["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)
        if mode == "with-opacity":
            color, radii, opa = rast(with_opacity=True, **names)
            ((color * g_img.to(dev)).sum() + (opa * g_opa.to(dev)).sum()).backward()
            images = (color.detach(), opa.detach())
        else:
            color, radii = rast(**names)
            (color * g_img.to(dev)).sum().backward()
            images = (color.detach(),)
    torch.cuda.synchronize()
    return images, {k: t.grad.detach().cpu().numpy().astype(np.float64).reshape(t.shape[0], -1) for k, t in names.items()}


_CHAIN = {"means3D": "means3D", "scales": "scales", "rotations": "rotations", "cov3D_precomp": "cov3D"}


@pytest.mark.parametrize("mode,color_mode,cov_mode", [("plain", "sh", "scale_rot"), ("plain", "precomp", "cov3d"),
                                                      ("with-opacity", "precomp", "scale_rot"), ("two-call", "sh", "scale_rot")])
@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_backward_is_the_default_path_plus_the_chain_through_the_scaling(monkeypatch, scale_mul, mode, color_mode, cov_mode):
    """Gradients with the option against g' = the gradients of the default path at opacities o' (random dL_dpix):
    dL/do = s g'_o; means3D and cov3D (or scales, rotations) = g' + the chain term of tests/antialias_ref.py in float64
    given gO = g'_o; colours / SH and means2D = g'.  Through gs_backward ("plain"), gs_backward_with_opacity and render()'s
    two rasterizer calls with the fused second backward (gs_backward_with_second).
    Bounds: shared parts 1e-5 max|g| per tensor; tensors with an added term the larger of that and 4 x the error of the
    fp32 CPU restatement of the term on this cloud.  Measured: 4 x the fp32 CPU error stays below the parity bar in every
    case, which therefore is the bound; e.g. plain / SH / scale + rotation at scale_mul 0.05: means3D max|g| 18.7, added
    term up to 0.269, fp32 CPU error 6.5e-8, bound 1.87e-4, device error 1.14e-6; scales 31.4, 33.3, 9.8e-6, 3.14e-4,
    6.5e-6; rotations 0.934, 0.886, 2.3e-7, 9.3e-6, 5.5e-7; opacities 1.53, 3.7, 2.2e-7, 1.53e-5, 1.7e-7; cov3D
    (precomputed) 2.69e3, 2.57e3, 5.4e-4, 2.69e-2, 5.2e-4.  Colours / SH and means2D: error 0.
    Also here (the same runs): the clamped Gaussian's added terms are exactly zero (its rows are g' bit for bit and
    dL/do = 0.005f g'_o), culled Gaussians get all-zero rows."""
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    on_state = _state(cloud, cam, dev, True, color_mode if mode != "two-call" else "sh", cov_mode)
    vis = on_state["radii"] > 0
    o_eff = _effective(cloud, on_state)
    gen = torch.Generator().manual_seed(21)
    g_img, g_opa = torch.randn(3, H, W, generator=gen), torch.randn(1, H, W, generator=gen)
    img_off, gp = _run_backward(cloud, cam, dev, mode, False, color_mode, cov_mode, o_eff, g_img, g_opa)
    from gsplat_mi355 import _lib
    counter = _CallCounter(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counter)
    img_on, got = _run_backward(cloud, cam, dev, mode, True, color_mode, cov_mode, cloud.opacity, g_img, g_opa)
    monkeypatch.undo()
    assert {k: counter.calls[k] for k in _BACKWARD_OF.values() if counter.calls[k]} == {_BACKWARD_OF[mode]: 1}, counter.calls
    for x, y in zip(img_on, img_off):
        assert torch.equal(x, y)
    gO = gp["opacities"][:, 0]
    assert np.abs(gO[vis]).max() > 0 and gO[CLAMP] != 0
    r64, r32 = _ref_scene(cloud, cam, vis, cov_mode), _ref_scene(cloud, cam, vis, cov_mode, dtype=torch.float32)
    _, s64, _ = r64.effective_opacity()
    _, s32, _ = r32.effective_opacity()
    chain64, chain32 = r64.chain(gO), r32.chain(gO)
    for name in got:
        g_ref = gp[name]
        bar = PARITY * np.abs(got[name]).max()
        if name == "opacities":
            want, cpu_err = s64[:, None] * g_ref, np.abs((s32 - s64) * gO).max()
        elif name in _CHAIN:
            add64, add32 = chain64[_CHAIN[name]], chain32[_CHAIN[name]]
            assert np.abs(add64).max() > 0
            want, cpu_err = g_ref + add64, np.abs(add32 - add64).max()
        else:
            want, cpu_err = g_ref, 0.0
        bound = max(bar, 4.0 * cpu_err)
        err = np.abs(got[name] - want).max()
        print("backward scale_mul=%g %s %s %s %-14s max|g| %.3g, added term max %.3g, fp32 CPU error %.3g, bound %.3g, error %.3g"
              % (scale_mul, mode, color_mode, cov_mode, name, np.abs(got[name]).max(),
                 np.abs(want - g_ref).max(), cpu_err, bound, err))
        assert np.isfinite(got[name]).all() and err <= bound, name
        # the clamped Gaussian: nothing added; culled Gaussians: zero rows
        if name == "opacities":
            assert np.float32(got[name][CLAMP, 0]) == np.float32(0.005) * np.float32(g_ref[CLAMP, 0])
        else:
            assert np.array_equal(got[name][CLAMP], g_ref[CLAMP]), name
        assert not got[name][~vis].any(), name


def test_nothing_is_non_finite_on_needles():
    """helpers.needle_cloud_and_camera: det0 = a0 c0 - b^2 cancels (and is rounded to zero or below for some): the image
    and every gradient stay finite with the option."""
    dev = torch.device("cuda:0")
    cloud, cam = helpers.needle_cloud_and_camera(1500, W, H, seed=3)
    gen = torch.Generator().manual_seed(2)
    g_img = torch.randn(3, H, W, generator=gen)
    for cov_mode in ("scale_rot", "cov3d"):
        images, grads = _run_backward(cloud, cam, dev, "plain", True, "sh", cov_mode, cloud.opacity, g_img, None)
        assert bool(torch.isfinite(images[0]).all())
        for name, g in grads.items():
            assert np.isfinite(g).all(), (cov_mode, name)
        assert np.abs(grads["means3D"]).max() > 0
    st = _state(cloud, cam, dev, True)
    vis = st["radii"] > 0
    o_dev = st["geom"]["rec"][vis, 5]
    print("needles: visible %d, o'/o in [%.3g, %.3g]" % (vis.sum(), (o_dev / cloud.opacity.numpy()[vis, 0]).min(),
                                                        (o_dev / cloud.opacity.numpy()[vis, 0]).max()))
    assert np.isfinite(o_dev).all() and (o_dev >= 0).all() and (o_dev <= cloud.opacity.numpy()[vis, 0] * (1 + 1e-6)).all()


def test_explicit_false_is_the_twelve_field_default_bit_for_bit():
    dev = torch.device("cuda:0")
    cloud, cam = _scene(0.05)
    gen = torch.Generator().manual_seed(5)
    g_img, g_opa = torch.randn(3, H, W, generator=gen), torch.randn(1, H, W, generator=gen)
    for mode in ("plain", "with-opacity"):
        i12, g12 = _run_backward(cloud, cam, dev, mode, None, "sh", "scale_rot", cloud.opacity, g_img, g_opa, settings_tail=())
        i13, g13 = _run_backward(cloud, cam, dev, mode, None, "sh", "scale_rot", cloud.opacity, g_img, g_opa, settings_tail=(False,))
        for x, y in zip(i12, i13):
            assert torch.equal(x, y)
        for name in g12:
            assert np.array_equal(g12[name], g13[name]), name


def test_geometry_is_never_shared_across_the_flag():
    """Same tensor objects, option on then off (and off then on) in consecutive calls: the second call is not served from
    the first call's geometry and equals a fresh stand-alone render."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    cloud, cam = _scene(0.05)
    kw = _leaves(_inputs(cloud, cam, dev, "precomp", "scale_rot"))
    kw["colors_precomp"].requires_grad_(False)
    kw["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)
    base = _settings(cam, dev)  # ONE set of camera tensors: only the flag differs between the calls
    fresh = {}
    for flag in (False, True):
        dgr.release_shared_geometry()
        fresh[flag] = dgr.GaussianRasterizer(base._replace(antialiasing=flag))(**kw)[0].detach().clone()
    assert not torch.equal(fresh[False], fresh[True])
    for first in (True, False):
        dgr.release_shared_geometry()
        hits0 = dgr._geom_cache.hits
        a = dgr.GaussianRasterizer(base._replace(antialiasing=first))(**kw)[0]
        b = dgr.GaussianRasterizer(base._replace(antialiasing=not first))(**kw)[0]
        assert dgr._geom_cache.hits == hits0
        assert torch.equal(a.detach(), fresh[first]) and torch.equal(b.detach(), fresh[not first])
        # (the same flag twice IS shared: the key differs in nothing else)
        dgr.release_shared_geometry()
        a = dgr.GaussianRasterizer(base._replace(antialiasing=first))(**kw)[0]
        c = dgr.GaussianRasterizer(base._replace(antialiasing=first))(**kw)[0]
        assert dgr._geom_cache.hits == hits0 + 1 and torch.equal(c.detach(), fresh[first])
    dgr.release_shared_geometry()


def test_opacity_pass_of_render_equals_a_stand_alone_second_call():
    """render(return_opacity=True) with the option: the opacity pass, served from the colour pass's records (1 - T of the
    effective opacities), against a stand-alone rasterizer call with colours = 1 and the option.  The shared pass writes
    1 - T, the stand-alone call composites sum(alpha T): equal to fp32 rounding, one rounding of T per contributor and one
    of the sum: (max n_contrib + 2) 2^-23."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355.render import Pipe, render
    from gsplat_mi355.scenes import GaussianCloud
    dev = torch.device("cuda:0")
    for scale_mul in (1.0, 0.05):
        cloud, cam = _scene(scale_mul)
        pc = GaussianCloud(cloud.xyz.to(dev), cloud.scales.to(dev), cloud.rotations.to(dev), cloud.opacity.to(dev),
                           cloud.shs.to(dev), cloud.sh_degree)
        pc.xyz.requires_grad_(True)
        dgr.release_shared_geometry()
        hits0 = dgr._geom_cache.hits
        pkg = render(cam.to(dev), pc, Pipe(antialiasing=True), torch.zeros(3, device=dev), return_opacity=True)
        cam.to("cpu")
        assert dgr._geom_cache.hits == hits0 + 1
        dgr.release_shared_geometry()
        ones = torch.ones(cloud.xyz.shape[0], 3, device=dev)
        with torch.no_grad():
            alone, _ = dgr.GaussianRasterizer(_settings(cam, dev, True))(
                means3D=pc.xyz, means2D=torch.zeros_like(pc.xyz), opacities=pc.opacity, colors_precomp=ones, scales=pc.scales,
                rotations=pc.rotations)
            plain, _ = dgr.GaussianRasterizer(_settings(cam, dev, False))(
                means3D=pc.xyz, means2D=torch.zeros_like(pc.xyz), opacities=pc.opacity, colors_precomp=ones, scales=pc.scales,
                rotations=pc.rotations)
        st = _state(cloud, cam, dev, True)
        assert np.array_equal(st["color"], pkg.render.detach().cpu().numpy())  # the colour pass: the option's own image
        bound = (int(st["image"]["n_contrib"].max()) + 2) * 2.0 ** -23
        err = float((pkg.opacity_render.detach() - alone[:1]).abs().max())
        gap = float((alone - plain).abs().max())
        print("opacity pass scale_mul=%g: error %.3g, bound %.3g; the option moves the opacity image by up to %.3g" % (scale_mul, err, bound, gap))
        assert err <= bound and gap > 100 * bound


def test_training_step_with_the_option_replays_bit_identically_from_a_graph():
    """Forward, L1 loss, backward with the option captured by torch.cuda.graph (the pattern of test_gpu_capture.py): the
    replay's loss and gradients are the eager step's, bit for bit."""
    from gsplat_mi355.camera import orbit_camera
    from gsplat_mi355.render import Pipe, l1_loss, render
    from gsplat_mi355.scenes import GaussianCloud
    dev = torch.device("cuda:0")
    cloud, _ = _scene(0.05)
    cam_d = orbit_camera(0, W, H, device=dev)
    bg = torch.zeros(3, device=dev)
    pipe = Pipe(antialiasing=True)
    side = torch.cuda.Stream(dev)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)

    def fresh():
        c = GaussianCloud(cloud.xyz.to(dev), cloud.scales.to(dev), cloud.rotations.to(dev), cloud.opacity.to(dev),
                          cloud.shs.to(dev), cloud.sh_degree)
        leaves = [c.xyz, c.opacity, c.scales, c.rotations, c.shs]
        for t in leaves:
            t.requires_grad_(True)
        return c, leaves

    def step(c):
        pkg = render(cam_d, c, pipe, bg)
        loss = l1_loss(pkg.render, gt)
        loss.backward()
        return loss, pkg.viewspace_points

    ce, le = fresh()
    loss_e, vp_e = step(ce)
    torch.cuda.synchronize()
    want = [t.grad.clone() for t in le] + [vp_e.grad.clone()]
    with torch.no_grad():  # the option is on in the step
        assert not torch.equal(render(cam_d, ce, Pipe(), bg).render, render(cam_d, ce, pipe, bg).render)
    cg, lg = fresh()
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            for t in lg:
                t.grad = None
            step(cg)
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    for t in lg:
        t.grad = None
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        loss_g, vp_g = step(cg)
    for _ in range(2):
        g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for k, (x, y) in enumerate(zip([t.grad for t in lg] + [vp_g.grad], want)):
        assert torch.equal(x, y), k
