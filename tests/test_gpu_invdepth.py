"""The rasterizer's inverse-depth image on the device (`with_invdepth=True`: invdepth = sum alpha T / z, differentiated in
the colour image's backward pass; the second image's colour gradient comes from csrc/second_colors.hip).

Scenes: the two clouds of tests/test_gpu_antialiasing.py -- helpers.cloud_and_camera(2048, 96, 80, seed=4) with scale_mul
1.0 and 0.05, each joined by its three hand-placed Gaussians (clamped, at the border, behind the near plane): six tiles
by five, neither image side a multiple of 16, 2051 Gaussians.  At scale 1.0 the tile lists are longer than the kernel's
staging batch of 256 entries (asserted) and pixels stop early on T < 1e-4; at 0.05 most pixels are empty and some
Gaussians touch no tile.  Images of up to 2048 tiles take the kernel's chunked walk (16 chunks per tile at scale 1.0, 8
at 0.05, where the workspace is smaller), one staging batch per chunk; a 40 x 40 scene with lists of ~9900 entries walks
three batches per chunk; a 784 x 776 scene takes the whole-list walk.  A frame whose pair count exceeds the declared
capacity (a replayed graph on a scene that has grown) is checked through the C ABI.

References: "formulation C" = what a caller had to write before the option existed, on the device -- a second rasterizer
call with colors_precomp = 1/z requiring a gradient (shared forward, a backward of its own); gs_oracle.backward of the
1/z-coloured scene; float64 autograd of oracle/dense_ref.py.  Bar: the project's parity bar, |delta| <= 1e-5 max|g| per
tensor (README).  Where the new kernel is compared, a Gaussian over the bar may be set aside only if the float64
reference shows one of its pairs within relative 1e-4 of a threshold decision (alpha = 1/255, T (1 - alpha) = 1e-4) at a
pixel with a non-zero gradient, and at most 2 % of the visible Gaussians may be.  Every test prints the figures it asserts.

Measured on an MI355X: the float64 reference finds 34 undecided pairs of 3.7 M tested at scale 1.0 (on 33 Gaussians), none
at 0.05, 16 of 0.8 M on the 512-Gaussian scene; no Gaussian had to be set aside anywhere.  Largest errors, as shares of the
tensor maximum: dL_dcolors2 2.7e-7 against two calls and 2.1e-7 against the oracle, means3D 2.8e-8 and 6.0e-7, the
geometry gradients against two calls up to 4.0e-7, every gradient against float64 autograd up to 9.5e-7, the image against
float64 up to 9.6e-7 absolute; the long-chunk scene against two calls up to 3.8e-7."""
import functools
import math

import numpy as np
import pytest
import torch

import helpers
from helpers import _CallCounter
from test_gpu_antialiasing import BEHIND, BORDER, CLAMP, H, W, _inputs, _scene, tile_rect  # noqa: F401

pytestmark = pytest.mark.gpu

PARITY = 1e-5   # |delta| <= 1e-5 max|g| per tensor: the project's parity bar (README)
BATCH = 256     # SC_BATCH of csrc/second_colors.hip: list entries staged per trip
NEAR = helpers.NEAR  # relative distance from a threshold decision within which the float64 reference calls a pair undecided


def _settings(cam, dev, *tail, sh_degree=3):
    """(as tests/test_gpu_antialiasing.py's, for a camera of any image size)"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
        cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), sh_degree, cam.camera_center.to(dev), False, False, *tail)


def _depths(cloud, cam, dev):
    """(z [P] as the device stored it, radii, state) of the cloud's forward."""
    from gsplat_mi355 import debug
    kw = _inputs(cloud, cam, dev, "sh", "scale_rot")
    st = debug.forward_state(_settings(cam, dev, sh_degree=cloud.sh_degree), kw.pop("means3D"), kw.pop("opacities"), **kw)
    return torch.from_numpy(st["geom"]["depths"]).to(dev), torch.from_numpy(st["radii"]).to(dev), st


def _inv_colors(z, radii):
    inv = torch.where(radii > 0, 1.0 / z, torch.zeros((), device=z.device))
    return inv.unsqueeze(1).expand(-1, 3).contiguous()


def _leaves(kw):
    for t in kw.values():
        t.requires_grad_(True)
    return kw


def _grads(names):
    return {k: t.grad.detach().clone() for k, t in names.items() if t.grad is not None}  # (no gradient: not used by the loss)


def _one_pass(cloud, cam, dev, gC, gD, color_mode="sh", cov_mode="scale_rot", antialiasing=False, hook=None, l1_target=None):
    """The option: (color, invdepth), gradients by name (+ "colors2" = dL_dcolors of the second image, from the hook).
    `l1_target`: the call also carries the fused L1 loss, added to the loss as it is."""
    import diff_gaussian_rasterization as dgr
    dgr.release_shared_geometry()
    rast = dgr.GaussianRasterizer(_settings(cam, dev, antialiasing, sh_degree=cloud.sh_degree))
    names = _leaves(_inputs(cloud, cam, dev, color_mode, cov_mode))
    names["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)
    if l1_target is None:
        (color, radii, inv), loss = rast(with_invdepth=True, **names), 0.0
    else:
        color, radii, inv, loss = rast(with_invdepth=True, l1_target=l1_target.to(dev), **names)
    assert tuple(inv.shape) == (1, cam.image_height, cam.image_width)
    if gC is not None:
        loss = loss + (color * gC.to(dev)).sum()
    if gD is not None:
        loss = loss + (inv * gD.to(dev)).sum()
    from gsplat_mi355 import debug
    seen = []
    debug.second_colors_hook = (lambda t: seen.append(t.detach().clone()))
    try:
        loss.backward()
    finally:
        debug.second_colors_hook = None
    torch.cuda.synchronize()
    g = _grads(names)
    if seen:
        g["colors2"] = seen[0]
    return (color.detach(), inv.detach(), radii), g


def _formulation_c(cloud, cam, dev, gC, gD, color_mode="sh", cov_mode="scale_rot", antialiasing=False, l1_target=None):
    """Two rasterizer calls: colour, then colors_precomp = 1/z requiring a gradient (values: the device's own depths, bit
    for bit; gradient: through z = means3D . V[:3, 2] + V[3, 2]).  `l1_target`: the colour call carries the fused L1 loss."""
    import diff_gaussian_rasterization as dgr
    dgr.release_shared_geometry()
    z_dev, radii_dev, _ = _depths(cloud, cam, dev)
    rast = dgr.GaussianRasterizer(_settings(cam, dev, antialiasing, sh_degree=cloud.sh_degree))
    names = _leaves(_inputs(cloud, cam, dev, color_mode, cov_mode))
    names["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)
    V = cam.world_view_transform.to(dev)
    hits0 = dgr._geom_cache.hits
    l1 = 0.0
    if l1_target is None:
        color, radii = rast(**names)
    else:
        color, radii, l1 = rast(l1_target=l1_target.to(dev), **names)
    zt = names["means3D"] @ V[:3, 2] + V[3, 2]
    soft = torch.where(radii > 0, 1.0 / zt, torch.zeros((), device=dev))
    exact = _inv_colors(z_dev, radii_dev)
    cols2 = (exact + (soft - soft.detach()).unsqueeze(1)).contiguous()   # the stored depths' values, z's gradient
    cols2.retain_grad()
    second = {k: v for k, v in names.items() if k not in ("shs", "colors_precomp")}
    img2, _ = rast(colors_precomp=cols2, **second)
    assert dgr._geom_cache.hits - hits0 == 1  # (shared forward)
    loss = (img2[:1] * gD.to(dev)).sum() + l1
    if gC is not None:
        loss = loss + (color * gC.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = _grads(names)
    g["colors2"] = cols2.grad.detach().clone()
    return (color.detach(), img2.detach()), g


@functools.lru_cache(maxsize=None)
def _float64(scale_mul, n=None, seed=None, WH=None, frame=0):
    """One dense float64 pass (oracle/dense_ref.py) over the scene with colours 1/z, bg = 0: the inverse-depth image, and per
    Gaussian whether one of its (pixel, Gaussian) pairs lies within relative NEAR of alpha = 1/255 or of T (1 - alpha) =
    1e-4 before the pixel is done; + the counts (undecided pairs, pairs tested against alpha = 1/255) and the visible mask."""
    from oracle import dense_ref
    if n is None:
        cloud, cam = _scene(scale_mul)
        w, h = W, H
    else:
        w, h = WH
        cloud, cam = helpers.cloud_and_camera(n, w, h, sh_degree=0, seed=seed, frame=frame)
    dt = torch.float64
    P = cloud.xyz.shape[0]
    with torch.no_grad():
        V = cam.world_view_transform.to(dt)
        z64 = cloud.xyz.to(dt) @ V[:3, 2] + V[3, 2]
        c64 = torch.where(z64 > 0.2, 1.0 / z64, torch.zeros_like(z64))[:, None].expand(P, 3)
        img, radii, aux = dense_ref.render(w, h, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, dtype=dt), V,
                                           cam.full_proj_transform.to(dt), cam.camera_center.to(dt), cloud.xyz.to(dt),
                                           torch.zeros(P, 3, dtype=dt), cloud.opacity.to(dt), colors_precomp=c64,
                                           scales=cloud.scales.to(dt), rotations=cloud.rotations.to(dt))
    u = helpers.undecided_pairs(aux, w, h)   # (alpha from aux["o_eff"]: here the opacities themselves)
    return dict(image=img[0].clone(), visible=(radii > 0).numpy(), **u)


def _assert_bar(name, got, want, setaside=None, cap=None):
    """Every row within PARITY * max|want| -- except rows of `setaside` Gaussians, of which at most `cap` may be over."""
    got = np.asarray(got, np.float64).reshape(want.shape[0], -1)
    want = np.asarray(want, np.float64).reshape(want.shape[0], -1)
    m = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max(1) / m
    over = err > PARITY
    n_aside = int((over & setaside).sum()) if setaside is not None else 0
    unexplained = over & ~setaside if setaside is not None else over
    print("%s: max|g| %.4g, largest error %.3g of it, rows over the bar %d, of them set aside %d (cap %s)"
          % (name, m, err.max(), int(over.sum()), n_aside, cap))
    assert not unexplained.any(), (name, np.nonzero(unexplained)[0][:8], err[unexplained][:8])
    if setaside is not None:
        assert n_aside <= cap, (name, n_aside, cap)


def _g(seed=31, w=W, h=H):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(3, h, w, generator=gen), torch.randn(1, h, w, generator=gen)


@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_image_is_the_stand_alone_render_of_inverse_depths(tile_rect, scale_mul, antialiasing):
    """invdepth == channel 0 of a stand-alone call with colors_precomp = 1/z, bg = 0 (torch.equal: the recolour is
    documented as same bits), also under antialiasing; against oracle/dense_ref.py in float64 within 1e-5 (the bound
    tests/test_gpu_parity.py puts on the colour image); empty pixels exactly 0.  The colour image and radii are those of a
    call without the flag, bit for bit."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    z, radii0, st = _depths(cloud, cam, dev)
    lens = st["image"]["ranges"][:, 1].astype(np.int64) - st["image"]["ranges"][:, 0]
    print("scale_mul %g tile_rect %d: longest tile list %d, num_rendered %d, empty pixels %d, culled %d"
          % (scale_mul, tile_rect, lens.max(), st["D"], int((st["image"]["n_contrib"] == 0).sum()), int((st["radii"] == 0).sum())))
    if scale_mul == 1.0:
        assert lens.max() > BATCH  # more than one staging batch
    else:
        assert (st["image"]["n_contrib"] == 0).sum() > 1000
    rast = dgr.GaussianRasterizer(_settings(cam, dev, antialiasing, sh_degree=cloud.sh_degree))
    with torch.no_grad():
        kw = _inputs(cloud, cam, dev, "sh", "scale_rot")
        m2d = torch.zeros(cloud.xyz.shape[0], 3, device=dev)
        color, radii, inv = rast(means2D=m2d, with_invdepth=True, **kw)
        plain, radii_p = rast(means2D=m2d, **kw)
        geo = {k: v for k, v in kw.items() if k != "shs"}
        alone, _ = rast(means2D=m2d, colors_precomp=_inv_colors(z, radii0), **geo)
    torch.cuda.synchronize()
    assert torch.equal(radii.cpu(), radii0.cpu()) and torch.equal(radii, radii_p) and torch.equal(color, plain)
    assert radii[CLAMP] > 0 and radii[BORDER] > 0 and radii[BEHIND] == 0
    assert torch.equal(inv[0], alone[0]) and torch.equal(alone[0], alone[1])
    empty = torch.from_numpy(st["image"]["n_contrib"] == 0).to(dev)
    if not antialiasing:
        assert not inv[0][empty].any()
        f64 = _float64(scale_mul)
        ref = f64["image"]
        print("float64: %d empty pixels, %d pixels stop early on T < 1e-4" % (int(f64["empty"].sum()), f64["early"]))
        assert not inv[0].cpu()[f64["empty"]].any()
        err = float((inv[0].cpu().double() - ref).abs().max())
        print("invdepth against float64: max |delta| %.3g (max value %.3g)" % (err, float(ref.max())))
        assert err < 1e-5


@pytest.mark.parametrize("color_mode,cov_mode", [("sh", "scale_rot"), ("precomp", "cov3d")])
@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_geometry_gradients_against_two_calls_and_colour_gradients_bit_for_bit(tile_rect, scale_mul, color_mode, cov_mode):
    """Random gC (3, H, W) and gD (1, H, W).  means2D, opacities and the covariance inputs of the one-pass call against
    formulation C on the device, at the parity bar, no exclusions (both sides take their decisions in render_bwd); the
    colour image's own dL_dcolors / dL_dsh bit for bit those of a call without the flag given the same gC."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    gC, gD = _g()
    _, one = _one_pass(cloud, cam, dev, gC, gD, color_mode, cov_mode)
    _, two = _formulation_c(cloud, cam, dev, gC, gD, color_mode, cov_mode)
    cov_names = ("scales", "rotations") if cov_mode == "scale_rot" else ("cov3D_precomp",)
    for k in ("means2D", "opacities") + cov_names:
        _assert_bar("%s (scale_mul %g, %s, %s)" % (k, scale_mul, color_mode, cov_mode), one[k].cpu().numpy(), two[k].cpu().numpy())
    # the colour image's own colour gradient: a call without the flag
    dgr.release_shared_geometry()
    rast = dgr.GaussianRasterizer(_settings(cam, dev, sh_degree=cloud.sh_degree))
    names = _leaves(_inputs(cloud, cam, dev, color_mode, cov_mode))
    names["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)
    color, _ = rast(**names)
    (color * gC.to(dev)).sum().backward()
    torch.cuda.synchronize()
    ck = "shs" if color_mode == "sh" else "colors_precomp"
    assert torch.equal(one[ck], names[ck].grad)


@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_second_image_colour_gradient_and_means3d_against_two_calls_and_the_oracle(oracle, tile_rect, scale_mul):
    """The new kernel: dL_dcolors of the inverse-depth render (debug hook) and the full means3D gradient against
    formulation C on the device and against gs_oracle.backward of the 1/z-coloured scene (its means3D + the chain through
    z formed in float64 from its own colour gradient), at the parity bar, with the attribution rule of the module
    docstring."""
    dev = torch.device("cuda:0")
    cloud, cam = _scene(scale_mul)
    f64 = _float64(scale_mul)
    flag, n_near, n_pairs, vis = f64["flag"], f64["near"], f64["met"], f64["visible"]
    cap = int(0.02 * vis.sum())
    print("float64 reference, scale_mul %g: %d undecided pairs of %d tested, on %d Gaussians (cap %d of %d visible)"
          % (scale_mul, n_near, n_pairs, int(flag.sum()), cap, int(vis.sum())))
    gC, gD = _g()
    _, one = _one_pass(cloud, cam, dev, None, gD)
    _, two = _formulation_c(cloud, cam, dev, None, gD)
    tag = " (scale_mul %g, tile_rect %d)" % (scale_mul, tile_rect)
    _assert_bar("dL_dcolors2 vs two calls" + tag, one["colors2"].cpu().numpy(), two["colors2"].cpu().numpy(), flag, cap)
    _assert_bar("means3D vs two calls" + tag, one["means3D"].cpu().numpy(), two["means3D"].cpu().numpy(), flag, cap)
    # the C oracle on the 1/z-coloured scene (colours: the device's stored depths, so that both walk the same numbers)
    z, radii0, _ = _depths(cloud, cam, dev)
    cols = _inv_colors(z, radii0).cpu()
    sc = helpers.oracle_scene(cloud, cam, color_mode="precomp", colors=cols)
    fw = oracle.forward(sc)
    g3 = np.zeros((3, H, W), np.float32)
    g3[0] = gD[0].numpy()
    b = oracle.backward(sc, fw, g3)
    V = cam.world_view_transform.numpy().astype(np.float64)
    zz = z.cpu().numpy().astype(np.float64)
    inv2 = np.where(fw["radii"] > 0, 1.0 / np.maximum(zz, 1e-30) ** 2, 0.0)
    want3 = b["means3D"].astype(np.float64) - (b["colors_precomp"].astype(np.float64).sum(1) * inv2)[:, None] * V[:3, 2][None]
    _assert_bar("dL_dcolors2 vs the oracle" + tag, one["colors2"].cpu().numpy(), b["colors_precomp"], flag, cap)
    _assert_bar("means3D vs the oracle" + tag, one["means3D"].cpu().numpy(), want3, flag, cap)
    # culled Gaussians: exact zeros
    assert not one["colors2"][BEHIND].any() and not one["means3D"][BEHIND].any()


def test_whole_list_walk_on_an_image_of_more_than_2048_tiles():
    """Images of up to 2048 tiles (every other scene of this file) cut the tile lists into chunks that start from
    transmittance products; larger ones walk whole lists, one workgroup per tile.  4000 Gaussians on 784 x 776 (49 x 49 =
    2401 tiles, neither side a multiple of 16): the image against the stand-alone render bit for bit, dL_dcolors2 and every
    gradient against formulation C on the device at the parity bar, no exclusions (no float64 reference at this size: both
    sides evaluate alpha with the same expression)."""
    dev = torch.device("cuda:0")
    w, h = 784, 776
    cloud, cam = helpers.cloud_and_camera(4000, w, h, sh_degree=1, seed=6, scale_mul=2.0)
    assert ((w + 15) // 16) * ((h + 15) // 16) > 2048
    gC, gD = _g(17, w, h)
    (color, inv, radii), one = _one_pass(cloud, cam, dev, gC, gD)
    (color_c, img2), two = _formulation_c(cloud, cam, dev, gC, gD)
    _, _, st = _depths(cloud, cam, dev)
    lens = st["image"]["ranges"][:, 1].astype(np.int64) - st["image"]["ranges"][:, 0]
    print("784 x 776: num_rendered %d, longest tile list %d, visible %d" % (st["D"], lens.max(), int((radii > 0).sum())))
    assert lens.max() > BATCH and int((radii > 0).sum()) > 3000
    assert torch.equal(color, color_c) and torch.equal(inv[0], img2[0])
    for k in ("colors2", "means3D", "means2D", "opacities", "scales", "rotations"):
        _assert_bar("whole lists: " + k, one[k].cpu().numpy(), two[k].cpu().numpy())


def test_chunked_walk_with_several_staging_batches_per_chunk():
    """A small image whose tile lists exceed 16 x 256 entries: 20000 Gaussians of four times the usual size and 0.08 of the
    usual opacity on 40 x 40 (nine tiles; lists of up to ~9900 entries, pixels with up to ~9900 contributors, a few of which
    stop on T < 1e-4), so that each of the 16 chunks of a list is walked in several staging batches and starts from the
    product of up to 15 chunk products.  Image against the stand-alone render bit for bit; dL_dcolors2 and every gradient
    against formulation C on the device at the parity bar, no exclusions."""
    dev = torch.device("cuda:0")
    w, h = 40, 40
    cloud, cam = helpers.cloud_and_camera(20000, w, h, sh_degree=1, seed=8, scale_mul=4.0)
    cloud.opacity = cloud.opacity * 0.08
    gC, gD = _g(19, w, h)
    (color, inv, radii), one = _one_pass(cloud, cam, dev, gC, gD)
    (color_c, img2), two = _formulation_c(cloud, cam, dev, gC, gD)
    _, _, st = _depths(cloud, cam, dev)
    lens = st["image"]["ranges"][:, 1].astype(np.int64) - st["image"]["ranges"][:, 0]
    print("40 x 40: num_rendered %d, longest tile list %d, most contributors of a pixel %d, smallest final T %.3g"
          % (st["D"], lens.max(), st["image"]["n_contrib"].max(), st["image"]["final_T"].min()))
    assert lens.max() > 2 * 16 * BATCH and st["image"]["n_contrib"].max() > 2 * 16 * BATCH
    assert torch.equal(color, color_c) and torch.equal(inv[0], img2[0])
    for k in ("colors2", "means3D", "means2D", "opacities", "scales", "rotations"):
        _assert_bar("long chunks: " + k, one[k].cpu().numpy(), two[k].cpu().numpy())


def test_a_frame_that_outgrew_its_capacity_gets_zero_colour_gradients():
    """A captured graph replayed on a scene whose pair count exceeds the capacity it was captured with renders an EMPTY frame
    (the kernels read the count on the device): no tile list, so the tile walk writes no row, while the records still number
    the real scene's pairs.  dL_dcolors of the second image must then be zeros, not sums over whatever the scratch held.
    Through the C ABI: the two-phase forward at a capacity of 1024 pairs against a frame of ~10000, the shared render, then
    gs_backward_with_second with dL_dcolors on a scratch filled with NaN patterns.  (The binning state and the scratch are
    ALLOCATED for the real count and only declared as 1024 pairs, so that nothing any kernel of the backward derives from the
    records' pair numbers can point outside them.)"""
    import ctypes
    from diff_gaussian_rasterization import _make_args
    from gsplat_mi355 import _lib
    dev = torch.device("cuda:0")
    cloud, cam = _scene(1.0)
    P = cloud.xyz.shape[0]
    kw = _inputs(cloud, cam, dev, "sh", "scale_rot")
    L = _lib.load()
    keep = []
    with torch.cuda.device(dev):
        a = _make_args(_settings(cam, dev, sh_degree=cloud.sh_degree), kw["means3D"], kw["shs"], None, kw["opacities"], kw["scales"],
                       kw["rotations"], None, keep)
        a.frame_stats = None
        sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        gb, ib = _lib.nbytes(L.gs_geom_bytes, P), _lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a))
        geom, geom2 = (torch.zeros(gb, dtype=torch.uint8, device=dev) for _ in range(2))
        img, img2 = (torch.zeros(ib, dtype=torch.uint8, device=dev) for _ in range(2))
        radii = torch.zeros(P, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64).pin_memory()
        _lib.check(L.gs_forward_preprocess(ctypes.byref(a), geom.data_ptr(), gb, img.data_ptr(), ib, radii.data_ptr(), count.data_ptr(), sptr))
        torch.cuda.synchronize()
        real, cap = int(count.item()), 1024
        assert real > 8 * cap
        bb, sb = _lib.nbytes(L.gs_binning_bytes, cap, W, H), _lib.nbytes(L.gs_backward_scratch_bytes, cap, P, W, H)
        binning = torch.full((_lib.nbytes(L.gs_binning_bytes, real, W, H),), 0xFF, dtype=torch.uint8, device=dev)
        scratch = torch.full((_lib.nbytes(L.gs_backward_scratch_bytes, real, P, W, H),), 0xFF, dtype=torch.uint8, device=dev)  # NaNs
        assert bb <= binning.numel() and sb <= scratch.numel()
        color, color2 = torch.full((3, H, W), 7.0, device=dev), torch.full((3, H, W), 7.0, device=dev)
        _lib.check(L.gs_forward_render(ctypes.byref(a), geom.data_ptr(), gb, binning.data_ptr(), bb, img.data_ptr(), ib, cap,
                                       color.data_ptr(), sptr))
        cols2 = torch.rand(P, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        a2 = _lib.GsFwdArgs.from_buffer_copy(a)
        a2.shs, a2.M, a2.colors_precomp = None, 0, cols2.data_ptr()
        _lib.check(L.gs_forward_shared(ctypes.byref(a2), geom.data_ptr(), img.data_ptr(), geom2.data_ptr(), gb, binning.data_ptr(), bb,
                                       img2.data_ptr(), ib, cap, color2.data_ptr(), sptr))
        torch.cuda.synchronize()
        assert not color.any() and not color2.any()   # the empty frame (zero background)
        gC, gD = _g(29)
        gC, g2 = gC.to(dev), torch.cat([gD, torch.zeros(2, H, W)]).to(dev)
        f = dict(dtype=torch.float32, device=dev)
        d = dict(means3D=torch.empty(P, 3, **f), means2D=torch.empty(P, 3, **f), sh=torch.empty(P, cloud.shs.shape[1], 3, **f),
                 colors=torch.empty(P, 3, **f), opacity=torch.empty(P, 1, **f), scales=torch.empty(P, 3, **f),
                 rot=torch.empty(P, 4, **f), cov=torch.empty(P, 6, **f))
        gr = _lib.GsGrads(*(d[k].data_ptr() for k in ("means3D", "means2D", "sh", "colors", "opacity", "scales", "rot", "cov")))
        d_colors2 = torch.full((P, 3), float("nan"), device=dev)
        si = _lib.GsSecondImage(cols2.data_ptr(), color2.data_ptr(), g2.data_ptr(), img2.data_ptr(), ib, int(a.long_lists),
                                d_colors2.data_ptr())
        _lib.check(L.gs_backward_with_second(ctypes.byref(a), radii.data_ptr(), geom.data_ptr(), gb, binning.data_ptr(), bb,
                                             img.data_ptr(), ib, cap, color.data_ptr(), gC.data_ptr(), ctypes.byref(si),
                                             scratch.data_ptr(), sb, ctypes.byref(gr), sptr))
        torch.cuda.synchronize()
    print("overflow: pair count %d against a declared capacity of %d; visible %d" % (real, cap, int((radii > 0).sum())))
    assert int((radii > 0).sum()) > 2000
    assert not d_colors2.any()   # (any() is True for a NaN)


def test_gradient_through_z_against_float64_autograd():
    """512 Gaussians (seed 2) on 64 x 48, the loss on invdepth alone, against float64 autograd of oracle/dense_ref.py with
    colours = 1/(means . V[:, 2]): the only check of the -w/z^2 chain and of its sign.  Same bar and attribution rule; the cap
    is a count here: 10 Gaussians (2 % of 512)."""
    from oracle import dense_ref
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    n, w, h = 512, 64, 48
    frame = 40  # (the orbit camera turned by 0.4 rad: viewmatrix[:3, 2] has an x and a z component)
    cloud, cam = helpers.cloud_and_camera(n, w, h, sh_degree=0, seed=2, frame=frame)
    f64 = _float64(None, n, 2, (w, h), frame)
    flag, n_near, n_pairs = f64["flag"], f64["near"], f64["met"]
    cap = 10
    print("float64 reference: %d undecided pairs of %d, on %d Gaussians (cap %d)" % (n_near, n_pairs, int(flag.sum()), cap))
    gD = torch.randn(1, h, w, generator=torch.Generator().manual_seed(8))
    dt = torch.float64
    leaves = dict(means3D=cloud.xyz.to(dt), means2D=torch.zeros(n, 3, dtype=dt), opacities=cloud.opacity.to(dt),
                  scales=cloud.scales.to(dt), rotations=cloud.rotations.to(dt))
    for t in leaves.values():
        t.requires_grad_(True)
    V = cam.world_view_transform.to(dt)
    assert abs(float(V[0, 2])) > 0.3 and abs(float(V[2, 2])) > 0.3
    z64 = leaves["means3D"] @ V[:3, 2] + V[3, 2]
    ref, radii64, _ = dense_ref.render(w, h, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, dtype=dt), V,
                                       cam.full_proj_transform.to(dt), cam.camera_center.to(dt), leaves["means3D"],
                                       leaves["means2D"], leaves["opacities"], colors_precomp=(1.0 / z64)[:, None].expand(n, 3),
                                       scales=leaves["scales"], rotations=leaves["rotations"])
    (ref[:1] * gD.to(dt)).sum().backward()
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    settings = GaussianRasterizationSettings(h, w, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
                                             cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 0,
                                             cam.camera_center.to(dev), False, False)
    dgr.release_shared_geometry()
    names = dict(means3D=cloud.xyz.to(dev), means2D=torch.zeros(n, 3, device=dev), opacities=cloud.opacity.to(dev),
                 scales=cloud.scales.to(dev), rotations=cloud.rotations.to(dev))
    _leaves(names)
    color, radii, inv = dgr.GaussianRasterizer(settings)(shs=cloud.shs.to(dev), with_invdepth=True, **names)
    from gsplat_mi355 import debug
    seen = []
    debug.second_colors_hook = (lambda t: seen.append(t.detach().clone()))
    try:
        (inv * gD.to(dev)).sum().backward()
    finally:
        debug.second_colors_hook = None
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), radii64.numpy())
    err = float((inv[0].detach().cpu().double() - ref[0].detach()).abs().max())
    print("invdepth against float64: max |delta| %.3g" % err)
    assert err < 1e-5
    # the chain through z is a visible share of the means3D gradient: without it (or with its sign flipped) the bar is missed
    z = names["means3D"].detach() @ cam.world_view_transform.to(dev)[:3, 2] + cam.world_view_transform.to(dev)[3, 2]
    chain = float((seen[0].sum(1) / (z * z))[radii > 0].abs().max())
    gmax = float(leaves["means3D"].grad.abs().max())
    print("chain through z: largest |w / z^2| %.4g against max|dL/dmeans3D| %.4g" % (chain, gmax))
    assert chain > 1000 * PARITY * gmax
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        _assert_bar(k + " vs float64 autograd", names[k].grad.cpu().numpy(), leaves[k].grad.numpy(), flag, cap)


def test_edges_unit_depth_fast_path_everything_culled_no_grad_and_single_gradients():
    """All Gaussians at z = 1 exactly (identity camera): the colours are all ones, the recolour's fast path writes 1 - T --
    asserted bit for bit against 1 - final_T -- and the gradients still match formulation C.  All Gaussians behind the
    camera (D = 0): zero image, zero gradients.  no_grad gives the image of the grad-mode call.  A gradient on invdepth
    alone equals the call given an explicit zero colour gradient, bit for bit; on the colour alone, the call without the
    flag, bit for bit."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355 import debug
    from gsplat_mi355.camera import Camera, focal2fov
    dev = torch.device("cuda:0")
    cloud, _ = _scene(1.0)
    n = 700
    gen = torch.Generator().manual_seed(12)
    cam = Camera(np.eye(3), np.zeros(3), focal2fov(90.0, W), focal2fov(90.0, H), W, H)
    V = cam.world_view_transform
    assert torch.equal(V[:3, :3], torch.eye(3)) and not V[3, :3].any()

    class C(object):
        pass
    flat = C()
    flat.xyz = torch.cat([torch.empty(n, 2).uniform_(-0.6, 0.6, generator=gen), torch.ones(n, 1)], 1).contiguous()
    flat.scales = torch.empty(n, 3).uniform_(0.01, 0.06, generator=gen)
    flat.rotations = cloud.rotations[:n].contiguous()
    flat.opacity = torch.empty(n, 1).uniform_(0.05, 0.95, generator=gen)
    flat.shs, flat.sh_degree = cloud.shs[:n].contiguous(), cloud.sh_degree
    gC, gD = _g(5)
    z, radii0, st = _depths(flat, cam, dev)
    assert bool((z[radii0 > 0] == 1.0).all()) and int((radii0 > 0).sum()) > 500
    (color, inv, radii), one = _one_pass(flat, cam, dev, gC, gD)
    assert torch.equal(inv[0].cpu(), 1.0 - torch.from_numpy(st["image"]["final_T"]))  # the all-ones fast path
    _, two = _formulation_c(flat, cam, dev, gC, gD)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "colors2"):
        _assert_bar("unit depth: " + k, one[k].cpu().numpy(), two[k].cpu().numpy())
    # no_grad; a single gradient
    rast = dgr.GaussianRasterizer(_settings(cam, dev, sh_degree=flat.sh_degree))
    with torch.no_grad():
        res = rast(means2D=torch.zeros(n, 3, device=dev), with_invdepth=True, **_inputs(flat, cam, dev, "sh", "scale_rot"))
    assert len(res) == 3 and torch.equal(res[0], color) and torch.equal(res[2], inv) and not res[2].requires_grad
    cloud1, cam1 = _scene(1.0)
    _, only_d = _one_pass(cloud1, cam1, dev, None, gD)
    _, zero_c = _one_pass(cloud1, cam1, dev, torch.zeros(3, H, W), gD)
    _, only_c = _one_pass(cloud1, cam1, dev, gC, None)
    assert "colors2" in only_d and "colors2" not in only_c
    for k in only_d:
        assert torch.equal(only_d[k], zero_c[k]), k
    dgr.release_shared_geometry()
    names = _leaves(_inputs(cloud1, cam1, dev, "sh", "scale_rot"))
    names["means2D"] = torch.zeros(cloud1.xyz.shape[0], 3, device=dev, requires_grad=True)
    col, _ = dgr.GaussianRasterizer(_settings(cam1, dev, sh_degree=cloud1.sh_degree))(**names)
    (col * gC.to(dev)).sum().backward()
    for k, t in names.items():
        assert torch.equal(only_c[k], t.grad), k
    # everything behind the camera: no pair at all
    back = C()
    back.xyz = flat.xyz * torch.tensor([1.0, 1.0, -1.0])
    back.scales, back.rotations, back.opacity, back.shs, back.sh_degree = flat.scales, flat.rotations, flat.opacity, flat.shs, flat.sh_degree
    (color0, inv0, radii_b), gb = _one_pass(back, cam, dev, gC, gD)
    assert not radii_b.any() and not inv0.any() and not color0.any()
    for k, t in gb.items():
        assert not t.any(), k
    assert "colors2" in gb


def test_render_with_the_flag_and_the_opacity_pass_behind_it():
    """render() with Pipe(invdepth=True) and return_opacity=True: the opacity pass behind the one-pass call is served from
    its geometry (a cache hit) and runs a backward of its own.  Colour and opacity images bit for bit those of render()
    without the flag, invdepth_render that of the rasterizer; the gradients of a loss on all three images equal the sum of
    the gradients of render() without the flag (colour + opacity) and of the one-pass call with the depth gradient alone,
    within twice the parity bar (two separately rounded results are added)."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355.render import Pipe, render
    from gsplat_mi355.scenes import GaussianCloud
    dev = torch.device("cuda:0")
    cloud, cam = _scene(1.0)
    gC, gD = _g(23)
    gO = torch.randn(1, H, W, generator=torch.Generator().manual_seed(24))

    def run(pipe, with_depth):
        dgr.release_shared_geometry()
        pc = GaussianCloud(cloud.xyz.to(dev), cloud.scales.to(dev), cloud.rotations.to(dev), cloud.opacity.to(dev),
                           cloud.shs.to(dev), cloud.sh_degree)
        names = _leaves(dict(means3D=pc.xyz, opacities=pc.opacity, scales=pc.scales, rotations=pc.rotations, shs=pc.shs))
        hits0 = dgr._geom_cache.hits
        pkg = render(cam.to(dev), pc, pipe, torch.zeros(3, device=dev), return_opacity=True)
        cam.to("cpu")
        assert dgr._geom_cache.hits - hits0 == 1  # the opacity pass was served from the first call's geometry
        loss = (pkg.render * gC.to(dev)).sum() + (pkg.opacity_render * gO.to(dev)).sum()
        if with_depth:
            loss = loss + (pkg.invdepth_render * gD.to(dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
        names["means2D"] = pkg.viewspace_points
        return pkg, _grads(names)

    plain, gp = run(Pipe(), False)
    assert plain.invdepth_render is None
    flagged, gf = run(Pipe(invdepth=True, fuse_opacity=True), True)  # (fuse_opacity gives way: the two-call opacity pass)
    (_, inv, _), gd = _one_pass(cloud, cam, dev, None, gD)
    assert torch.equal(flagged.render, plain.render) and torch.equal(flagged.opacity_render, plain.opacity_render)
    assert torch.equal(flagged.invdepth_render.detach(), inv)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        want = gp[k].double() + (gd[k].double() if k in gd else 0.0)
        got = gf[k].double().reshape(want.shape[0], -1).cpu().numpy()
        want = want.reshape(want.shape[0], -1).cpu().numpy()
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
        print("render() with the flag, %s: max|g| %.4g, largest error %.3g of it" % (k, np.abs(want).max(), err))
        assert err <= 2 * PARITY, k


def test_two_runs_give_the_same_bits_and_a_captured_step_replays_the_eager_one():
    """Every output of two runs is bit-identical (no atomics anywhere in the path); one forward + backward with the flag,
    captured with torch.cuda.graph after eager frames on the side stream (the recipe of tests/test_gpu_capture.py),
    replays bit-identically to the eager step."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    cloud, cam = _scene(1.0)
    gC, gD = _g(3)
    (c1, i1, _), a = _one_pass(cloud, cam, dev, gC, gD)
    (c2, i2, _), b = _one_pass(cloud, cam, dev, gC, gD)
    assert torch.equal(c1, c2) and torch.equal(i1, i2) and set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    gCd, gDd = gC.to(dev), gD.to(dev)
    rast = dgr.GaussianRasterizer(_settings(cam, dev, sh_degree=cloud.sh_degree))
    names = _leaves(_inputs(cloud, cam, dev, "sh", "scale_rot"))
    names["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, device=dev, requires_grad=True)

    def step():
        color, radii, inv = rast(with_invdepth=True, **names)
        ((color * gCd).sum() + (inv * gDd).sum()).backward()
        return color, inv

    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            for t in names.values():
                t.grad = None
            dgr.release_shared_geometry()
            step()
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    for t in names.values():
        t.grad = None
    dgr.release_shared_geometry()
    graph = torch.cuda.CUDAGraph()
    dgr.captured_forwards(clear=True)
    with torch.cuda.graph(graph, stream=side):
        color_g, inv_g = step()
    (cnt, capacity), = dgr.captured_forwards(clear=True)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert 0 < int(cnt.item()) <= capacity
    assert torch.equal(color_g, c1) and torch.equal(inv_g, i1)
    for k, t in names.items():
        assert torch.equal(t.grad, a[k]), k


def test_one_forward_one_shared_forward_one_backward(monkeypatch):
    """Launch accounting: the one-pass call makes one gs_forward, one gs_forward_shared, one gs_backward_with_second and
    no gs_backward."""
    from gsplat_mi355 import _lib
    dev = torch.device("cuda:0")
    cloud, cam = _scene(1.0)
    gC, gD = _g(4)
    _one_pass(cloud, cam, dev, gC, gD)  # (sizes the binning state for this shape: the counted frame does not render twice)
    counter = _CallCounter(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counter)
    _one_pass(cloud, cam, dev, gC, gD)
    monkeypatch.undo()
    calls = {k: v for k, v in counter.calls.items() if k.startswith(("gs_forward", "gs_backward", "gs_opacity"))}
    print(calls)
    assert calls == {"gs_forward": 1, "gs_forward_shared": 1, "gs_backward_with_second": 1}
