"""The rasterizer's inverse-depth image, host side (no GPU): the C ABI's new trailing field GsSecondImage.dL_dcolors in the
binding and in the header, the `with_invdepth` argument through the public surface, argument handling of
gs_backward_with_second with and without the field, and a float64 check of the DEFINITION the GPU tests compare against:
invdepth = sum alpha T / z, which is the colour image of the same geometry with colours (1/z, 1/z, 1/z) over a zero
background."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import abi_header
import helpers
import test_cabi_host as cabi
from test_cabi_host import lib  # noqa: F401  (the fixture: builds the library if it is not there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_second_image_struct_has_the_trailing_field_in_binding_and_header():
    from gsplat_mi355 import _lib
    assert _lib.GsSecondImage._fields_[-1] == ("dL_dcolors", ctypes.c_void_p)
    assert abi_header.parse().structs["GsSecondImage"][-1].name == "dL_dcolors"
    header = abi_header.text()
    assert "get theirs when asked" in header and "get none" not in header
    capture = header[header.index("Stream capture"):header.index("typedef struct GsFwdArgs {")]
    assert "GsSecondImage.dL_dcolors" in capture


def test_the_binding_names_the_not_all_ones_word_as_the_library_does():
    """The wrapper clears the geometry state's "a second render's colours are not all ones" word after the node's own
    shared render; its index in the count block is the library's enum, mirrored in the binding."""
    from gsplat_mi355 import _lib
    src = open(os.path.join(ROOT, "3dgs-avatar-release_amd", "csrc", "common.h")).read()
    m = re.search(r"enum \{ COUNT_PAIRS = 0, COUNT_NOT_ONES = (\d+), COUNT_ZERO_BYTES = (\d+) \}", src)
    assert m and int(m.group(1)) == _lib.GS_COUNT_NOT_ONES
    assert 8 * (_lib.GS_COUNT_NOT_ONES + 1) <= int(m.group(2))  # inside what the numbering kernels clear with the count


def test_six_argument_construction_leaves_the_new_field_null():
    from gsplat_mi355 import _lib
    si = _lib.GsSecondImage(cabi.FAKE, cabi.FAKE, cabi.FAKE, cabi.FAKE, cabi.BIG, 0)
    assert si.dL_dcolors is None and si.long_lists == 0 and si.img_bytes == cabi.BIG
    assert _lib.GsSecondImage(1, 2, 3, 4, 5, 1, 7).dL_dcolors == 7


def test_public_surface_accepts_with_invdepth():
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355.render import Pipe
    for fn in (dgr.GaussianRasterizer.forward, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "with_invdepth" in p and p["with_invdepth"].default is False
    n_inputs = len(inspect.signature(dgr._RasterizeGaussians.forward).parameters) - 1  # (ctx)
    assert "with_invdepth" in inspect.signature(dgr._RasterizeGaussians.forward).parameters
    assert len(dgr._InferenceCtx.needs_input_grad) == n_inputs and not any(dgr._InferenceCtx.needs_input_grad)
    assert len(dgr.GaussianRasterizationSettings._fields) == 13
    assert Pipe(invdepth=True).invdepth is True and Pipe().invdepth is False


def test_opacity_and_invdepth_together_are_refused_before_any_device_call(monkeypatch):
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355 import _lib

    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_library)
    settings = dgr.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                                 torch.zeros(3), False, False)
    n = 4
    with pytest.raises(NotImplementedError):
        dgr.GaussianRasterizer(settings)(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 3), opacities=torch.ones(n, 1),
                                         colors_precomp=torch.ones(n, 3), scales=torch.ones(n, 3),
                                         rotations=torch.ones(n, 4), with_opacity=True, with_invdepth=True)


@pytest.mark.parametrize("dcolors", [None, cabi.FAKE], ids=["null", "set"])
def test_backward_with_second_answers_bad_arguments_as_before(lib, dcolors):  # noqa: F811
    """Every bad-argument case tests/test_cabi_host.py records for gs_backward_with_second (codes of the library before the
    field existed), with GsSecondImage.dL_dcolors NULL and non-NULL: fake pointers, never dereferenced -- all of them fail
    validation before anything is enqueued."""
    calls = cabi._entry_points(lib)
    cases = [(over, rc) for name, over, rc in cabi.BOUNDARY_CASES if name == "with_second"]
    cases += [(dict(second_img_bytes=cabi.SMALL), cabi.BAD_ARG),
              (dict(a_W=1024, a_H=1024, second_long_lists=1), cabi.BAD_ARG),
              (dict(a_W=1024, a_H=1024, a_long_lists=1, second_long_lists=0), cabi.BAD_ARG),
              (dict(second_out_color=None), cabi.BAD_ARG), (dict(second_dL_dpix=None), cabi.BAD_ARG)]
    assert len(cases) >= 12
    for over, rc in cases:
        if over.get("second", True) is not None:
            over = dict(over, second_dL_dcolors=dcolors)
        assert calls["with_second"](**over) == rc, over


def test_definition_in_float64_colour_render_of_inverse_depths_is_sum_alpha_T_over_z():
    """oracle.dense_ref.render with colors_precomp = 1/z in three channels and bg = 0 against sum alpha T / z built
    directly from its aux (the blended pairs `include`, the conics, centres and depths): what the GPU tests use as the
    reference image IS the definition."""
    from oracle import dense_ref
    n, W, H = 256, 48, 40
    cloud, cam = helpers.cloud_and_camera(n, W, H, sh_degree=0, seed=2, scale_mul=0.3)  # (small enough to leave empty pixels)
    dt = torch.float64
    V = cam.world_view_transform.to(dt)
    z = cloud.xyz.to(dt) @ V[:3, 2] + V[3, 2]
    inv = torch.where(z > 0.2, 1.0 / z, torch.zeros_like(z))
    args = (W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, dtype=dt), V, cam.full_proj_transform.to(dt),
            cam.camera_center.to(dt), cloud.xyz.to(dt), torch.zeros(n, 3, dtype=dt), cloud.opacity.to(dt))
    color, radii, aux = dense_ref.render(*args, colors_precomp=inv[:, None].expand(n, 3), scales=cloud.scales.to(dt),
                                         rotations=cloud.rotations.to(dt))
    assert torch.allclose(aux["depth"], z, rtol=0, atol=1e-12)
    o = aux["order"]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    dx = aux["px"][o][None] - xs.reshape(-1)[:, None]
    dy = aux["py"][o][None] - ys.reshape(-1)[:, None]
    con = aux["conic"][o]
    power = -0.5 * (con[:, 0][None] * dx * dx + con[:, 2][None] * dy * dy) - con[:, 1][None] * dx * dy
    alpha = torch.clamp_max(cloud.opacity.to(dt).reshape(-1)[o][None] * torch.exp(power), 0.99)
    a = torch.where(aux["include"], alpha, torch.zeros_like(alpha))
    T = torch.cumprod(1.0 - a, 1)
    T = torch.cat([torch.ones(H * W, 1, dtype=dt), T[:, :-1]], 1)
    direct = ((a * T) / z[o][None]).sum(1).view(H, W)
    assert (radii > 0).sum() > 100 and float(direct.max()) > 0.05
    assert torch.equal(color[0], color[1]) and torch.equal(color[0], color[2])
    err = float((color[0] - direct).abs().max())
    print("definition: max |colour render of 1/z - sum alpha T / z| = %.3g (max value %.3g)" % (err, float(direct.max())))
    assert err <= 1e-13
    empty = ~aux["include"].any(1).view(H, W)
    assert empty.any() and not color[0][empty].any()
