"""oracle/dense_ref.py's options (antialiasing; aux["invdepth"], aux["opacity"], aux["s"], aux["o_eff"]) on the CPU, before
tests/test_gpu_option_matrix.py uses them as the reference of the device.

The option's per-Gaussian part against tests/antialias_ref.py (an elementwise restatement in the order of csrc/gs_math.h,
written for the option alone) on the two 2051-Gaussian scenes of tests/test_gpu_antialiasing.py; the inverse-depth image
against what it is defined as, a render of the colours 1/depth over a black background; and the defaults against a call
that names none of the new keywords.  Bar: 1e-12 of the tensor's maximum (float64, two operation orders).

tests/antialias_ref.py forms the focal lengths and the clamp limits in fp32, as the kernel does; the twin forms them in
float64, so the restatement is asked for float64 scalars here (`scalar=np.float64`) -- with fp32 ones the two differ by 2e-8.

Measured: o' and s within 2.3e-16 of their maximum, the gradients of sum(gO o') within 2.5e-15 (rotations at scale 1.0;
means3D 1.3e-15, scales and cov3D_precomp 3.1e-16); inverse depth within 6.7e-16, its gradients within 1e-16."""
import math

import numpy as np
import pytest
import torch

import antialias_ref as ref
import helpers
from test_gpu_antialiasing import BEHIND, BORDER, CLAMP, H, W, _scene

TOL = 1e-12
DT = torch.float64


def _camera(cam, bg=(0.0, 0.0, 0.0)):
    return (cam.image_width, cam.image_height, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.tensor(bg, dtype=DT),
            cam.world_view_transform.to(DT), cam.full_proj_transform.to(DT), cam.camera_center.to(DT))


def _leaves(cloud, cov_mode):
    kw = dict(means3D=cloud.xyz.to(DT), means2D=torch.zeros(cloud.xyz.shape[0], 3, dtype=DT), opacities=cloud.opacity.to(DT))
    if cov_mode == "scale_rot":
        kw.update(scales=cloud.scales.to(DT), rotations=cloud.rotations.to(DT))
    else:
        kw["cov3D_precomp"] = helpers.covariance6_cpu(cloud).to(DT)
    for t in kw.values():
        t.requires_grad_(True)
    return kw


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max() / m
    print("%s: max %.4g, largest error %.3g of it" % (name, m, err))
    assert np.isfinite(got).all() and err <= TOL, name


@pytest.mark.parametrize("cov_mode", ["scale_rot", "cov3d"])
@pytest.mark.parametrize("scale_mul", [1.0, 0.05])
def test_effective_opacity_and_its_chain_against_the_restatement(scale_mul, cov_mode):
    """aux["o_eff"] and autograd of sum(gO o') w.r.t. means3D and the covariance inputs against Scene.effective_opacity() and
    Scene.chain(gO) on the rows with radii > 0; the clamped row: s = 0.005 exactly and exactly zero added terms."""
    from oracle import dense_ref
    cloud, cam = _scene(scale_mul)
    kw = _leaves(cloud, cov_mode)
    _, radii, aux = dense_ref.render(*_camera(cam), colors_precomp=torch.zeros(cloud.xyz.shape[0], 3, dtype=DT),
                                     antialiasing=True, **kw)
    vis = (radii > 0).numpy()
    assert vis[CLAMP] and vis[BORDER] and not vis[BEHIND] and vis.sum() > 1500
    cov = (dict(scales=cloud.scales.numpy(), rotations=cloud.rotations.numpy()) if cov_mode == "scale_rot"
           else dict(cov6=helpers.covariance6_cpu(cloud).numpy()))
    sc = ref.Scene(cloud.xyz.numpy(), cloud.opacity.numpy(), cam.world_view_transform.numpy(), W, H, math.tan(cam.FoVx * 0.5),
                   math.tan(cam.FoVy * 0.5), rows=vis, scalar=np.float64, **cov)   # (focal lengths in float64, as the twin forms them)
    o64, s64, free = sc.effective_opacity()
    assert not free[CLAMP] and free[vis].sum() == vis.sum() - 1
    tag = " (scale_mul %g, %s)" % (scale_mul, cov_mode)
    _close("o'" + tag, aux["o_eff"].detach().numpy()[vis], o64[vis])
    _close("s" + tag, aux["s"].detach().numpy()[vis], s64[vis])
    assert float(aux["s"].detach()[CLAMP]) == 0.005
    assert float(aux["o_eff"].detach()[CLAMP]) == float(cloud.opacity.to(DT)[CLAMP, 0]) * 0.005
    if scale_mul == 0.05:
        assert np.median(s64[vis]) < 0.5
    gO = torch.randn(cloud.xyz.shape[0], generator=torch.Generator().manual_seed(6))   # (fp32 values: what chain() takes)
    names = ["means3D"] + (["scales", "rotations"] if cov_mode == "scale_rot" else ["cov3D_precomp"])
    got = torch.autograd.grad((aux["o_eff"] * gO.to(DT)).sum(), [kw[k] for k in names])
    want = sc.chain(gO.numpy())
    for k, g in zip(names, got):
        w = want["cov3D" if k == "cov3D_precomp" else k]
        assert np.abs(w).max() > 0
        _close(k + tag, g.numpy()[vis], w[vis])
        assert not g[CLAMP].any() and not w[CLAMP].any(), k   # the clamped branch is a constant


def test_inverse_depth_is_the_render_of_inverse_depths_over_black():
    """aux["invdepth"] and its gradients (a non-black background, antialiasing on) against channel 0 of a second call with
    colors_precomp = 1/depth, differentiable through means3D, and bg = 0; aux["opacity"] against its definition."""
    from oracle import dense_ref
    n, w, h = 512, 64, 48
    cloud, cam = helpers.cloud_and_camera(n, w, h, sh_degree=3, seed=2, frame=40)
    gD = torch.randn(1, h, w, generator=torch.Generator().manual_seed(8)).to(DT)
    bg = (0.3, 0.6, 0.1)
    a = _leaves(cloud, "scale_rot")
    img, radii, aux = dense_ref.render(*_camera(cam, bg), shs=cloud.shs.to(DT), sh_degree=3, antialiasing=True, **a)
    ga = torch.autograd.grad((aux["invdepth"] * gD).sum(), list(a.values()))
    b = _leaves(cloud, "scale_rot")
    V = cam.world_view_transform.to(DT)
    z = b["means3D"] @ V[:3, 2] + V[3, 2]
    img2, radii2, aux2 = dense_ref.render(*_camera(cam), colors_precomp=(1.0 / z)[:, None].expand(n, 3), antialiasing=True, **b)
    gb = torch.autograd.grad((img2[:1] * gD).sum(), list(b.values()))
    assert torch.equal(radii, radii2) and int((radii > 0).sum()) > 400
    _close("invdepth", aux["invdepth"].detach().numpy(), img2[:1].detach().numpy())
    for k, x, y in zip(a, ga, gb):
        assert float(y.abs().max()) > 0, k
        _close("invdepth, " + k, x.numpy(), y.numpy())
    T = aux["T_final"].detach()
    assert torch.equal(aux["opacity"].detach()[0], (1.0 - T) + T * bg[0]) and float(T.min()) < 0.5 < float(T.max())
    assert not aux["invdepth"].detach()[0][~aux["include"].any(1).view(h, w)].any()   # nothing composited: exactly 0


@pytest.mark.parametrize("cov_mode", ["scale_rot", "cov3d"])
def test_defaults_are_a_call_that_names_no_new_keyword(cov_mode):
    """antialiasing=False named against not named: image, radii and every aux entry torch.equal; s is all ones and o' = o."""
    from oracle import dense_ref
    n, w, h = 300, 48, 32
    cloud, cam = helpers.cloud_and_camera(n, w, h, sh_degree=2, seed=11, scale_mul=1.5)
    with torch.no_grad():
        kw = {k: v.detach() for k, v in _leaves(cloud, cov_mode).items()}
        bare = dense_ref.render(*_camera(cam, (0.2, 0.1, 0.3)), shs=cloud.shs.to(DT), sh_degree=2, scale_modifier=0.7, **kw)
        named = dense_ref.render(*_camera(cam, (0.2, 0.1, 0.3)), shs=cloud.shs.to(DT), sh_degree=2, scale_modifier=0.7,
                                 antialiasing=False, **kw)
        on = dense_ref.render(*_camera(cam, (0.2, 0.1, 0.3)), shs=cloud.shs.to(DT), sh_degree=2, scale_modifier=0.7,
                              antialiasing=True, **kw)
    assert torch.equal(bare[0], named[0]) and torch.equal(bare[1], named[1]) and set(bare[2]) == set(named[2])
    for k in bare[2]:
        assert torch.equal(bare[2][k], named[2][k]), k
    assert torch.equal(bare[2]["s"], torch.ones(n, dtype=DT)) and torch.equal(bare[2]["o_eff"], kw["opacities"].reshape(-1))
    assert torch.equal(on[1], bare[1]) and not torch.equal(on[0], bare[0]) and float(on[2]["s"].max()) < 1.0
