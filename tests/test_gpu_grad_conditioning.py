"""Rasterizer gradients per Gaussian, each against its own scale (the bound of tests/grad_conditioning.py: u (n A + C0 A +
C1 B) from the oracle's or_render_backward_cond, derivation and constants there, validated without a device in
tests/test_grad_conditioning_host.py).  Every other gradient test of the suite divides the error by the tensor's largest
element; a faint, sub-pixel or deeply buried Gaussian is then below the bar whatever its gradient is.  Here EVERY element is
compared with the bound of its own Gaussian's sums, no element exempt, and a Gaussian without pairs must have exact zeros.

Frames of 40 x 24 (one full tile row, a partial row, a partial column), a few hundred Gaussians, the oracle conditioned on
the device's attributed threshold decisions as everywhere in the suite:
  ladder  opacities 0.9 .. 1.5 / 255 and footprints from screen-filling to a tenth of a pixel, six large bright ones in front
  wall    24 near-opaque Gaussians in front of 100 ordinary ones: T of 1e-2 .. 1e-4 behind them, pixels that stop early
  edge    centres outside the frame reaching in with their tails, the last partial tile, a near-opaque layer in front
  long    test_gpu_bwd_round_boundary._stack(420, opacity=(0.012, 0.02), small=140): the backward in chunks from checkpoints
Each asserts its premise first (grad_conditioning.premise): the A_i span six decades and a quarter of the Gaussians with
pairs have rows below 1e-5 of their tensor's maximum, in every tensor compared.  The Long frame is the one the chunked-backward
test fixes, all opacities 0.012 .. 0.02 and T >= 6e-3: its A_i span four decades in the conic sums only and none of its rows
is that small, so there the span is asserted on the widest of the nine sums and the share is printed, not asserted.

Measured on an MI355X, largest error / bound over all elements (m3D means3D, m2D means2D, opa opacities, col colors_precomp,
scl scales, rot rotations; mode 0 plain, 1 with_opacity, 2 / 3 second image with arbitrary colours / colours one).  The two
`sh 5.6` are from before the SH rows' chain term took the basis polynomials' absolute form (grad_conditioning.sh_jacobian_abs:
one Gaussian's x (xx - 3 yy) is -1.07e-6); every other SH row of those runs was at or below 0.009.  Without the bound's
front-to-back term (C3 cond_R) the same runs gave 3.3 to 33 on the geometric sums of ladder, wall and edge (largest: edge,
opacities 32.6, means2D 30.9; ladder 26.7; wall 16.8), all in the decades of A_i below 1, and these figures on the colour sums:
    ladder mode 0                m3D 0.024  m2D 0.048  opa 0.026  cov3D 0.029  col 0.035
    ladder mode 1                m3D 0.017  m2D 0.035  opa 0.019  cov3D 0.024  col 0.032
    ladder mode 2                m3D 0.018  m2D 0.037  opa 0.038  cov3D 0.019  col 0.032
    ladder mode 3                m3D 0.013  m2D 0.025  opa 0.012  cov3D 0.016  col 0.032
    wall mode 0                  m3D 0.008  m2D 0.016  opa 0.016  cov3D 0.008  col 0.026
    wall mode 1                  m3D 0.006  m2D 0.012  opa 0.012  cov3D 0.006  col 0.026
    wall mode 2                  m3D 0.0055  m2D 0.011  opa 0.011  cov3D 0.0055  col 0.026
    wall mode 3                  m3D 0.0038  m2D 0.0075  opa 0.0075  cov3D 0.0038  col 0.026
    edge mode 0                  m3D 0.014  m2D 0.029  opa 0.029  cov3D 0.014  col 0.03
    long mode 0                  m3D 0.00094  m2D 0.0016  opa 0.0025  cov3D 0.0023  col 0.0082
    long mode 0 unchunked        m3D 0.00094  m2D 0.0016  opa 0.0025  cov3D 0.0023  col 0.0082
    ladder sh                    m3D 0.025  m2D 0.051  opa 0.024  sh 0.023  scl 0.028  rot 0.014
    ladder sh antialiasing       m3D 0.008  m2D 0.017  opa 0.0087  sh 0.022  scl 0.0089  rot 0.0089
    wall sh                      m3D 0.0081  m2D 0.017  opa 0.017  sh 5.6  scl 0.008  rot 0.0072
    wall sh antialiasing         m3D 0.014  m2D 0.029  opa 0.014  sh 5.6  scl 0.014  rot 0.014
    per decade of A_i (all scenes): 1e-7: 0.03  1e-6: 0.027  1e-5: 0.029  1e-4: 0.029  1e-3: 0.026  1e-2: 0.029  1e-1: 0.051  1e0: 0.037  1e1: 0.029  1e2: 0.015  1e3: 0.0035  1e4: 1.8e-05
"""
import math

import numpy as np
import pytest
import torch

import grad_conditioning as gc
import helpers
from test_gpu_parity import _attribute, _inputs, _settings

pytestmark = pytest.mark.gpu

W, H, BG = gc.W, gc.H, gc.BG
PRECOMP = ("means3D", "means2D", "opacities", "cov3D_precomp", "colors_precomp")
SH = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
ORACLE_NAME = dict(shs="sh")


def _device(cloud, cam, color_mode, cov_mode, mode=0, antialiasing=False, g0=None, g1=None, cols2=None):
    """One frame through the drop-in rasterizer, two backward passes of it; returns (image, gradients by leaf name).  `mode`
    as in test_gpu_bwd_round_boundary._run: 0 one image, 1 with_opacity=True, 2 / 3 a second image with the colours `cols2`."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    n = cloud.xyz.shape[0]
    settings = _settings(cam, cloud, BG, dev)._replace(antialiasing=antialiasing)

    def once(backwards):
        dgr.release_shared_geometry()
        leaves = {k: v.clone().requires_grad_(True) for k, v in _inputs(cloud, cam, color_mode, cov_mode, dev).items()}
        leaves.update(means3D=cloud.xyz.to(dev).requires_grad_(True), means2D=torch.zeros(n, 3, device=dev, requires_grad=True),
                      opacities=cloud.opacity.to(dev).requires_grad_(True))
        rast = dgr.GaussianRasterizer(settings)
        if mode == 1:
            img, _, opa = rast(with_opacity=True, **leaves)
            loss = (img * g0.to(dev)).sum() + (opa * g1[:1].to(dev)).sum()
        else:
            img, _ = rast(**leaves)
            loss = (img * g0.to(dev)).sum()
            if mode >= 2:
                second = dict(leaves, colors_precomp=cols2.to(dev))
                img2, _ = rast(**second)
                loss = loss + (img2 * g1.to(dev)).sum()
        grads = []
        for k in range(backwards):
            for t in leaves.values():
                t.grad = None
            loss.backward(retain_graph=k + 1 < backwards)
            grads.append({name: t.grad.detach().cpu().numpy().copy() for name, t in leaves.items()})
        torch.cuda.synchronize()
        return img.detach().cpu().numpy(), grads

    if mode <= 1:
        img, (got, again) = once(2)
    else:  # (the two-image step hands its second render's state to one backward: the frame is run twice instead)
        img, (got,) = once(1)
        img_b, (again,) = once(1)
        assert np.array_equal(img, img_b)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), "two backward passes differ in " + k
    return img, got


def _state(cloud, cam, color_mode, cov_mode, antialiasing=False):
    from gsplat_mi355 import debug
    dev = torch.device("cuda:0")
    settings = _settings(cam, cloud, BG, dev)._replace(antialiasing=antialiasing)
    return debug.forward_state(settings, cloud.xyz.to(dev), cloud.opacity.to(dev), **_inputs(cloud, cam, color_mode, cov_mode, dev))


def _compare(oracle, tag, got, want, cond, J, names, culled, extra_bound=None, J_chain=None):
    """Every element of every tensor of `names` against its bound; prints the largest ratio per tensor and per decade of A_i."""
    worst = {}
    for name in names:
        on = ORACLE_NAME.get(name, name)
        w = np.asarray(want[on], np.float64).reshape(culled.size, -1)
        g = got[name].reshape(culled.size, -1)
        if extra_bound and name in extra_bound:
            bound, A_row = extra_bound[name]
        elif name in gc.DIRECT:
            bound, A_row = gc.direct_bound(cond, name), cond["cond_A"][:, gc.DIRECT[name]].max(1)
        else:
            bound = gc.derived_bound(oracle, cond, J[on], (J_chain or {}).get(on))
            A_row = oracle.through_jacobian(J[on], cond["cond_A"]).max(1)
        r = gc.ratios(g, w, bound)
        assert (g[culled] == 0).all(), "%s: %s: a culled Gaussian has a gradient" % (tag, name)
        assert (g[cond["cond_n"] == 0] == 0).all(), "%s: %s: a Gaussian without pairs has a gradient" % (tag, name)
        table = gc.decade_table(r, A_row)
        worst[name] = float(r.max())
        print("%s %-14s largest error / bound %.3g (error / tensor maximum %.3g); per decade of A_i: %s"
              % (tag, name, r.max(), helpers.rel_to_max(g, w), " ".join("1e%d:%.2g" % kv for kv in sorted(table.items()))))
    for name, r in worst.items():
        assert r <= 1.0, "%s: %s exceeds its per-Gaussian bound: %.3g" % (tag, name, r)
    return worst


def _conditioned(oracle, sc, st, tag):
    fw = oracle.forward(sc)
    assert np.array_equal(st["radii"], fw["radii"])
    return _attribute(oracle, sc, fw, st["color"], st["image"]["final_T"], st["image"]["n_contrib"], tag)


def _precomputed(oracle, scene, mode, chunks=1):
    from gsplat_mi355 import _lib
    cloud, cam = gc.SCENES[scene]()
    n = cloud.xyz.shape[0]
    tag = "%s mode %d%s" % (scene, mode, "" if chunks else " unchunked")
    g0, g1 = gc.pixel_gradients(scene), gc.pixel_gradients(scene, second=True)
    cols2 = torch.rand(n, 3, generator=torch.Generator().manual_seed(11)) if mode == 2 else torch.ones(n, 3)
    _lib.tuning("bwd_chunks", chunks)
    try:
        img, got = _device(cloud, cam, "precomp", "cov", mode, g0=g0, g1=g1, cols2=cols2)
    finally:
        _lib.tuning("bwd_chunks", 1)
    st = _state(cloud, cam, "precomp", "cov")
    assert np.array_equal(img, st["color"])
    sc = helpers.oracle_scene(cloud, cam, bg=BG, color_mode="precomp", cov_mode="cov")
    fwc, ov = _conditioned(oracle, sc, st, tag)
    want = oracle.backward(sc, fwc, g0.numpy(), ov, conditioning=True)
    cond = {k: want[k] for k in gc.COND}
    if mode >= 1:  # the conditions of the two images add (the second image's colour sums go nowhere)
        sc2 = helpers.oracle_scene(cloud, cam, bg=BG, color_mode="precomp", colors=cols2, cov_mode="cov")
        fw2 = oracle.forward(sc2)
        im2 = oracle.render_forward(sc2, fw2["geom"], fw2["binning"], ov)
        g2 = g1.numpy().copy()
        if mode == 1:
            g2[1:] = 0.0  # the opacity image is one channel of the colours-one image
        b2 = oracle.backward(sc2, dict(fw2, image=im2, color=im2["color"]), g2, ov, conditioning=True)
        want = dict(want)
        for k in ("means3D", "means2D", "opacities", "cov3D_precomp"):
            want[k] = np.asarray(want[k], np.float64) + b2[k]
        for k in ("cond_A", "cond_B", "cond_R", "sums"):
            b2[k][:, 6:] = 0.0
        cond = gc.add_conditions(cond, b2)
    return tag, sc, fwc, got, want, cond


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["plain", "with-opacity", "second-image-arbitrary-colours", "second-image-colours-one"])
@pytest.mark.parametrize("scene", ["ladder", "wall"])
def test_precomputed_inputs_every_kernel_mode(oracle, scene, mode):
    tag, sc, fwc, got, want, cond = _precomputed(oracle, scene, mode)
    gc.premise(cond, want, PRECOMP, gc.DECADES[scene], tag)
    if scene == "wall":  # pixels stop early, and Gaussians behind the wall are left without a single pair
        assert float(fwc["image"]["final_T"].min()) < 2e-4 and (cond["cond_n"][fwc["radii"] > 0] == 0).any()
    _compare(oracle, tag, got, want, cond, oracle.preprocess_jacobian(sc, fwc), PRECOMP, fwc["radii"] == 0)


@pytest.mark.parametrize("scene,chunks", [("edge", 1), ("long", 1), ("long", 0)], ids=["edge", "long", "long-one-wave-per-quadrant"])
def test_edge_and_long_lists(oracle, scene, chunks):
    tag, sc, fwc, got, want, cond = _precomputed(oracle, scene, 0, chunks)
    if scene == "long":
        # (see the module docstring: the frame is fixed by the chunked-backward test)
        vis = cond["cond_n"] > 0
        spans = [math.log10(cond["cond_A"][vis, k].max() / cond["cond_A"][vis, k].min()) for k in range(9)]
        shares = {k: float((np.abs(want[k]).reshape(vis.size, -1).max(1)[vis] < 1e-5 * np.abs(want[k]).max()).mean()) for k in PRECOMP}
        print("%s: A_i span per sum, decades: %s; share of rows below 1e-5 of the tensor maximum: %s" % (tag, " ".join("%.1f" % s for s in spans), shares))
        assert max(spans) >= gc.DECADES[scene]
        assert int(fwc["image"]["n_contrib"].max()) > 2 * 128  # pixels whose walk spans three chunks
        if chunks == 0:  # the one-wave walk is another path: its bits differ from the chunked walk's somewhere
            _, _, _, chunked, _, _ = _precomputed(oracle, scene, 0, 1)
            assert any((chunked[k].view(np.uint32) != got[k].view(np.uint32)).any() for k in got)
    else:
        gc.premise(cond, want, PRECOMP, gc.DECADES[scene], tag)
        assert (fwc["radii"] == 0).any()  # Gaussians too far outside are culled: exact zeros
    _compare(oracle, tag, got, want, cond, oracle.preprocess_jacobian(sc, fwc), PRECOMP, fwc["radii"] == 0)


def _effective(cloud, st):
    """o' [n, 1] as the device stored it (record word 5); culled Gaussians keep o."""
    o = cloud.opacity.numpy().copy()
    vis = st["radii"] > 0
    o[vis, 0] = st["geom"]["rec"][vis, 5]
    return torch.from_numpy(o)


@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain", "antialiasing"])
@pytest.mark.parametrize("scene", ["ladder", "wall"])
def test_sh_degree_3_with_scales_and_rotations(oracle, scene, antialiasing):
    """shs + scales / rotations.  With antialiasing the reference is, as in test_gpu_antialiasing.py, the default path at the
    effective opacities o' = o s the device stored (the oracle conditioned on that frame) plus the chain through s of
    tests/antialias_ref.py in float64: dL/do = s g'_o, means3D / scales / rotations = g' + d o' / d theta g'_o.  The opacity
    sum then reaches four tensors: its column of their Jacobians is d o' / d theta (s for the opacities, from the float64
    twin), and the bound is the derived one for all of them."""
    import antialias_ref
    import copy
    from oracle import dense_ref
    cloud, cam = gc.SCENES[scene]()
    n = cloud.xyz.shape[0]
    tag = "%s sh%s" % (scene, " antialiasing" if antialiasing else "")
    g0 = gc.pixel_gradients(scene)
    img, got = _device(cloud, cam, "sh", "scale_rot", 0, antialiasing, g0=g0)
    st = _state(cloud, cam, "sh", "scale_rot", antialiasing)
    assert np.array_equal(img, st["color"])
    ocloud = cloud
    if antialiasing:
        ocloud = copy.copy(cloud)
        ocloud.opacity = _effective(cloud, st)
        assert not torch.equal(ocloud.opacity, cloud.opacity)
    sc = helpers.oracle_scene(ocloud, cam, bg=BG)
    fwc, ov = _conditioned(oracle, sc, st, tag)
    want = dict(oracle.backward(sc, fwc, g0.numpy(), ov, conditioning=True))
    cond = {k: want[k] for k in gc.COND}
    J = oracle.preprocess_jacobian(sc, fwc)
    extra = None
    if antialiasing:
        vis = fwc["radii"] > 0
        t = lambda x: torch.from_numpy(np.asarray(x, np.float64))
        _, _, aux = dense_ref.render(W, H, sc.tanfovx, sc.tanfovy, t(sc.bg), t(sc.viewmatrix), t(sc.projmatrix), t(sc.campos),
                                     t(cloud.xyz), torch.zeros(n, 3, dtype=torch.float64), t(cloud.opacity), shs=t(cloud.shs),
                                     scales=t(cloud.scales), rotations=t(cloud.rotations), sh_degree=3, antialiasing=True)
        s = aux["s"].numpy()
        ref = antialias_ref.Scene(cloud.xyz.numpy(), cloud.opacity.numpy(), cam.world_view_transform.numpy(), W, H,
                                  sc.tanfovx, sc.tanfovy, scales=cloud.scales.numpy(), rotations=cloud.rotations.numpy(), rows=vis)
        o64, s_ref, _ = ref.effective_opacity()
        assert np.abs(s[vis] - s_ref[vis]).max() <= 1e-6  # (the twin's s and the restatement's, focal lengths in float64 and fp32)
        gO = cond["sums"][:, 5]
        chain, unit = ref.chain(gO), ref.chain(np.ones(n))
        want["opacities"] = (s * gO)[:, None]
        J = {k: v.astype(np.float64).copy() for k, v in J.items()}
        for k in ("means3D", "scales", "rotations"):
            want[k] = np.asarray(want[k], np.float64) + chain[k]
            J[k][:, :, 5] = unit[k]
        Jo = np.zeros((n, 1, 9))
        Jo[:, 0, 5] = s
        extra = {"opacities": (gc.derived_bound(oracle, cond, Jo), oracle.through_jacobian(Jo, cond["cond_A"]).max(1))}
    gc.premise(cond, {ORACLE_NAME.get(k, k): want[ORACLE_NAME.get(k, k)] for k in SH}, [ORACLE_NAME.get(k, k) for k in SH],
               gc.DECADES[scene], tag)
    _compare(oracle, tag, got, want, cond, J, SH, fwc["radii"] == 0, extra, {"sh": gc.sh_jacobian_abs(sc, fwc, J["sh"])})
