"""The oracle (and the package's camera helper) against fixtures generated from the reference's own
importable Python (tests/golden/make_golden.py): utils/sh_utils.py and utils/graphics_utils.py.
These are the only parts of the hot path the reference tree pins."""
import os

import numpy as np
import pytest
import torch

from gsplat_mi355.camera import Camera, focal2fov
from gsplat_mi355.scenes import rgb_to_sh

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _all_visible_camera():
    """A camera that sees every point of the fixture (points at radius 2.5, pushed +10 in z)."""
    view = np.eye(4, dtype=np.float32)
    view[3, 2] = 10.0
    proj = np.eye(4, dtype=np.float32)
    proj[2, 3] = 1.0
    proj[3, 3] = 0.0
    return view, (view @ proj).astype(np.float32)


def test_sh_polynomial_matches_reference_eval_sh(oracle):
    g = np.load(os.path.join(GOLD, "sh_eval.npz"))
    dirs = g["dirs"]
    n = dirs.shape[0]
    # reference layout [..., C, coeffs] -> rasterizer layout (n, coeffs, C) (gaussian_model.py:145-148)
    shs = np.ascontiguousarray(g["sh"].transpose(0, 2, 1)).astype(np.float32)
    means = (dirs * 2.5).astype(np.float32)  # campos = 0, so the view direction is `dirs`
    view, projm = _all_visible_camera()
    for deg in range(4):
        sc = oracle.Scene(64, 64, 1.0, 1.0, np.zeros(3), view, projm, np.zeros(3), means, np.ones(n, np.float32),
                          shs=shs, sh_degree=deg, scales=np.full((n, 3), 0.05, np.float32),
                          rotations=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
        st = oracle.preprocess(sc)
        vis = st["radii"] > 0
        assert vis.sum() > n // 2
        assert np.abs(st["rgb"][vis] - g["color_deg%d" % deg][vis]).max() < 2e-6
        raw = g["eval_deg%d" % deg][vis] + 0.5
        sure = np.abs(raw) > 1e-5
        assert ((st["clamped"][vis] != 0) == (raw < 0))[sure].all()


def test_rgb2sh():
    g = np.load(os.path.join(GOLD, "sh_eval.npz"))
    got = rgb_to_sh(torch.from_numpy(g["rgb"])).numpy()
    assert np.abs(got - g["rgb2sh"]).max() < 1e-12


def test_camera_matrices_match_reference_graphics_utils():
    g = np.load(os.path.join(GOLD, "cameras.npz"))
    for k in range(int(g["count"])):
        W, H = [int(v) for v in g["WH_%d" % k]]
        fovx, fovy = g["fov_%d" % k]
        cam = Camera(g["R_%d" % k], g["T_%d" % k], fovx, fovy, W, H)
        assert np.array_equal(cam.world_view_transform.numpy(), g["world_view_%d" % k])
        assert np.array_equal(cam.projection_matrix.numpy(), g["proj_%d" % k])
        assert np.array_equal(cam.full_proj_transform.numpy(), g["full_proj_%d" % k])
        # camera_center = inverse(world_view)[3, :3] in fp32 (the reference's formula, bit for bit on this host); the
        # fixture's value is that inverse on another host, and LAPACK's fp32 inverse rounds differently from CPU to CPU
        wv = torch.from_numpy(g["world_view_%d" % k])
        assert np.array_equal(cam.camera_center.numpy(), wv.inverse()[3, :3].numpy())
        np.testing.assert_array_max_ulp(cam.camera_center.numpy(), g["center_%d" % k], maxulp=4)
        assert focal2fov(500.0 * W / 512.0, W) == fovx


def test_image_losses_match_reference_loss_utils(oracle):
    """N2 pinned: the oracle's L1 and SSIM (values and gradients w.r.t. the rendered image) against fixtures produced by
    the reference's own `l1_loss`, `gaussian`, `create_window`, `ssim`, `_ssim` (utils/loss_utils.py:21-67) run on seeded
    CPU images in fp64 and in fp32 (tests/golden/make_golden.py executes exactly those function definitions).  The
    oracle accumulates in double: it must sit on the reference's fp64 result (1e-9) and within fp32 conv2d rounding of
    the reference's fp32 result; the window entries are the reference's fp32 ones bit for bit."""
    g = np.load(os.path.join(GOLD, "losses.npz"))
    # the reference's 11x11 window (fp32): outer product of the normalised 1-D Gaussian, identical for every channel
    w = g["window"]
    assert w.shape == (3, 1, 11, 11) and w.dtype == np.float32
    g1 = np.array([np.float32(np.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))) for k in range(11)], np.float32)
    assert abs(float(w[0, 0].sum()) - 1.0) < 1e-6 and np.array_equal(w[0], w[2])
    for k in range(int(g["count"])):
        a, b = g["img1_%d" % k], g["img2_%d" % k]
        v, grad = oracle.ssim(a, b)
        assert abs(v - float(g["ssim_f64_%d" % k])) < 1e-9, k
        gs = np.abs(g["ssim_grad_f64_%d" % k]).max()
        if gs > 0:
            assert np.abs(grad - g["ssim_grad_f64_%d" % k]).max() <= 1e-6 * gs, k
        # the reference's own fp32 evaluation differs from fp64 by conv2d rounding (sigma = E[x^2] - mu^2 cancels)
        assert abs(v - float(g["ssim_f32_%d" % k])) < 2e-5, k
        if gs > 0:
            assert np.abs(grad - g["ssim_grad_f32_%d" % k]).max() <= 5e-4 * gs, k
        lv, lgrad = oracle.l1_loss(a, b)
        assert abs(lv - float(g["l1_f64_%d" % k])) <= 1e-12 + 1e-9 * abs(lv), k
        assert abs(lv - float(g["l1_f32_%d" % k])) <= 1e-6 * max(abs(lv), 1e-30) + 1e-9, k
        assert np.array_equal(lgrad, g["l1_grad_f32_%d" % k]), k  # sign(x - y) / n, bit for bit
    assert abs(float(g["ssim_f64_2"]) - 1.0) < 1e-12  # identical images


# ---- round 4: prepass.npz -- the per-Gaussian chains either side of the rasterizer, generated by executing the reference's
# own definitions (tests/golden/make_golden.py::make_prepass).  fp32 against fp32 computed in another operation order:
# tolerances are relative to each tensor's largest magnitude.
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


PREPASS_TOL = 2e-6


def _prepass():
    return np.load(os.path.join(GOLD, "prepass.npz"))


@pytest.mark.parametrize("tag", ["quat", "quat_unit", "matrix"])
@pytest.mark.parametrize("mod", [1.0, 0.6])
def test_build_covariance_oracle_matches_the_references_own_chain(oracle, tag, mod):
    """or_build_covariance against build_covariance_from_scaling_rotation (scene/gaussian_model.py:28-32 over
    utils/general_utils.py:73-108,194-207) executed by the generator: quaternions of any norm, unit quaternions and the
    deformer's 3x3 rotation_precomp (models/deformer/rigid.py:229-231); values and both gradients."""
    d = _prepass()
    rot = d["cov_rot_precomp"] if tag == "matrix" else d["cov_" + tag]
    k = "cov_%s_mod%g" % (tag, mod)
    cov, ds, dr = oracle.build_covariance(d["cov_scaling"], mod, rot, d["cov_g6"])
    assert _rel(cov, d[k]) <= PREPASS_TOL
    assert _rel(ds, d[k + "_dscaling"]) <= 4 * PREPASS_TOL
    assert _rel(dr.reshape(d[k + "_drotation"].shape), d[k + "_drotation"]) <= 4 * PREPASS_TOL


def test_in_kernel_covariance_of_the_scale_rotation_path_matches_the_references_chain(oracle):
    """A4 step 3: the covariance or_preprocess builds from (scales, unit quaternions) -- the kernel does not renormalise
    -- is what the reference's chain gives for the same inputs (the HIP preprocess is bit-exact against or_preprocess
    in conic and radii: tests/test_gpu_parity.py::test_preprocess_and_binning_bit_exact)."""
    d = _prepass()
    import helpers
    n = d["cov_scaling"].shape[0]
    cloud, cam = helpers.cloud_and_camera(n, 64, 64, sh_degree=0, seed=2)
    for mod in (1.0, 0.6):
        sc = oracle.Scene(64, 64, 0.5, 0.5, np.zeros(3, np.float32), cam.world_view_transform.numpy(),
                          cam.full_proj_transform.numpy(), cam.camera_center.numpy(), np.zeros((n, 3), np.float32),
                          np.full(n, 0.5, np.float32), colors_precomp=np.ones((n, 3), np.float32), scales=d["cov_scaling"],
                          rotations=d["cov_quat_unit"], scale_modifier=mod)
        st = oracle.preprocess(sc)
        assert (st["radii"] > 0).all()  # (every Gaussian at the origin, in front of the camera: none culled)
        assert _rel(st["cov3D"], d["cov_quat_unit_mod%g" % mod]) <= PREPASS_TOL


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", ["plain", "cano", "cano_noise"])
def test_sh2rgb_oracle_matches_the_references_SH2RGB_forward(oracle, deg, mode):
    """or_sh2rgb against SH2RGB.forward (models/texture/texture.py:21-38) executed by the generator: the 1e-12 in the
    normalisation, the rotation into the canonical frame by the transposed bone rotation, the view-noise matrix, the
    +0.5 / clamp -- values, d/dfeatures, d/dxyz."""
    d = _prepass()
    M = (deg + 1) ** 2 if deg < 3 else 16
    k = "sh2rgb_deg%d_%s" % (deg, mode)
    R = d["sh_fwd_transform"][:, :3, :3] if mode != "plain" else None
    noise = d[k + "_noise"] if mode == "cano_noise" else None
    col, cl, dsh, dxyz = oracle.sh2rgb(d["sh_features"][:, :M], d["sh_xyz"], d["sh_campos"], deg, R, noise, d["sh_gcol"])
    assert _rel(col, d[k]) <= PREPASS_TOL
    assert ((d[k] == 0) == (cl != 0).reshape(-1, 1).repeat(3, 1) & (d[k] == 0)).all()
    assert (d[k] == 0).any()  # the clamp is exercised
    assert _rel(dsh, d[k + "_dfeatures"]) <= 4 * PREPASS_TOL
    if deg > 0:
        assert _rel(dxyz, d[k + "_dxyz"]) <= 2e-5  # (a difference of nearly equal terms through the normalisation)
    else:
        assert np.abs(dxyz).max() == 0 and np.abs(d[k + "_dxyz"]).max() == 0


def test_densification_statistics_match_the_references_statements(oracle):
    """gs_oracle.densify_stats against add_densification_stats (scene/gaussian_model.py:464-466) and the max_radii2D
    statement of train.py:219, both executed by the generator."""
    d = _prepass()
    mr, acc, dn = oracle.densify_stats(d["st_radii"], d["st_vgrad"], d["st_max_radii2D_in"], d["st_accum_in"], d["st_denom_in"])
    assert np.array_equal(mr, d["st_max_radii2D"])
    assert np.array_equal(dn, d["st_denom"].reshape(-1))
    assert _rel(acc, d["st_accum"].reshape(-1)) <= 1e-6
    assert (d["st_radii"] == 0).any() and (d["st_radii"] > d["st_max_radii2D_in"]).any()


def test_initial_scales_rule_on_brute_force_distances(oracle):
    """The oracle's distCUDA2 restatement (or_dist2) under the statements of create_from_pcd that consume it
    (scene/gaussian_model.py:186-187: clamp at 1e-7, log sqrt, repeated over the three axes), executed by the
    generator on a numpy brute force: duplicates land on the clamp."""
    d = _prepass()
    got = oracle.dist2(d["pcd_points"])
    assert np.array_equal(got.view(np.uint32), d["pcd_mean_d2"].view(np.uint32))
    dist2 = np.maximum(got, np.float32(1e-7))
    assert np.array_equal(dist2, d["pcd_dist2"]) and (dist2 == np.float32(1e-7)).sum() >= 40
    scales = np.log(np.sqrt(dist2))[:, None].repeat(3, 1)
    assert np.abs(scales - d["pcd_scales"]).max() <= 1e-6


def test_oracle_still_produces_its_committed_dumps(oracle):
    """the oracle against ITS OWN committed outputs (tests/golden/self_oracle.npz, written by
    tests/golden/make_self_dumps.py) -- every intermediate of A4-A8 for five small scenes, one per input combination and
    one in the snug tile-rectangle mode.  Not a pin against upstream (the reference holds no rasterizer source): a guard
    against drift -- an edit of oracle/gs_oracle.c that moves the bar the HIP path is held to shows up here.  Integers bit
    for bit; floats to 1e-6 of each tensor's maximum (another libm may round expf differently in the last place)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_self_dumps", os.path.join(GOLD, "make_self_dumps.py"))
    msd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(msd)
    d = np.load(os.path.join(GOLD, "self_oracle.npz"))
    for name, *_ in msd.CASES:
        sc = msd.scene_of(d, name)
        got = msd.outputs_of(oracle, sc, d[name + "/in/dL_dpix"])
        want = {k[len(name) + 5:]: d[k] for k in d.files if k.startswith(name + "/out/")}
        assert sorted(got) == sorted(want), name
        assert int(got["binning/D"]) > 3000
        for k, w in want.items():
            g = np.asarray(got[k])
            if w.dtype.kind in "iub":
                # (a pair within an ulp of a threshold may flip under another expf: n_contrib / n_blended may then move)
                if k in ("image/n_contrib", "image/n_blended"):
                    assert (g != w).mean() <= 1e-3, (name, k)
                else:
                    assert np.array_equal(g, w), (name, k)
            else:
                m = max(float(np.abs(w).max()), 1e-30)
                tol = 1e-6 if not k.startswith(("image/color", "image/final_T", "grad/")) else 2e-6
                bad = np.abs(g.astype(np.float64) - w) / m > tol
                assert bad.mean() <= (1e-3 if k.startswith(("image/", "grad/")) else 0.0), (name, k, float(bad.mean()))
