"""The per-Gaussian gradient bound of tests/grad_conditioning.py (u (n A + C0 A + C1 B), derivation there), validated on
the references alone: the CPU oracle's fp32 terms against the float64 twin oracle/dense_ref.py -- no device.

The twin is given the oracle's own per-Gaussian 2-D state (pixel position and conic, the fp32 values as float64:
dense_ref.render's `state2d`), so that what is compared is the compositing arithmetic the bound describes and not the
rounding of the projection in front of it, which the device shares with the oracle bit for bit
(test_gpu_parity.py::test_preprocess_and_binning_bit_exact).

Measured, validation at HALF the constants (C0 / 2 = 26, C1 / 2 = 6, no n_i part), largest |oracle - twin| / bound over all
Gaussians and the nine sums, on reduced forms of the device scenes whose every threshold decision keeps a margin of 1e-3:
ladder (40 Gaussians) 0.052, wall (38) 0.030, edge (53, 26 with pairs) 0.026, plain cloud (40) 0.020; the colour sums are
the tightest (0.02 - 0.05), the geometric sums 0.002 - 0.013.  The eight-probe Jacobian reproduces the derived rows within
0.17 (scales), 0.12 (rotations), 0.011 (cov3D), 0.006 (means3D), 0.0015 (sh) of C2 u |J| |s|.

The device's bound has a fourth term, C3 cond_R, for the kernel's front-to-back dL/dalpha recurrence; this file evaluates that
recurrence in fp32 and shows both that the three-term bound does not hold it (8.1 times, where A_i is small) and that the
four-term bound does (0.013).  With that term the dropped pair of the sensitivity test -- T ~ 1e-4 behind two dozen pairs -- is
rejected through its colour row (3e4 bounds); its geometric rows are within what the kernel itself can lose there.

Two statements of the issue this file cannot make as written, both consequences of Cabs_c being the pixel's TOTAL absolute
colour (own pair included), which is what the issue prescribes and what gs_oracle.c computes:
* "A == |sum| for one Gaussian on one pixel": the pair's own alpha T |col| is part of Cabs, so the six geometric sums have
  A == (1 + alpha T) |sum| there, and the colour sum A == |sum|; both are asserted, to rounding.
* "A >= |sum|" is not a theorem: T |col - accum_rec| <= T (|col| + Cabs) needs Cabs >= |accum_rec|, which a dark Gaussian of
  large alpha directly in front of a much brighter one violates.  It is asserted on every scene of the suite, where it holds."""
import numpy as np
import pytest
import torch

import grad_conditioning as gc
import helpers
from oracle import dense_ref

U = gc.U


def _scene(cloud, cam, tile_rect=0, color_mode="precomp", cov_mode="cov", bg=gc.BG):
    return helpers.oracle_scene(cloud, cam, bg=bg, color_mode=color_mode, cov_mode=cov_mode, tile_rect=tile_rect)


def _with_margins(oracle, maker, **kw):
    """The first seed at which no threshold decision of the oracle's forward lies within 1e-3 of its threshold."""
    for seed in range(400):
        cloud, cam = maker(seed=seed, **kw)
        if float(cloud.opacity.max()) > 0.95:
            continue  # (alpha would reach the 0.99 clamp, through which autograd passes nothing and the kernels do)
        sc = _scene(cloud, cam)
        fw = oracle.forward(sc, margin=True)
        if float(fw["image"]["margin"].min()) >= 1e-3:
            return seed, cloud, cam, sc, fw
    raise AssertionError("no seed with a margin of 1e-3 on every decision")


def _plain(seed, n=40):
    cloud, cam = helpers.cloud_and_camera(n, gc.W, gc.H, sh_degree=3, seed=seed, scale_mul=1.5)
    cloud.opacity = cloud.opacity.clamp(max=0.9)
    return cloud, cam


def _twin(sc, fw):
    """dense_ref.render in float64 on the oracle's 2-D state: (colour image [3, H, W], leaves means2D, conic, opacities,
    colours, aux)."""
    dt = torch.float64
    t = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    st = fw["geom"]
    leaves = dict(means2D=torch.zeros(sc.P, 3, dtype=dt), conic=t(st["conic_opacity"][:, :3]).clone(),
                  opacities=t(sc.opacities).reshape(-1, 1).clone(), colors=t(sc.colors_precomp).clone())
    for v in leaves.values():
        v.requires_grad_(True)
    color, radii, aux = dense_ref.render(sc.W, sc.H, sc.tanfovx, sc.tanfovy, t(sc.bg), t(sc.viewmatrix), t(sc.projmatrix),
                                         t(sc.campos), t(sc.means3D), leaves["means2D"], leaves["opacities"],
                                         colors_precomp=leaves["colors"], cov3D_precomp=t(sc.cov3D_precomp),
                                         state2d=(t(st["xy"]), leaves["conic"]))
    assert np.array_equal(radii.numpy(), fw["radii"])
    return color, leaves, aux


def _nine(grads):
    """The twin's gradients in the layout of oracle.SUMS.  The render backward keeps HALF of d / d conic_B (upstream's
    convention: the off-diagonal entry counted once per side of the symmetric matrix; or_preprocess_backward's formulas
    expect it so), autograd the whole."""
    m2, cn, op, cl = grads
    return np.concatenate([m2[:, :2].numpy(), cn.numpy() * np.array([1.0, 0.5, 1.0]), op.numpy().reshape(-1, 1), cl.numpy()], 1)


def _twin_include(sc, aux):
    inc = np.zeros((sc.H * sc.W, sc.P), bool)
    inc[:, aux["order"].numpy()] = aux["include"].numpy()
    return inc


VALIDATION = {"ladder": (gc.ladder, dict(n=40)), "wall": (gc.wall, dict(n_wall=8, n_back=30)), "edge": (gc.edge, dict(n_out=30, n_last=14, n_front=3, n_rest=6)),
              "plain": (_plain, {})}


@pytest.mark.parametrize("tag", sorted(VALIDATION))
def test_oracle_terms_lie_within_half_the_constants_of_the_float64_twin(oracle, tag):
    """See the module docstring: every element of the nine sums, no element exempt, at C0 / 2 and C1 / 2 and without the
    n_i part (the oracle adds its fp32 terms in double)."""
    maker, kw = VALIDATION[tag]
    seed, cloud, cam, sc, fw = _with_margins(oracle, maker, **kw)
    g = gc.pixel_gradients(tag)
    want = oracle.backward(sc, fw, g.numpy(), conditioning=True)
    color, leaves, aux = _twin(sc, fw)
    assert np.array_equal(_twin_include(sc, aux), oracle.included_pairs(sc, fw))  # the same pairs, before any number is compared
    grads = torch.autograd.grad((color * g.double()).sum(), list(leaves.values()))
    twin = _nine(grads)
    bound = gc.sum_bound(want, scale=0.5, with_n=False, front_to_back=False)
    r = gc.ratios(want["sums"], twin, bound)
    vis = want["cond_n"] > 0
    print("%s (seed %d): %d Gaussians with pairs of %d, largest |oracle - twin| / bound at half the constants: %.3g (per sum: %s)"
          % (tag, seed, vis.sum(), sc.P, r.max(), " ".join("%.2g" % x for x in r.max(0))))
    assert vis.sum() >= 20 and np.abs(twin).max() > 0
    assert (want["sums"][~vis] == 0).all() and (twin[~vis] == 0).all()
    assert r.max() <= 1.0, (tag, np.unravel_index(r.argmax(), r.shape), r.max())


@pytest.mark.parametrize("tag", sorted(gc.SCENES))
def test_absolute_sums_dominate_the_sums_and_leave_the_old_outputs_alone(oracle, tag):
    """On the four device scenes (in the product's tile-rectangle mode): A >= |sum| for every element (to the rounding of the
    fp32 terms), B >= A (Q + m >= 1), n = the number of included pairs; and oracle.backward gives the same bits with and
    without the new outputs."""
    cloud, cam = gc.SCENES[tag]()
    sc = _scene(cloud, cam, tile_rect=None)
    fw = oracle.forward(sc)
    g = gc.pixel_gradients(tag).numpy()
    old, new = oracle.backward(sc, fw, g), oracle.backward(sc, fw, g, conditioning=True)
    for k, v in old.items():
        assert (v is None and new[k] is None) or np.array_equal(v.view(np.uint32), new[k].view(np.uint32)), k
    A, B, s = new["cond_A"], new["cond_B"], new["sums"]
    assert (A * (1 + 8 * U) >= np.abs(s)).all()
    assert (B >= A).all() and (A >= 0).all()
    assert np.array_equal(new["cond_n"], oracle.included_pairs(sc, fw).sum(0))
    assert ((new["cond_n"] == 0) == (A.max(1) == 0)).all()


def test_absolute_sum_of_a_single_pair_is_the_magnitude_of_its_term(oracle):
    """One Gaussian that passes alpha >= 1 / 255 on one pixel only, black background, colour in one channel: the colour sum has
    A == |sum|, the six geometric sums A == (1 + alpha T) |sum| (the pair's own alpha T |col| is in Cabs; T = 1), B ==
    (Q + 1) A."""
    cloud, cam = helpers.cloud_and_camera(1, 16, 16, sh_degree=0, seed=0)
    f = 500.0 * 16 / 512.0
    cloud.xyz = torch.tensor([[(7.2 - 7.5) * 3.0 / f, (5.9 - 7.5) * 3.0 / f, 0.0]])
    cloud.scales = torch.full((1, 3), 1e-3)
    cloud.opacity = torch.tensor([[0.008]])
    cols = torch.tensor([[0.7, 0.0, 0.0]])
    sc = helpers.oracle_scene(cloud, cam, bg=(0.0, 0.0, 0.0), color_mode="precomp", colors=cols, cov_mode="cov", tile_rect=0)
    fw = oracle.forward(sc)
    assert int(oracle.included_pairs(sc, fw).sum()) == 1
    g = torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(1)).numpy()
    b = oracle.backward(sc, fw, g, conditioning=True)
    A, B, s = b["cond_A"][0], b["cond_B"][0], b["sums"][0]
    alpha = 1.0 - float(fw["image"]["final_T"].min())
    assert 1.0 / 255.0 <= alpha < 0.008 and b["cond_n"][0] == 1 and np.abs(s).min() > 0
    assert np.allclose(A[6:], np.abs(s[6:]), rtol=4 * U, atol=0)
    assert np.allclose(A[:6], (1.0 + alpha) * np.abs(s[:6]), rtol=16 * U, atol=0)
    co, xy = fw["geom"]["conic_opacity"][0].astype(np.float64), fw["geom"]["xy"][0].astype(np.float64)
    dx, dy = xy[0] - 7.0, xy[1] - 6.0
    Q = 0.5 * (abs(co[0]) * dx * dx + abs(co[2]) * dy * dy) + abs(co[1] * dx * dy)
    assert np.allclose(B[:7], (Q + 1.0) * A[:7], rtol=1e-12, atol=0)


def test_absolute_sums_are_not_below_the_twins_per_pixel_jacobian(oracle):
    """16 x 16, 24 Gaussians: sum over the pixels of |sum_c g_c dC_c / dtheta| from 256 backward passes of the float64 twin
    is what a sum of per-pixel contributions cannot have less condition than; the oracle's absolute form splits every
    pixel's contribution further (per channel, per addend), so A is at or above it."""
    Wd = Hd = 16
    seed = 0
    while True:
        cloud, cam = helpers.cloud_and_camera(24, Wd, Hd, sh_degree=3, seed=seed, scale_mul=2.0)
        cloud.opacity = cloud.opacity.clamp(max=0.9)
        sc = _scene(cloud, cam)
        fw = oracle.forward(sc, margin=True)
        if float(fw["image"]["margin"].min()) >= 1e-3:
            break
        seed += 1
    g = torch.randn(3, Hd, Wd, generator=torch.Generator().manual_seed(2))
    b = oracle.backward(sc, fw, g.numpy(), conditioning=True)
    color, leaves, aux = _twin(sc, fw)
    assert np.array_equal(_twin_include(sc, aux), oracle.included_pairs(sc, fw))
    per_pixel = (color * g.double()).sum(0).reshape(-1)
    total = np.zeros((sc.P, 9))
    for p in range(Wd * Hd):
        total += np.abs(_nine(torch.autograd.grad(per_pixel[p], list(leaves.values()), retain_graph=True)))
    vis = b["cond_n"] > 0
    low = (total / np.where(b["cond_A"] > 0, b["cond_A"], 1.0))[vis]
    print("seed %d: %d Gaussians with pairs; per-pixel Jacobian sum / A between %.3g and %.3g" % (seed, vis.sum(), low.min(), low.max()))
    assert vis.sum() >= 12 and (total[~vis] == 0).all()
    assert (b["cond_A"] * (1 + 1e-6) >= total).all()


@pytest.mark.parametrize("color_mode,cov_mode", [("precomp", "cov"), ("sh", "scale_rot")])
def test_eight_probe_jacobian_reproduces_the_derived_tensors(oracle, color_mode, cov_mode):
    """oracle.preprocess_jacobian: J_i s_i (J in fp32 from the probes, the product in double) against oracle.backward's own
    derived rows, within the chain's operation count C2 u |J_i| |s_i| (both sides are rounded fp32 chains of C2 / 2 each)."""
    cloud, cam = gc.ladder()
    sc = _scene(cloud, cam, tile_rect=None, color_mode=color_mode, cov_mode=cov_mode)
    fw = oracle.forward(sc)
    b = oracle.backward(sc, fw, gc.pixel_gradients("ladder").numpy(), conditioning=True)
    s32 = b["sums"].astype(np.float32).astype(np.float64)  # what or_preprocess_backward was given
    J = oracle.preprocess_jacobian(sc, fw)
    names = ["means3D", "cov3D_precomp"] + (["sh"] if color_mode == "sh" else []) + (["scales", "rotations"] if cov_mode == "scale_rot" else [])
    assert sorted(J) == sorted(names)
    for name in names:
        Jn = J[name].astype(np.float64)
        rows = np.einsum("pkj,pj->pk", Jn, s32)
        want = b[name].reshape(sc.P, -1).astype(np.float64)
        bound = gc.C2 * U * oracle.through_jacobian(Jn, np.abs(s32))
        r = gc.ratios(rows, want, bound)
        print("%s/%s %-14s largest |J s - row| / (C2 u |J||s|): %.3g" % (color_mode, cov_mode, name, r.max()))
        assert np.abs(want).max() > 0 and r.max() <= 1.0, name
        assert (Jn[:, :, 5] == 0).all()


def test_a_dropped_pair_is_rejected_by_the_bound_and_accepted_by_the_tensor_maximum_bar(oracle):
    """The gap, demonstrated on the Wall scene without a device: the Gaussian with the fewest pairs among those whose means2D
    row is below 1e-6 of the tensor's maximum loses one pair (forced to SKIP through the override table, forward and
    backward).  Every tensor of the altered result passes _bulk_close(tol=1e-5, frac=0.0), the bar of the suite's gradient
    tests; the per-Gaussian bound rejects it."""
    from test_gpu_parity import _bulk_close
    cloud, cam = gc.wall()
    sc = _scene(cloud, cam, tile_rect=None)
    fw = oracle.forward(sc)
    g = gc.pixel_gradients("wall").numpy()
    want = oracle.backward(sc, fw, g, conditioning=True)
    row = np.abs(want["means2D"]).max(1)
    cand = np.flatnonzero((want["cond_n"] > 0) & (row < 1e-6 * row.max()) & (row > 0))
    assert cand.size > 0
    i = int(cand[np.argmin(want["cond_n"][cand])])
    pid = int(np.flatnonzero(oracle.included_pairs(sc, fw)[:, i])[0])
    tile = (pid // sc.W // 16) * ((sc.W + 15) // 16) + (pid % sc.W) // 16
    r0, r1 = (int(x) for x in fw["binning"]["ranges"][tile])
    j = r0 + int(np.flatnonzero(fw["binning"]["point_list"][r0:r1] == i)[0])
    ov = oracle.Overrides([(pid << 32) | j], [1], [0.0])
    im = oracle.render_forward(sc, fw["geom"], fw["binning"], ov)
    altered = oracle.backward(sc, dict(fw, image=im, color=im["color"]), g, ov, conditioning=True)
    assert altered["cond_n"][i] == want["cond_n"][i] - 1
    J = oracle.preprocess_jacobian(sc, fw)
    rejected = []
    for name in ("means2D", "opacities", "colors_precomp", "means3D", "cov3D_precomp"):
        _bulk_close(altered[name], want[name], tol=1e-5, frac=0.0, name=name)  # today's bar: accepted
        bound = gc.direct_bound(want, name) if name in gc.DIRECT else gc.derived_bound(oracle, want, J[name])
        r = gc.ratios(altered[name].reshape(sc.P, -1), want[name].reshape(sc.P, -1), bound)
        print("Gaussian %d (%d pairs, means2D row %.3g of the maximum) without pair (pixel %d, entry %d): %-14s error / bound %.3g, "
              "error / tensor maximum %.3g" % (i, want["cond_n"][i], row[i] / row.max(), pid, j, name, r[i].max(),
                                              helpers.rel_to_max(altered[name], want[name])))
        if r[i].max() > 1.0:
            rejected.append(name)
    # (its colour row is off by 3e4 bounds.  The geometric rows of a Gaussian buried this deep, T ~ 1e-4 behind two dozen pairs, are
    # within the bound's front-to-back term: the kernel's own dL/dalpha there is a difference of numbers 1e4 times larger.)
    assert "colors_precomp" in rejected, rejected


def _front_to_back_opacity_sums(oracle, sc, fw, g, dtype):
    """The opacity sums with dL/dalpha formed as csrc/render_bwd.hip forms it (front to back, T (c . g) - Rem / (1 - alpha), Rem a
    running difference from out_color . g), every operation rounded to `dtype`, from the oracle's fp32 alpha and G; the
    per-Gaussian sums in double."""
    f32 = np.float32
    st, bn, im = fw["geom"], fw["binning"], fw["image"]
    inc = oracle.included_pairs(sc, fw)
    dot = lambda a, b: dtype(dtype(dtype(a[0] * b[0]) + dtype(a[1] * b[1])) + dtype(a[2] * b[2]))
    out = np.zeros(sc.P)
    for pid in range(sc.W * sc.H):
        px, py = pid % sc.W, pid // sc.W
        r0, r1 = bn["ranges"][(py // 16) * ((sc.W + 15) // 16) + px // 16]
        gp = g[:, py, px].astype(dtype)
        T, rem = dtype(1.0), dot(im["color"][:, py, px].astype(dtype), gp)
        for j in range(r0, r1):
            i = bn["point_list"][j]
            if not inc[pid, i]:
                continue
            co, dx, dy = st["conic_opacity"][i], f32(st["xy"][i, 0] - f32(px)), f32(st["xy"][i, 1] - f32(py))
            G = f32(np.exp(f32(f32(-0.5) * f32(f32(co[0] * dx * dx) + f32(co[2] * dy * dy)) - f32(co[1] * dx * dy))))
            alpha = dtype(min(f32(0.99), f32(co[3] * G)))
            cg = dot(st["rgb"][i].astype(dtype), gp)
            rem = dtype(np.float64(rem) - np.float64(cg) * np.float64(dtype(alpha * T)))  # one FMA
            one_m = dtype(dtype(1.0) - alpha)
            dL_dalpha = dtype(dtype(T * cg) - dtype(rem * dtype(dtype(1.0) / one_m)))
            T = dtype(T * one_m)
            out[i] += float(G) * float(dL_dalpha)
    return out


def test_front_to_back_recurrence_in_fp32_needs_the_bounds_third_term_and_fits_it(oracle):
    """Why the device's bound has C3 cond_R (tests/grad_conditioning.py): the kernel's dL/dalpha recurrence evaluated in fp32
    on the CPU, on the Wall scene, against the same recurrence in float64 (which agrees with the oracle's back-to-front sums).
    Without the term the fp32 recurrence exceeds the bound several times over, only where A_i is small; with it, it does not.
    Measured: without 8.1 (decade 1e-5 of A_i; 0.5 in decade 1e-2, 0.06 from 1 up), with 0.013."""
    cloud, cam = gc.wall()
    sc = _scene(cloud, cam, tile_rect=None)
    fw = oracle.forward(sc)
    g = gc.pixel_gradients("wall").numpy()
    want = oracle.backward(sc, fw, g, conditioning=True)
    lo, hi = (_front_to_back_opacity_sums(oracle, sc, fw, g, t) for t in (np.float32, np.float64))
    s, A = want["sums"][:, 5], want["cond_A"][:, 5]
    assert np.abs(hi - s).max() <= 1e-6 * np.abs(s).max()  # the same sums, the other way round
    vis = want["cond_n"] > 0
    without = gc.ratios(lo, hi, gc.sum_bound(want, with_n=False, front_to_back=False)[:, 5])[vis]
    with_r = gc.ratios(lo, hi, gc.sum_bound(want, with_n=False)[:, 5])[vis]
    print("fp32 front-to-back recurrence, error / bound: without cond_R %.3g (A_i >= 1: %.3g), with %.3g"
          % (without.max(), without[A[vis] >= 1.0].max(), with_r.max()))
    assert without.max() > 2.0 and without[A[vis] >= 1.0].max() <= 1.0
    assert with_r.max() <= 1.0
