"""The streaming kernels around the rasterizer at the sizes where their code paths change: FusedAdam across chunk tails,
launches, groups and step numbers; densify_stats at block edges; the L1 / BCE losses below one float4 and past the capped
grid; SSIM on images smaller than its window or its tile, and one row or column into a second tile; operands that do
not start on a 16-byte boundary.  Each against a plain high-precision restatement (oracle/gs_oracle.py, torch float64 on
the CPU) at the bars of the existing tests in test_gpu_parity.py."""
import math

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- FusedAdam

COUNTS = [0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 45 * 1001]


def _grad(rs, n, k):
    """Magnitudes over 1e-12 .. 1e3 with exact zeros: per tensor a decade (one tensor spans the whole range per element)."""
    if k % 7 == 6:
        mag = 10.0 ** rs.uniform(-12, 3, n)
    else:
        mag = 10.0 ** (float([-12, -9, -6, -3, 0, 3][k % 6]) + rs.uniform(-1, 1, n))
    g = rs.normal(size=n) * mag
    g[::5] = 0.0
    if k == 4:
        g[:] = 0.0
    return g.astype(np.float32)


def test_fused_adam_across_chunks_launches_groups_and_step_numbers(oracle):
    """One FusedAdam: a group of 24 parameters, 22 of them on one step number (two launches of at most
    GS_ADAM_MAX_TENSORS), with every chunk-tail size, two empty ones and one without a gradient among them; a second
    group with other betas / eps; parameters whose `step` starts at 7 and at 29 999 (their own launches).  Three steps against oracle.adam_step (float64) and
    torch.optim.Adam on the CPU: 2e-6 of each tensor's maximum."""
    from gsplat_mi355 import _lib
    from gsplat_mi355.optim import FusedAdam
    rs = np.random.default_rng(21)
    # (count, group, preloaded step or None, has a gradient)
    spec = [(c, 0, None, True) for c in COUNTS] + [(0, 0, None, True)] + [(c, 0, None, True) for c in COUNTS[1:]]
    spec.insert(11, (1025, 0, 3, False))                       # no gradient, in the middle of the big group
    spec += [(4097, 0, 7, True), (1025, 1, None, True), (3, 1, None, True), (45 * 1001, 1, None, True),
             (257, 1, 29999, True)]
    assert sum(1 for s in spec if s[1] == 0 and s[3] and s[2] is None) > _lib.GS_ADAM_MAX_TENSORS
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15), dict(lr=5e-3, betas=(0.8, 0.99), eps=1e-8)]
    init = [rs.normal(size=c).astype(np.float32) for c, _, _, _ in spec]
    pre = [None if s is None else (rs.normal(size=c).astype(np.float32) * 1e-2, rs.random(c).astype(np.float32) * 1e-4)
           for c, _, s, _ in spec]

    def make(cls, dev):
        ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in init]
        opt = cls([dict(params=[p for p, s in zip(ps, spec) if s[1] == gi], name=str(gi), **g) for gi, g in enumerate(groups)],
                  lr=0.0)
        for p, (c, _, s, _), st in zip(ps, spec, pre):
            if s is not None:
                opt.state[p] = {"step": torch.tensor(float(s)), "exp_avg": torch.from_numpy(st[0]).to(dev),
                                "exp_avg_sq": torch.from_numpy(st[1]).to(dev)}
        return ps, opt

    mine, o_mine = make(FusedAdam, DEV)
    ref, o_ref = make(torch.optim.Adam, "cpu")
    orc = [(a.astype(np.float64), *(np.zeros(a.shape) if st is None else st[j].astype(np.float64) for j in (0, 1)))
           for a, st in zip(init, pre)]
    for t in range(1, 4):
        grads = [_grad(rs, c, k) for k, (c, _, _, _) in enumerate(spec)]
        for pm, pr, g, s in zip(mine, ref, grads, spec):
            pm.grad = torch.from_numpy(g).to(DEV) if s[3] else None
            pr.grad = torch.from_numpy(g) if s[3] else None
        o_mine.step()
        o_ref.step()
        for k, (pm, pr, g, s) in enumerate(zip(mine, ref, grads, spec)):
            c, gi, s0, has = s
            hp = groups[gi]
            got = pm.detach().cpu().numpy().astype(np.float64)
            if not has:  # untouched: the bits and the preloaded state
                assert np.array_equal(got, init[k].astype(np.float64)), k
                st = o_mine.state[pm]
                assert float(st["step"]) == s0 and np.array_equal(st["exp_avg"].cpu().numpy(), pre[k][0]), k
                assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), pre[k][1]), k
                continue
            step = (s0 or 0) + t
            orc[k] = oracle.adam_step(*orc[k][:1], g, *orc[k][1:], hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], step)
            q, m, v = orc[k]
            st = o_mine.state[pm]
            assert set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == step, k
            assert float(o_ref.state[pr]["step"]) == step
            assert got.shape == (c,)
            if c == 0:
                continue
            scale = np.abs(q).max()
            assert np.abs(got - q).max() <= 2e-6 * scale, (k, c, t)
            assert np.abs(got - pr.detach().numpy()).max() <= 2e-6 * scale, (k, c, t)
            assert np.abs(st["exp_avg"].cpu().numpy() - m).max() <= 2e-6 * max(np.abs(m).max(), 1e-30), (k, c, t)
            assert np.abs(st["exp_avg_sq"].cpu().numpy() - v).max() <= 2e-6 * max(np.abs(v).max(), 1e-30), (k, c, t)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100001])
def test_densify_stats_at_block_edges(oracle, n):
    from gsplat_mi355.optim import densify_stats
    rng = np.random.default_rng(n)
    radii = rng.integers(-1, 40, size=n).astype(np.int32)
    radii[radii < 0] = 0
    radii[-1] = 7  # the last element is visible
    vg = rng.normal(size=(n, 3)).astype(np.float32)
    mr, acc, dn = (rng.random(n).astype(np.float32) * 20 for _ in range(3))
    want = oracle.densify_stats(radii, vg, mr, acc, dn)
    t = [torch.from_numpy(a).to(DEV) for a in (mr, acc.reshape(n, 1), dn.reshape(n, 1))]
    densify_stats(torch.from_numpy(radii).to(DEV), torch.from_numpy(vg).to(DEV), *t)
    for got, w in zip(t, want):
        assert np.array_equal(got.cpu().numpy().reshape(-1), w)


# ---- losses

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 4 * 256 * 1024 + 3, 3 * 1024 * 1024 + 7])
def test_l1_loss_tail_and_capped_grid(oracle, n):
    """n < 4 (no float4 at all: block 0 does everything), n mod 4 != 0 tails, and the grid capped at L1_MAX_BLOCKS
    (the last size strides three times over the float4s).  Value 1e-6 relative, gradient bit-exact."""
    from gsplat_mi355.render import l1_loss
    g = torch.Generator().manual_seed(n)
    a, b = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if n >= 5:
        a[0] = b[0]  # sign(0) = 0, in the float4 part and (n mod 4 >= 2) in the tail; the last element differs
    if n % 4 >= 2 and n >= 6:
        a[-2] = b[-2]
    want, want_grad = oracle.l1_loss(a.numpy(), b.numpy())
    x = a.to(DEV).requires_grad_(True)
    loss = l1_loss(x, b.to(DEV))
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want, rel=1e-6)
    assert np.array_equal(x.grad.cpu().numpy(), want_grad)


@pytest.mark.parametrize("n", [1, 5, 12707, 1100003])
def test_bce_mask_loss_tail_and_capped_grid(n):
    """Against torch float64 on the CPU: value 2e-6 relative, gradient 1e-5 of its maximum, zero where clamped."""
    import torch.nn.functional as F
    from gsplat_mi355.render import bce_mask_loss
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g)
    if n >= 5:
        x[0], x[-1] = 0.0, 1.0  # below and above the clamp
    y = (torch.rand(n, generator=g) > 0.4).float()
    xd = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy(torch.clamp(xd, 1.0e-3, 1.0 - 1.0e-3), y.double())
    (3.0 * ref).backward()
    xg = x.to(DEV).requires_grad_(True)
    loss = bce_mask_loss(xg, y.to(DEV))
    (3.0 * loss).backward()
    assert float(loss.detach()) == pytest.approx(float(ref.detach()), rel=2e-6)
    want, got = xd.grad.numpy(), xg.grad.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    if n >= 5:
        assert got[0] == 0 and got[-1] == 0


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 3), (1, 1, 300), (1, 11, 11), (3, 32, 32), (3, 33, 33), (4, 45, 77),
                                   (2, 33, 600)])
def test_ssim_small_images_and_tile_edges(oracle, shape):
    """Images smaller than the 11-tap window and the 42 x 42 halo tile, exactly one tile, one row and column into a
    second tile, C other than 1 and 3.  Against oracle.ssim: value 1e-5 absolute, gradient 1e-4 of its maximum."""
    from gsplat_mi355.render import ssim
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    b = (a + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
    want, want_grad = oracle.ssim(a.numpy(), b.numpy())
    x = a.to(DEV).requires_grad_(True)
    val = ssim(x, b.to(DEV))
    (0.2 * (1.0 - val)).backward()
    assert float(val.detach()) == pytest.approx(want, abs=1e-5)
    got = x.grad.cpu().numpy() / -0.2
    assert np.abs(got - want_grad).max() <= 1e-4 * np.abs(want_grad).max()
    assert float(ssim(a.to(DEV), b.to(DEV))) == float(val.detach())


# ---- operands that do not start on a 16-byte boundary

def test_l1_loss_of_views_off_a_16_byte_boundary():
    """img[1:] of a (3, H, W) image with H W odd starts 4 bytes past a boundary; the kernel reads float4s, so the wrapper
    copies it: the same loss bits and gradient bits as aligned copies, the gradient delivered to the view."""
    from gsplat_mi355 import _lib
    from gsplat_mi355.render import l1_loss
    H, W = 17, 31
    g = torch.Generator().manual_seed(3)
    img = torch.rand(3, H, W, generator=g).to(DEV).requires_grad_(True)
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    assert not _lib.is_aligned(img[1:]) and not _lib.is_aligned(gt[1:]) and img[1:].is_contiguous()
    loss = l1_loss(img[1:], gt[1:])
    loss.backward()
    x = img.detach()[1:].clone().requires_grad_(True)
    want = l1_loss(x, gt[1:].clone())
    want.backward()
    assert float(loss.detach()) == float(want.detach())
    assert torch.equal(img.grad[1:], x.grad) and not img.grad[0].any()
    # one misaligned operand at a time
    assert float(l1_loss(x.detach(), gt[1:])) == float(want.detach())
    assert float(l1_loss(img.detach()[1:], gt[1:].clone())) == float(want.detach())


def test_quaternion_views_off_a_16_byte_boundary():
    """build_covariance_from_scaling_rotation and the rasterizer read quaternions as float4 (the C ABI refuses an
    unaligned pointer): a contiguous (N, 4) view one float into its storage gives the bits of an aligned copy, values and
    gradients."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gsplat_mi355 import _lib
    from gsplat_mi355.prepass import build_covariance_from_scaling_rotation
    n, W, H = 1500, 96, 64
    cloud, cam = helpers.cloud_and_camera(n, W, H, sh_degree=1, seed=4)
    scales = cloud.scales.to(DEV)
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(3, device=DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(DEV),
        projmatrix=cam.full_proj_transform.to(DEV), sh_degree=1, campos=cam.camera_center.to(DEV), prefiltered=False,
        debug=False)

    def quaternions(offset):
        """A leaf whose (N, 4) view starts `offset` floats into it."""
        store = torch.zeros(4 * n + offset, device=DEV)
        store[offset:] = cloud.rotations.reshape(-1).to(DEV)
        store.requires_grad_(True)
        q = store[offset:].view(n, 4)
        assert q.is_contiguous() and _lib.is_aligned(q) == (offset == 0)
        return store, q

    def run(offset):
        store, q = quaternions(offset)
        cov = build_covariance_from_scaling_rotation(scales, 1.0, q)
        (cov * torch.linspace(-1, 1, 6, device=DEV)).sum().backward()
        g_cov = store.grad[offset:].clone()
        store, q = quaternions(offset)
        color, radii = GaussianRasterizer(settings)(means3D=cloud.xyz.to(DEV), means2D=torch.zeros(n, 3, device=DEV),
                                                    opacities=cloud.opacity.to(DEV), shs=cloud.shs.to(DEV),
                                                    scales=scales, rotations=q)
        color.sum().backward()
        return cov.detach(), g_cov, color.detach(), radii, store.grad[offset:].clone()

    got, want = run(1), run(0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(want[1].abs().max()) > 0 and float(want[4].abs().max()) > 0
