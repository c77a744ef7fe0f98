"""Same bits across builds: calls every entry point that shares the fixed-order primitives of csrc/ordered_sum.h,
csrc/sorted_lists.h and csrc/slab.h (and the workspace carver) on fixed seeded inputs and prints, per output tensor, its
name, shape and the SHA-256 of its bytes.  The inputs are the smallest at which each primitive can go wrong: float4 tails,
more partials than one sweep of a final kernel, ragged last slabs, hub rows and long gaps in the sorted lists.

Usage:  python tools/module_digests.py > a.txt;  GSPLAT_LIB_PATH=<other build> python tools/module_digests.py > b.txt
        diff a.txt b.txt      (empty: the two libraries compute the same bits; each run in a process of its own)
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "3dgs-avatar-release_amd"))
import torch  # noqa: E402

from gsplat_mi355 import _lib, aiap, densify, hashgrid, nonrigid, optim, skinning, texture  # noqa: E402
from gsplat_mi355.camera import orbit_camera  # noqa: E402
from gsplat_mi355.debug import forward_state  # noqa: E402
from gsplat_mi355.knn import knn_points  # noqa: E402
from gsplat_mi355.render import Pipe, bce_mask_loss, l1_loss, render, ssim  # noqa: E402
from gsplat_mi355.scenes import GaussianCloud, synthetic_cloud  # noqa: E402
from simple_knn._C import distCUDA2  # noqa: E402

DEV = torch.device("cuda:0")
GEN = torch.Generator().manual_seed(20240611)


def rand(*shape, normal=False, grad=False):
    t = (torch.randn(*shape, generator=GEN) if normal else torch.rand(*shape, generator=GEN)).to(DEV)
    return t.requires_grad_(grad)


def out(name, t):
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu().numpy()
    print("%-44s %-22s %s" % (name, tuple(t.shape), hashlib.sha256(t.tobytes()).hexdigest()), flush=True)


def grads(prefix, loss, leaves):
    for t in leaves.values():
        t.grad = None
    loss.backward()
    for k, t in leaves.items():
        out("%s.d_%s" % (prefix, k), t.grad)


def losses():
    for n in (4 * 256 * 3 + 3, 4 * 256 * 257 + 2):  # float4 tail; more than 256 partials (the final kernel loops twice)
        x, y = rand(n, grad=True), rand(n)
        for name, fn in (("l1", l1_loss), ("bce", bce_mask_loss)):
            v = fn(x, y)
            out("%s[%d].loss" % (name, n), v)
            grads("%s[%d]" % (name, n), v, {"x": x})
    a, b = rand(3, 301, 1003, grad=True), rand(3, 301, 1003)  # 3 x 10 x 32 = 960 partials, sides not multiples of 32
    v = ssim(a, b)
    out("ssim.value", v)
    grads("ssim", v, {"img1": a})


def rasterizer():
    cloud = synthetic_cloud(300, sh_degree=3, seed=0, device=DEV)
    cam, bg = orbit_camera(0, 1024, 528, device=DEV), torch.zeros(3, device=DEV)
    leaves = {f: getattr(cloud, f).requires_grad_(True) for f in GaussianCloud.FIELDS}
    pkg = render(cam, cloud, Pipe(), bg, l1_target=rand(3, 528, 1024))  # 64 x 33 tiles: 8448 quadrant partials
    out("fused_l1.loss", pkg.l1)
    out("fused_l1.image", pkg.render)
    grads("fused_l1", pkg.l1, leaves)
    out("fused_l1.d_means2D", pkg.viewspace_points.grad)
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    import math
    st = GaussianRasterizationSettings(
        image_height=528, image_width=1024, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg,
        scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3,
        campos=cam.camera_center, prefiltered=False, debug=False)
    for sort in (1, 0):  # the bucket depth sort, then the radix sort's path (PairSort's accessors in capi.hip)
        _lib.tuning("depth_sort", sort)
        with torch.no_grad():
            fs = forward_state(st, cloud.xyz.detach(), cloud.opacity.detach(), shs=cloud.shs.detach(),
                               scales=cloud.scales.detach(), rotations=cloud.rotations.detach())
        out("forward[depth_sort=%d].image" % sort, fs["color"])
        out("forward[depth_sort=%d].point_list" % sort, fs["binning"]["point_list"])
    _lib.tuning("depth_sort", 1)


def lists():
    N, K = 1000, 5
    idx = torch.randint(0, N, (N, K), generator=GEN)
    idx[:200, 1] = 0                                  # a hub: 200 rows point at row 0 (above AIAP_HEAVY)
    idx[idx.ge(300) & idx.lt(400)] = 450              # nobody points at rows 300 .. 399: a gap above a wave
    idx[7, 2], idx[500, 4], idx[999, 1] = -1, N, N + 5  # a few out-of-range indices
    idx = idx.to(DEV)
    xs = {k: rand(N, d, normal=True, grad=True) for k, d in (("xc0", 3), ("xd0", 3), ("xc1", 6), ("xd1", 6))}
    l0, l1 = aiap._AiapFunction.apply(idx, xs["xc0"], xs["xd0"], xs["xc1"], xs["xd1"])
    out("aiap.loss0", l0)
    out("aiap.loss1", l1)
    grads("aiap", l0 + 100.0 * l1, xs)
    one = {"xc": rand(1, 3, grad=True), "xd": rand(1, 3, grad=True)}
    v = aiap.aiap_loss(one["xc"], one["xd"], nn_ix=torch.zeros(1, K, dtype=torch.int64, device=DEV))
    out("aiap[N=1].loss", v)
    grads("aiap[N=1]", v, one)
    for F in (1, 2, 8):
        cfg = hashgrid.parse_config(3, dict(n_levels=4, n_features_per_level=F, log2_hashmap_size=10))
        n_params = hashgrid.levels(cfg)[3]
        # 2500 points inside one level-0 cell (eight lists of three HG_CHUNKs each), 500 in a small cube (few entries of
        # the coarse levels: gaps of more than a wave of empty entries between the lists)
        pts = torch.cat([rand(2500, 3) * 0.025 + 0.405, rand(500, 3) * 0.1 + 0.7])
        g = rand(3000, 4 * F, normal=True)
        for want_x, want_p in ((False, True), (True, False), (True, True)):
            x, th = pts.clone().requires_grad_(want_x), (rand(n_params, normal=True) * 0.1).requires_grad_(want_p)
            tag = "hashgrid[F=%d,dx=%d,dp=%d]" % (F, want_x, want_p)
            o = hashgrid.hashgrid_encode(x, th, cfg)
            out(tag + ".out", o)
            grads(tag, (o * g).sum(), dict(([("x", x)] if want_x else []) + ([("params", th)] if want_p else [])))
    for P in (100, 5000):
        p = rand(P, 3, normal=True)
        r = knn_points(p, p, K=5)
        out("knn_points[%d].dists" % P, r.dists)
        out("knn_points[%d].idx" % P, r.idx)
        out("knn_dist2[%d]" % P, distCUDA2(p))


def densification():
    n = 256 * 4 + 1  # one block of the classify / map kernels + 1
    r = lambda *s: rand(*s, normal=True)
    params = {"xyz": r(n, 3), "f_dc": r(n, 1, 3), "f_rest": r(n, 15, 3), "opacity": r(n, 1) * 0.9 + 0.5,
              "scaling": r(n, 3) * 1.5 - 4.6, "rotation": r(n, 4)}
    stats = {"xyz_gradient_accum": torch.exp(r(n, 1) * 0.7) * 0.0002, "denom": torch.full((n, 1), 1.0, device=DEV),
             "max_radii2D": rand(n) * 40.0}
    plan = densify.plan_densify(params, stats, grad_threshold=0.0002, percent_dense=0.01, extent=1.0, min_opacity=0.05,
                                max_screen_size=20)
    out("densify.flags", plan.flags)
    out("densify.row_map", torch.stack(plan.row_map()))
    new, new_stats = densify.apply_plan(plan, params, None, stats, noise=r(n, 2, 3))
    for k in densify.GROUPS:
        out("densify.new_" + k, new[k])


def skin():
    for n in (256 * 70 + 5, 5):  # more than 64 block partials (runs of unequal length) and a ragged last slab; one short block
        tfs = rand(24, 4, 4, normal=True, grad=True)
        for C, weights in ((25, False), (24, False), (24, True)):
            leaves = {"w": rand(n, C, normal=True, grad=True), "tfs": tfs, "xyz": rand(n, 3, normal=True, grad=True),
                      "rot": rand(n, 4, normal=True, grad=True)}
            xb, rb, T = skinning.linear_blend_skinning(leaves["w"], tfs, leaves["xyz"], leaves["rot"], weights=weights)
            tag = "skinning[n=%d,C=%d,weights=%d]" % (n, C, weights)
            out(tag + ".xyz", xb); out(tag + ".rot", rb); out(tag + ".T_fwd", T)
            grads(tag, (xb * rand(n, 3, normal=True)).sum() + (rb * rand(n, 3, 3, normal=True)).sum(), leaves)
        for C in (25, 24):
            lg, tg = rand(n, C, normal=True, grad=True), torch.softmax(rand(n, 24, normal=True), dim=1)
            v = skinning.skinning_mse_loss(lg, tg)
            out("skin_loss[n=%d,C=%d].loss" % (n, C), v)
            grads("skin_loss[n=%d,C=%d]" % (n, C), v, {"logits": lg})


def tails():
    n = texture.rows_per_block(79) * 300 + 7  # more than 256 block partials of the latent sum; slab of 7 x 79 floats
    lv = {"dc": rand(n, 1, 1, normal=True, grad=True), "rest": rand(n, 31, 1, normal=True, grad=True),
          "xyz": rand(n, 3, normal=True, grad=True), "feature": rand(n, 16, normal=True, grad=True),
          "latent": rand(1, 16, normal=True, grad=True)}
    T = torch.zeros(n, 4, 4, device=DEV)
    T[:, :3, :3] = torch.linalg.qr(rand(n, 3, 3, normal=True).cpu())[0].to(DEV)
    noise = torch.linalg.qr(torch.randn(3, 3, generator=GEN))[0]
    inp = texture.color_mlp_input([lv["dc"], lv["rest"]], lv["xyz"], torch.tensor([0.5, -1.0, 2.5], device=DEV), 3,
                                  fwd_transform=T, view_noise=noise, after=[lv["feature"]], latent=lv["latent"])
    out("texture.input", inp)
    grads("texture", (inp * rand(n, 79, normal=True)).sum(), lv)
    for F in (0, 16):
        D = 10 + F
        n = min((8192 // D) & ~3, 256) * 300 + 7
        lv = {"deltas": rand(n, D, normal=True, grad=True), "xyz": rand(n, 3, normal=True, grad=True),
              "scaling": rand(n, 3, normal=True, grad=True), "rotation": rand(n, 4, normal=True, grad=True)}
        xo, so, ro, feat, ls = nonrigid.nonrigid_apply(lv["deltas"], lv["xyz"], lv["scaling"], lv["rotation"])
        tag = "nonrigid[F=%d]" % F
        out(tag + ".xyz", xo); out(tag + ".scaling", so); out(tag + ".rotation", ro)
        total = (xo * rand(n, 3, normal=True)).sum() + (so * rand(n, 3, normal=True)).sum() + (ro * rand(n, 4, normal=True)).sum()
        if feat is not None:
            out(tag + ".feature", feat)
            total = total + (feat * rand(n, F, normal=True)).sum()
        for k in sorted(ls):
            out("%s.%s" % (tag, k), ls[k])
            total = total + ls[k]
        grads(tag, total, lv)
    ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in (2048 * 200 + 3, 2048 * 60 + 1, 777)]  # 263 chunks
    for p in ps:
        p.grad = rand(p.numel() + 1, normal=True)[1:] if p.numel() == 777 else rand(p.numel(), normal=True)  # one unaligned
    out("grad_norm.total", optim.clip_grad_norm_(ps, 0.1))
    for k, p in enumerate(ps):
        out("grad_norm.scaled[%d]" % k, p.grad)


if __name__ == "__main__":
    for part in (losses, rasterizer, lists, densification, skin, tails):
        part()
        torch.cuda.synchronize()
