"""The rasterizer's options in combination, against ONE float64 autograd twin of the whole call (oracle/dense_ref.py with
`antialiasing`, aux["invdepth"], aux["opacity"]): antialiasing x head (plain, with_opacity, with_invdepth) x l1_target x
inputs ((shs, scales + rotations), (colors_precomp, cov3D_precomp)) x scale_modifier (1.0, 0.7) x both tile_rect modes,
through the public GaussianRasterizer, over a non-black background.  Every option has a thorough test of its own
(test_gpu_antialiasing.py, test_gpu_invdepth.py, test_gpu_parity.py, test_gpu_cameras.py); what is tested here is that
they compose: one render_bwd launch carries the L1 prologue, the second image and the opacity channel, gaussian_bwd adds
the antialiasing chain, second_colors.hip forms dL_dcolors of the second image and the wrapper closes the chain through z.

Scene: helpers.cloud_and_camera(512, 64, 48, sh_degree=3, seed=99, frame=40) (the scene of test_gpu_invdepth.py's
test_gradient_through_z_against_float64_autograd -- its view matrix has x and z components in column 2 -- at another
cloud seed: see "Set aside" below) joined by the three hand-placed Gaussians of test_gpu_antialiasing._scene, re-placed
for this image: scale 1e-6 (the clamp of s), centre half a pixel inside the right border, behind the near plane -- 515
Gaussians, 4 x 3 tiles; background (0.3, 0.6, 0.1).  A second camera, helpers.posed_camera("inside"), sits in the cloud.

Reference: one dense_ref.render pass per (camera, antialiasing, inputs, scale_modifier), cached; the loss is linear in
the images' upstream gradients, so the pass is differentiated once per image (colour given gC, the L1 term, opacity given
gO, inverse depth given gD) and a case's reference is the combination its loss names.  gC, gO, gD are fixed random
images scaled by 1e-4 so that the L1 term (0.7 mean |colour - gt|: +-0.7 / 9216 per value) is a visible share of every
tensor.  gt = clip(render64 +- u, 0, 1), u uniform in [0.05, 0.3], resampled until every |render64 - gt| >= 0.01: with
the image within 1e-5 of float64 the sign of (colour - gt) is the same decision on both sides (the margin is asserted).

Bars.  Images 1e-5 absolute (test_gpu_parity.py, test_gpu_invdepth.py).  l1: relative 2e-6 against the float64 mean of
the device's own image (the bar of test_l1_fused_into_the_rasterizer...), and 1e-5 absolute against the twin's value
(|mean|a - gt| - mean|b - gt|| <= max|a - b|, the image bar).  Gradients: |delta| <= 1e-5 max|g| per tensor, with the
attribution rule of test_gpu_invdepth.py (helpers.undecided_pairs on the effective opacities; at most 2 % of the visible
Gaussians).  Each crossed-in term -- the antialiasing chain, the chain through z, the L1 part, the opacity image's part --
is asserted, on the float64 side, to exceed 1000 x the bar of the tensor it lands in: a kernel that dropped it fails.
One term cannot be raised to that by scaling an upstream gradient, because it is proportional to the same dL/do' as the
rest of its tensor: the antialiasing chain into means3D (s depends on the position only through the projection's
Jacobian) is 190 to 1330 x the bar on the orbit scene, and under the inside camera (footprints of tens of pixels, s
within 1e-3 of 1) the whole chain is 25 to 31 x (means3D) and 150 to 260 x (scales, rotations, cov3D) the bar.  There
the assertion is 10 x the bar -- a dropped term still misses the bar tenfold; everywhere else it is 1000 x.

Fused against separate L1 (l1_target against gsplat_mi355.render.l1_loss on the returned image): bit for bit for every
head and both antialiasing values.  Both form g = dL_dpix + sign(colour - gt) w / (3 H W) per value in fp32 -- the
separate path in the loss kernel and autograd's accumulation, the fused one in render_bwd's pixel prologue -- and feed the
same launches; a loss without a direct colour gradient compares NULL dL_dpix with a gradient image of the L1 term alone.

render(): a call that carries l1_target takes no geometry from the cache, but it still OFFERS its own; the opacity pass
behind Pipe(invdepth=True) therefore is a cache hit also with l1_target (1 hit, asserted), and none is possible with
fuse_opacity (one call).

Set aside.  The cap -- 2 % of the visible Gaussians: 10 of 514 on the orbit scene, 4 of 218 from inside the cloud -- is a
condition on the references alone (asserted by every case, computed on the CPU).  Seed 2 flags 16 Gaussians at
scale_modifier 1; the seeds were tried in order, with both cameras, and 99 is the first at which no reference exceeds its
cap.  Flagged there (undecided pairs = Gaussians, of the pairs tested): orbit, scale_modifier 1.0: 8 of 0.83 M with and
without antialiasing; 0.7: 6 or 7 without (one pair lies 3e-7 from the window's edge, and the cloud's scales differ in the
last fp32 bit between hosts), 8 with, of 0.60 M; inside: 4 of 0.41 M (the next pair is 1.6e-5 outside the window).

Measured on an MI355X, 132 cases, 5.7 s in all, the ten float64 references 2.6 s of it: NO Gaussian over the bar anywhere,
so none set aside.  Largest error as a share of the tensor's maximum, over all cases: means3D 3.1e-6, means2D 1.8e-6,
opacities 1.1e-6, scales 2.1e-6, rotations 3.6e-6, cov3D_precomp 3.7e-6, shs 7.5e-7, colors_precomp 5.8e-7; through
render() up to 1.5e-6 (scales); the long lists, device against device, up to 6.5e-7.  Images within 6.4e-7 of float64 on
the orbit scene and 2.0e-6 from inside the cloud; l1 equal to the float64 mean of the device's image to 8 digits.
Crossed-in terms against the bar of their tensor (smallest and largest multiple over the cases): L1 18000 to 186000,
opacity image 18700 to 86000, inverse-depth image 39000 to 155000, chain through z 6000 to 45000, colour image 31000 to
196000; antialiasing chain into scales 260 (inside) to 90000, rotations 250 (inside) to 5100, cov3D 310 (inside) to
115000, means3D 25 (inside), 190 to 1330 (orbit); s on dL/do 39 (inside) to 6500.  A wrapper that drops the fused L1 when
the inverse-depth gradient is present fails 17 of the 26 cases that use both."""
import functools
import math

import numpy as np
import pytest
import torch

import helpers
from test_gpu_antialiasing import _effective, tile_rect  # noqa: F401
from test_gpu_invdepth import BATCH, PARITY, _assert_bar, _formulation_c, _one_pass

pytestmark = pytest.mark.gpu

N0, W, H = 512, 64, 48
SEED = 99         # the first cloud seed (2, 3, ...) at which no float64 reference flags more Gaussians than its cap
CLAMP, BORDER, BEHIND = N0, N0 + 1, N0 + 2   # rows of the hand-placed Gaussians
BG = (0.3, 0.6, 0.1)
DT = torch.float64
G_SCALE = 1e-4    # on gC, gO, gD (unit normal): the L1 term's +-0.7 / (3 H W) = 7.6e-5 per value is then of their size
L1_WEIGHT = 0.7
GD_SCALE = 4.0    # on gD beside that: inverse depths are ~0.3, so that the image's part matches the others'
MARGIN = 0.01     # every |render64 - gt| is at least this: 1000 x the image bar
VISIBLE = 1000.0  # a crossed-in term exceeds this many times the bar of the tensor it lands in
WEAK = 10.0       # ... except the antialiasing chain where no upstream gradient can raise it (module docstring)
INPUTS = {"sh": ("shs", "scales", "rotations"), "precomp": ("colors_precomp", "cov3D_precomp")}
COV = {"sh": ("scales", "rotations"), "precomp": ("cov3D_precomp",)}
COLOR = {"sh": "shs", "precomp": "colors_precomp"}


@functools.lru_cache(maxsize=None)
def _scene(pose="orbit"):
    cloud, cam = helpers.cloud_and_camera(N0, W, H, sh_degree=3, seed=SEED, frame=40)
    V = cam.world_view_transform.numpy().astype(np.float64)
    assert abs(V[0, 2]) > 0.3 and abs(V[2, 2]) > 0.3
    fx, fy = W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5))
    # (as test_gpu_antialiasing._scene; the clamped one on the centre of pixel (34, 22))
    view_pts = np.array([[(34.5 - W / 2) * 3.0 / fx, (22.5 - H / 2) * 3.0 / fy, 3.0],
                         [(W / 2 - 0.5) * 3.0 / fx, 0.02, 3.0],
                         [0.0, 0.0, 0.1]])
    world = (view_pts - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    q = torch.randn(3, 4, generator=torch.Generator().manual_seed(9))
    cloud.xyz = torch.cat([cloud.xyz, torch.from_numpy(world).float()]).contiguous()
    cloud.scales = torch.cat([cloud.scales, torch.tensor([[1e-6] * 3, [0.02, 0.05, 0.03], [0.02] * 3])]).contiguous()
    cloud.rotations = torch.cat([cloud.rotations, q / q.norm(dim=1, keepdim=True)]).contiguous()
    cloud.opacity = torch.cat([cloud.opacity, torch.tensor([[0.9], [0.8], [0.7]])]).contiguous()
    cloud.shs = torch.cat([cloud.shs, cloud.shs[:3]]).contiguous()
    if pose == "inside":
        cam = helpers.posed_camera("inside", W, H)
    return cloud, cam


def _cpu_inputs(pose, inputs, mod):
    """fp32 CPU tensors of one call, by keyword (cov3D_precomp is built WITH the modifier: the rasterizer applies none to it)."""
    cloud, cam = _scene(pose)
    kw = dict(means3D=cloud.xyz, opacities=cloud.opacity)
    if inputs == "sh":
        kw.update(shs=cloud.shs, scales=cloud.scales, rotations=cloud.rotations)
    else:
        kw.update(colors_precomp=helpers.precomp_colors(cloud, cam), cov3D_precomp=helpers.covariance6_cpu(cloud, mod))
    return kw


@functools.lru_cache(maxsize=None)
def _upstream():
    gen = torch.Generator().manual_seed(41)
    gC = torch.randn(3, H, W, generator=gen) * G_SCALE
    gO = torch.randn(1, H, W, generator=gen) * G_SCALE
    gD = torch.randn(1, H, W, generator=gen) * (G_SCALE * GD_SCALE)
    return dict(C=gC, O=gO, D=gD)


def _ground_truth(img64, seed):
    """clip(render64 +- u, 0, 1), u uniform in [0.05, 0.3], resampled where |render64 - gt| (gt as the fp32 image the device
    is given) falls below MARGIN."""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.zeros(3, H, W)
    todo = torch.ones(3, H, W, dtype=torch.bool)
    while bool(todo.any()):
        sign = torch.where(torch.rand(3, H, W, generator=gen) < 0.5, -1.0, 1.0).to(DT)
        u = torch.empty(3, H, W, dtype=DT).uniform_(0.05, 0.3, generator=gen)
        cand = (img64 + sign * u).clamp(0.0, 1.0).float()
        gt = torch.where(todo, cand, gt)
        todo = (img64 - gt.to(DT)).abs() < MARGIN
    return gt


@functools.lru_cache(maxsize=None)
def _ref(pose, antialiasing, inputs, mod):
    """The float64 twin of one (camera, antialiasing, inputs, scale_modifier): images, radii, gt, and per image B in C
    (colour given gC), L (the L1 term, weight 1), O (opacity given gO), D (inverse depth given gD) the gradients of every
    input, + what of them came through s (the antialiasing chain) and through z; + the undecided pairs."""
    from oracle import dense_ref
    cloud, cam = _scene(pose)
    leaves = {k: v.to(DT).requires_grad_(True) for k, v in _cpu_inputs(pose, inputs, mod).items()}
    leaves["means2D"] = torch.zeros(cloud.xyz.shape[0], 3, dtype=DT, requires_grad=True)
    V = cam.world_view_transform.to(DT)
    img, radii, aux = dense_ref.render(W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.tensor(BG, dtype=DT), V,
                                       cam.full_proj_transform.to(DT), cam.camera_center.to(DT), sh_degree=cloud.sh_degree,
                                       scale_modifier=mod, antialiasing=antialiasing, **leaves)
    gt_seed = 1000 + 8 * ["orbit", "inside"].index(pose) + 4 * antialiasing + 2 * (inputs == "sh") + (mod == 1.0)
    gt = _ground_truth(img.detach(), gt_seed)
    up = _upstream()
    l1 = (img - gt.to(DT)).abs().mean()
    losses = dict(C=(img * up["C"].to(DT)).sum(), L=l1, O=(aux["opacity"] * up["O"].to(DT)).sum(),
                  D=(aux["invdepth"] * up["D"].to(DT)).sum())
    names = list(leaves)
    geo = ["means3D"] + list(COV[inputs])
    inner = [aux["depth"]] + ([aux["s"]] if antialiasing else [])
    grads, chain, zchain = {}, {}, None
    for b, loss in losses.items():
        g = torch.autograd.grad(loss, [leaves[k] for k in names] + inner, retain_graph=True, allow_unused=True)
        grads[b] = {k: (torch.zeros_like(leaves[k]) if x is None else x).numpy() for k, x in zip(names, g)}
        if b == "D":
            zchain = (g[len(names)][:, None] * V[:3, 2][None]).numpy()   # dL/dz of the inverse-depth image, into means3D
        else:
            assert g[len(names)] is None   # (only the inverse-depth image looks at z itself)
        if antialiasing:
            gs = g[len(names) + 1]
            c = torch.autograd.grad(aux["s"], [leaves[k] for k in geo], grad_outputs=gs, retain_graph=True, allow_unused=True)
            chain[b] = {k: (torch.zeros_like(leaves[k]) if x is None else x).numpy() for k, x in zip(geo, c)}
    u = helpers.undecided_pairs(aux, W, H)
    vis = (radii > 0).numpy()
    return dict(color=img.detach(), opacity=aux["opacity"].detach(), invdepth=aux["invdepth"].detach(), radii=radii.numpy(),
                gt=gt, l1=float(l1.detach()), grads=grads, chain=chain, zchain=zchain, s=aux["s"].detach().numpy(), visible=vis,
                flag=u["flag"], near=u["near"], met=u["met"], cap=int(0.02 * vis.sum()))


def _settings(cam, dev, antialiasing, mod, bg=BG):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.tensor(bg, device=dev), mod, cam.world_view_transform.to(dev),
        cam.full_proj_transform.to(dev), 3, cam.camera_center.to(dev), False, False, antialiasing)


def _weights(terms):
    return {b: (L1_WEIGHT if b == "L" else 1.0) for b in terms}


class _Call(object):
    """One rasterizer call on fresh leaves, with its loss: `terms` names the images the loss uses (C, O, D as in _ref; L: the
    fused l1 result; S: gsplat_mi355.render.l1_loss on the returned colour image instead).  `gt` is handed over as l1_target
    whenever given (unless `fused` is off), used by the loss or not."""

    def __init__(self, dev, pose, antialiasing, head, inputs, mod, gt=None, opacities=None, fused=True):
        import diff_gaussian_rasterization as dgr
        _, cam = _scene(pose)
        self.dev, self.head = dev, head
        self.names = {k: v.to(dev).requires_grad_(True) for k, v in _cpu_inputs(pose, inputs, mod).items()}
        if opacities is not None:
            self.names["opacities"] = opacities.to(dev).requires_grad_(True)
        self.names["means2D"] = torch.zeros(self.names["means3D"].shape[0], 3, device=dev, requires_grad=True)
        self.rast = dgr.GaussianRasterizer(_settings(cam, dev, antialiasing, mod))
        self.kw = dict(self.names)
        if head == "opacity":
            self.kw["with_opacity"] = True
        if head == "invdepth":
            self.kw["with_invdepth"] = True
        self.gt = None if gt is None else gt.to(dev)
        if gt is not None and fused:
            self.kw["l1_target"] = self.gt
        self.up = {b: t.to(dev) for b, t in _upstream().items()}

    def forward(self):
        res = self.rast(**self.kw)
        out = dict(color=res[0], radii=res[1], l1=res[-1] if "l1_target" in self.kw else None)
        if self.head == "opacity":
            out["opacity"] = res[2]
        if self.head == "invdepth":
            out["invdepth"] = res[2]
        return out

    def loss(self, out, terms):
        from gsplat_mi355.render import l1_loss
        image = dict(C="color", O="opacity", D="invdepth")
        loss = 0.0
        for b in terms:
            if b == "L":
                loss = loss + L1_WEIGHT * out["l1"]
            elif b == "S":
                loss = loss + L1_WEIGHT * l1_loss(out["color"], self.gt)
            else:
                loss = loss + (out[image[b]] * self.up[b]).sum()
        return loss

    def step(self, terms):
        import diff_gaussian_rasterization as dgr
        dgr.release_shared_geometry()
        for t in self.names.values():
            t.grad = None
        out = self.forward()
        self.loss(out, terms).backward()
        return out

    def run(self, terms):
        out = self.step(terms)
        torch.cuda.synchronize()
        grads = {k: t.grad.detach().clone() for k, t in self.names.items()}
        return {k: (v.detach().clone() if v is not None else None) for k, v in out.items()}, grads


def _variants(head, l1):
    """The losses of one head: every image it returns (+ the fused L1); for with_invdepth also without a direct colour
    gradient (with L: dL_dpix = NULL) and the inverse depth alone (with l1_target handed over all the same)."""
    full = {"plain": "C", "opacity": "CO", "invdepth": "CD"}[head] + ("L" if l1 else "")
    return [full] + ((["DL"] if l1 else []) + ["D"] if head == "invdepth" else [])


def _want(ref, terms):
    w = _weights(terms)
    return {k: sum(w[b] * ref["grads"][b][k] for b in terms) for k in ref["grads"]["C"]}


def _assert_terms_visible(tag, ref, terms, antialiasing, inputs, inside=False):
    """On the float64 side: what each option crosses into a tensor exceeds VISIBLE x that tensor's bar (WEAK x: the
    antialiasing chain into means3D, and into every tensor from inside the cloud)."""
    want = _want(ref, terms)
    w = _weights(terms)
    bar = {k: PARITY * np.abs(v).max() for k, v in want.items()}
    parts = []
    if antialiasing:
        for k in ("means3D",) + COV[inputs]:
            floor = WEAK if (inside or k == "means3D") else VISIBLE
            parts.append(("antialiasing chain", k, sum(w[b] * ref["chain"][b][k] for b in terms), floor))
        s = np.where(ref["visible"], ref["s"], 1.0)
        s[CLAMP] = 1.0   # (not counted: its 1/s = 200 would carry the check alone)
        # (s g' against g': what a backward that forgot the factor would be off by; beyond the issue's four terms, WEAK)
        parts.append(("opacity scaling", "opacities", want["opacities"][:, 0] * (1.0 / s - 1.0), WEAK))
    if "D" in terms:
        parts.append(("chain through z", "means3D", ref["zchain"]))
        parts += [("inverse-depth image", k, ref["grads"]["D"][k]) for k in want if k != COLOR[inputs]]
    if "L" in terms:
        parts += [("L1", k, L1_WEIGHT * ref["grads"]["L"][k]) for k in want]
    if "O" in terms:
        parts += [("opacity image", k, ref["grads"]["O"][k]) for k in want if k != COLOR[inputs]]
    if "C" in terms:
        parts += [("colour image", k, ref["grads"]["C"][k]) for k in want]
    for what, k, v, *floor in parts:
        size = np.abs(v).max()
        print("%s: %s into %s: %.3g = %.0f x the bar" % (tag, what, k, size, size / bar[k]))
        assert size > (floor[0] if floor else VISIBLE) * bar[k], (tag, what, k)


def _compare_images(tag, ref, out, head):
    assert np.array_equal(out["radii"].cpu().numpy(), ref["radii"]), tag
    for k in ("color",) + ((head,) if head != "plain" else ()):
        err = float((out[k].cpu().to(DT) - ref[k]).abs().max())
        print("%s: %s image against float64: max |delta| %.3g" % (tag, k, err))
        assert err < 1e-5, (tag, k)
    if out["l1"] is not None:
        gt64 = ref["gt"].to(DT)
        assert float((ref["color"] - gt64).abs().min()) >= MARGIN   # the sign of (colour - gt) is decided alike on both sides
        own = float((out["color"].cpu().to(DT) - gt64).abs().mean())
        got = float(out["l1"])
        print("%s: l1 %.8g, float64 of the device's image %.8g, twin %.8g" % (tag, got, own, ref["l1"]))
        assert got == pytest.approx(own, rel=2e-6) and abs(got - ref["l1"]) <= 1e-5, tag


def _compare_grads(tag, ref, grads, terms):
    want = _want(ref, terms)
    culled = ~ref["visible"]
    for k, g in grads.items():
        _assert_bar("%s: %s" % (tag, k), g.cpu().numpy(), want[k], ref["flag"], ref["cap"])
        assert not g[torch.from_numpy(culled).to(g.device)].any(), (tag, k)   # culled rows: exact zeros


def _print_setaside(tag, ref):
    print("%s: float64 reference: %d undecided pairs of %d tested, on %d Gaussians (cap %d of %d visible)"
          % (tag, ref["near"], ref["met"], int(ref["flag"].sum()), ref["cap"], int(ref["visible"].sum())))
    assert int(ref["flag"].sum()) <= ref["cap"]   # (a condition on the scene: change the seed if the reference alone breaks it)


@pytest.mark.parametrize("mod", [1.0, 0.7])
@pytest.mark.parametrize("inputs", ["sh", "precomp"])
@pytest.mark.parametrize("l1", [False, True], ids=["no-l1", "l1"])
@pytest.mark.parametrize("head", ["plain", "opacity", "invdepth"])
@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain-alpha", "antialiased"])
def test_every_combination_against_the_float64_twin(tile_rect, antialiasing, head, l1, inputs, mod):
    """Images, radii, l1 and every gradient of every loss of the head (_variants) against the twin; culled rows and the
    row behind the near plane exact zeros; each crossed-in term visible."""
    dev = torch.device("cuda:0")
    ref = _ref("orbit", antialiasing, inputs, mod)
    base = "aa %d %s l1 %d %s mod %g tile_rect %d" % (antialiasing, head, l1, inputs, mod, tile_rect)
    _print_setaside(base, ref)
    assert ref["radii"][CLAMP] > 0 and ref["radii"][BORDER] > 0 and ref["radii"][BEHIND] == 0
    call = _Call(dev, "orbit", antialiasing, head, inputs, mod, gt=ref["gt"] if l1 else None)
    for terms in _variants(head, l1):
        tag = base + " loss " + terms
        _assert_terms_visible(tag, ref, terms, antialiasing, inputs)
        out, grads = call.run(terms)
        _compare_images(tag, ref, out, head)
        _compare_grads(tag, ref, grads, terms)
        assert not any(g[BEHIND].any() for g in grads.values())


@pytest.mark.parametrize("inputs", ["sh", "precomp"])
def test_the_fullest_combination_from_inside_the_cloud(tile_rect, inputs):
    """Antialiasing, with_invdepth, L1, scale_modifier 0.7 under helpers.posed_camera("inside"): near-plane culls, huge
    on-screen radii with clamped rects, both Jacobian clamps (asserted)."""
    dev = torch.device("cuda:0")
    cloud, cam = _scene("inside")
    ref = _ref("inside", True, inputs, 0.7)
    vs = helpers.view_stats(cloud, cam)
    tag = "inside %s tile_rect %d" % (inputs, tile_rect)
    print("%s: %s, largest radius %d" % (tag, vs, ref["radii"].max()))
    _print_setaside(tag, ref)
    assert vs["culled"] > 50 and vs["xclamp"] > 0 and vs["yclamp"] > 0 and ref["radii"].max() > max(W, H)
    call = _Call(dev, "inside", True, "invdepth", inputs, 0.7, gt=ref["gt"])
    for terms in ("CDL", "DL"):
        _assert_terms_visible(tag + " loss " + terms, ref, terms, True, inputs, inside=True)
        out, grads = call.run(terms)
        _compare_images(tag + " loss " + terms, ref, out, "invdepth")
        _compare_grads(tag + " loss " + terms, ref, grads, terms)


@pytest.mark.parametrize("inputs", ["sh", "precomp"])
@pytest.mark.parametrize("l1", [False, True], ids=["no-l1", "l1"])
@pytest.mark.parametrize("head", ["plain", "opacity", "invdepth"])
def test_the_clamped_gaussian_gets_no_added_term_under_any_head(head, l1, inputs):
    """Antialiasing on against the default path at the effective opacities o' the device stored (scale_modifier 0.7): the
    images bit for bit; the row of scale 1e-6, whose s is clamped, gets dL/do = 0.005f g'_o and, in every other tensor,
    the default path's row bit for bit -- no antialiasing term -- as test_gpu_antialiasing.py asserts for the plain head."""
    from gsplat_mi355 import debug
    dev = torch.device("cuda:0")
    cloud, cam = _scene("orbit")
    ref = _ref("orbit", True, inputs, 0.7)
    kw = {k: v.to(dev) for k, v in _cpu_inputs("orbit", inputs, 0.7).items()}
    st = debug.forward_state(_settings(cam, dev, True, 0.7), kw.pop("means3D"), kw.pop("opacities"), **kw)
    o_eff = _effective(cloud, st)
    assert float(o_eff[CLAMP, 0]) == float(np.float32(0.9) * np.float32(0.005))
    terms = _variants(head, l1)[0]
    gt = ref["gt"] if l1 else None
    on, g_on = _Call(dev, "orbit", True, head, inputs, 0.7, gt=gt).run(terms)
    off, g_off = _Call(dev, "orbit", False, head, inputs, 0.7, gt=gt, opacities=o_eff).run(terms)
    for k, v in on.items():
        assert v is None or torch.equal(v, off[k]), k
    for k in g_on:
        if k == "opacities":
            assert g_off[k][CLAMP, 0] != 0
            assert np.float32(g_on[k][CLAMP, 0].item()) == np.float32(0.005) * np.float32(g_off[k][CLAMP, 0].item())
        else:
            assert torch.equal(g_on[k][CLAMP], g_off[k][CLAMP]), k
    assert not torch.equal(g_on["means3D"][:N0], g_off["means3D"][:N0])   # (the other rows do get the chain)


@pytest.mark.parametrize("inputs", ["sh", "precomp"])
@pytest.mark.parametrize("head", ["plain", "opacity", "invdepth"])
@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain-alpha", "antialiased"])
def test_l1_target_changes_no_image_and_is_the_separate_l1_loss_bit_for_bit(antialiasing, head, inputs):
    """Handing l1_target over leaves every image and radii bit-identical; the gradients of a loss with the fused l1 equal
    those of the same loss with l1_loss(colour, gt) on the returned image bit for bit (module docstring), also without a
    direct colour gradient (with_invdepth: NULL dL_dpix against a gradient image holding the L1 term alone)."""
    dev = torch.device("cuda:0")
    ref = _ref("orbit", antialiasing, inputs, 0.7)
    full = _variants(head, True)[0]
    without, _ = _Call(dev, "orbit", antialiasing, head, inputs, 0.7).run(full.replace("L", ""))
    for terms in [full] + (["DL"] if head == "invdepth" else []):
        fused, g_fused = _Call(dev, "orbit", antialiasing, head, inputs, 0.7, gt=ref["gt"]).run(terms)
        separate, g_sep = _Call(dev, "orbit", antialiasing, head, inputs, 0.7, gt=ref["gt"], fused=False).run(terms.replace("L", "S"))
        for k, v in without.items():
            assert v is None or (torch.equal(v, fused[k]) and torch.equal(v, separate[k])), k
        for k in g_fused:
            assert float(g_sep[k].abs().max()) > 0 and torch.equal(g_fused[k], g_sep[k]), (terms, k)


def test_invdepth_with_opacity_still_raises():
    dev = torch.device("cuda:0")
    call = _Call(dev, "orbit", True, "invdepth", "sh", 0.7, gt=_ref("orbit", True, "sh", 0.7)["gt"])
    call.kw["with_opacity"] = True
    with pytest.raises(NotImplementedError) as e:
        call.rast(**call.kw)
    assert str(e.value) == ("diff_gaussian_rasterization: with_invdepth and with_opacity cannot be combined in one call "
                            "(render the opacity image with a second call on the same geometry)")


def test_two_runs_give_the_same_bits_and_a_captured_step_replays_the_eager_one():
    """The fullest combination (antialiasing, with_invdepth, L1, scale_modifier 0.7, colour + depth + l1 in the loss): two
    runs bit-identical; one captured step (the recipe of tests/test_gpu_capture.py: side stream, two eager frames first)
    replays bit-identically to the eager step."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    gt = _ref("orbit", True, "sh", 0.7)["gt"]
    out1, g1 = _Call(dev, "orbit", True, "invdepth", "sh", 0.7, gt=gt).run("CDL")
    out2, g2 = _Call(dev, "orbit", True, "invdepth", "sh", 0.7, gt=gt).run("CDL")
    for k in out1:
        assert torch.equal(out1[k], out2[k]), k
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    call = _Call(dev, "orbit", True, "invdepth", "sh", 0.7, gt=gt)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            call.step("CDL")
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    for t in call.names.values():
        t.grad = None
    dgr.release_shared_geometry()
    graph = torch.cuda.CUDAGraph()
    dgr.captured_forwards(clear=True)
    with torch.cuda.graph(graph, stream=side):
        out_g = call.forward()
        call.loss(out_g, "CDL").backward()
    (cnt, capacity), = dgr.captured_forwards(clear=True)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert 0 < int(cnt.item()) <= capacity
    for k in out1:
        assert torch.equal(out_g[k].detach(), out1[k]), k
    for k, t in call.names.items():
        assert torch.equal(t.grad, g1[k]), k


def _render_case(pipe_kw, hits, bar):
    """render() with l1_target, return_opacity and scaling_modifier 0.7 on the orbit scene against the twin; `hits`: how
    many of its rasterizer calls are served from the geometry cache; `bar`: on every gradient tensor."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355.render import Pipe, render
    from gsplat_mi355.scenes import GaussianCloud
    dev = torch.device("cuda:0")
    cloud, cam = _scene("orbit")
    ref = _ref("orbit", True, "sh", 0.7)
    up = {b: t.to(dev) for b, t in _upstream().items()}
    pc = GaussianCloud(cloud.xyz.to(dev), cloud.scales.to(dev), cloud.rotations.to(dev), cloud.opacity.to(dev), cloud.shs.to(dev),
                       cloud.sh_degree)
    names = dict(means3D=pc.xyz, opacities=pc.opacity, scales=pc.scales, rotations=pc.rotations, shs=pc.shs)
    for t in names.values():
        t.requires_grad_(True)
    dgr.release_shared_geometry()
    hits0 = dgr._geom_cache.hits
    pkg = render(cam.to(dev), pc, Pipe(**pipe_kw), torch.tensor(BG, device=dev), scaling_modifier=0.7, return_opacity=True,
                 l1_target=ref["gt"].to(dev))
    cam.to("cpu")
    got_hits = dgr._geom_cache.hits - hits0
    print("render(%s): %d geometry-cache hits" % (pipe_kw, got_hits))
    assert got_hits == hits
    terms = "COL" + ("D" if pipe_kw.get("invdepth") else "")
    loss = (pkg.render * up["C"]).sum() + (pkg.opacity_render * up["O"]).sum() + L1_WEIGHT * pkg.l1
    if "D" in terms:
        loss = loss + (pkg.invdepth_render * up["D"]).sum()
    else:
        assert pkg.invdepth_render is None
    loss.backward()
    torch.cuda.synchronize()
    names["means2D"] = pkg.viewspace_points
    tag = "render(%s)" % ", ".join(sorted(pipe_kw))
    _print_setaside(tag, ref)
    _assert_terms_visible(tag, ref, terms, True, "sh")
    out = dict(color=pkg.render.detach(), radii=pkg.radii, l1=pkg.l1.detach(), opacity=pkg.opacity_render.detach())
    _compare_images(tag, ref, out, "opacity")
    if "D" in terms:
        assert float((pkg.invdepth_render.detach().cpu().to(DT) - ref["invdepth"]).abs().max()) < 1e-5
    want = _want(ref, terms)
    for k, t in names.items():
        g = t.grad.cpu().numpy().astype(np.float64).reshape(want[k].shape[0], -1)
        w = want[k].reshape(want[k].shape[0], -1)
        err = np.abs(g - w).max(1) / np.abs(w).max()
        over = (err > bar) & ~ref["flag"]
        print("%s: %s: max|g| %.4g, largest error %.3g of it" % (tag, k, np.abs(w).max(), err.max()))
        assert not over.any() and int((err > bar).sum()) <= ref["cap"], (tag, k)


def test_render_with_antialiasing_invdepth_l1_and_the_opacity_pass_behind_it():
    """Pipe(antialiasing=True, invdepth=True), return_opacity=True, l1_target, scaling_modifier 0.7: the one-pass call, then
    the opacity pass served from its geometry (1 cache hit: module docstring) with a backward of its own -- two separately
    rounded backward results are summed, hence twice the parity bar (as test_gpu_invdepth.py's render() test)."""
    _render_case(dict(antialiasing=True, invdepth=True), hits=1, bar=2 * PARITY)


def test_render_with_antialiasing_fused_opacity_and_l1():
    """Pipe(antialiasing=True, fuse_opacity=True), l1_target: one rasterizer call, no cache hit, the parity bar."""
    _render_case(dict(antialiasing=True, fuse_opacity=True), hits=0, bar=PARITY)


@pytest.mark.parametrize("l1", [False, True], ids=["no-l1", "l1"])
@pytest.mark.parametrize("color_mode,cov_mode", [("sh", "scale_rot"), ("precomp", "cov3d")])
def test_long_lists_one_pass_against_two_calls_under_antialiasing(color_mode, cov_mode, l1):
    """Tile lists of more than one 256-entry staging batch (test_gpu_antialiasing._scene(1.0): 2051 Gaussians, 96 x 80; no
    float64 autograd at this size): the one-pass call against two calls, both with the flag, device against device at the
    parity bar with no exclusions -- also with l1_target on the colour call."""
    import test_gpu_antialiasing as aa
    import test_gpu_invdepth as inv
    dev = torch.device("cuda:0")
    cloud, cam = aa._scene(1.0)
    _, _, st = inv._depths(cloud, cam, dev)
    lens = st["image"]["ranges"][:, 1].astype(np.int64) - st["image"]["ranges"][:, 0]
    assert lens.max() > BATCH
    gC, gD = inv._g(37)
    gt = torch.rand(3, aa.H, aa.W, generator=torch.Generator().manual_seed(38)) if l1 else None
    if l1:   # (of the size of the L1 term, so that it is a visible share; asserted below through its effect)
        gC, gD = gC * G_SCALE, gD * G_SCALE
    (c1, i1, _), one = _one_pass(cloud, cam, dev, gC, gD, color_mode, cov_mode, antialiasing=True, l1_target=gt)
    (c2, i2), two = _formulation_c(cloud, cam, dev, gC, gD, color_mode, cov_mode, antialiasing=True, l1_target=gt)
    assert torch.equal(c1, c2) and torch.equal(i1[0], i2[0])
    cov_names = ("scales", "rotations") if cov_mode == "scale_rot" else ("cov3D_precomp",)
    for k in ("means3D", "means2D", "opacities", "colors2", "shs" if color_mode == "sh" else "colors_precomp") + cov_names:
        _assert_bar("long lists %s %s l1 %d: %s" % (color_mode, cov_mode, l1, k), one[k].cpu().numpy(), two[k].cpu().numpy())
    if l1:
        _, bare = _one_pass(cloud, cam, dev, gC, gD, color_mode, cov_mode, antialiasing=True)
        m = float(one["means3D"].abs().max())
        assert float((one["means3D"] - bare["means3D"]).abs().max()) > VISIBLE * PARITY * m
