"""The short kernels of a frame whose loads are issued together (tile_write's prologue, segment_starts, the tile orderings,
segment_reduce, the depth ranking's counting and scattering passes), at the sizes where their clamped, unconditional loads
and the values chosen afterwards can go wrong: segment counts on both sides of every batch of segment-count loads up to
TB_MAX_SEG, a tile row wider than a wave, a frame beyond its capacity, tile counts around the 1024 tiles a round of the
ordering takes, culled Gaussians at both ends of a workgroup.  Integers against the CPU oracle, exactly; gradients with the
bar of test_gpu_parity.test_backward_matches_oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch

import helpers
from test_gpu_parity import _attribute, _bulk_close, _inputs, _settings

pytestmark = pytest.mark.gpu


def _frame(cloud, cam, cap=None, backward=False, bg=(0.0, 0.0, 0.0)):
    """The two-phase forward through the C ABI (as gsplat_mi355.debug.forward_state runs it) with the binning state
    DECLARED for `cap` pairs (None: the frame's count) and allocated for the larger of the two; with `backward`, gs_backward
    on a fixed random image gradient as well, for the tile order it leaves behind its sums in the scratch."""
    from diff_gaussian_rasterization import _make_args
    from gsplat_mi355 import _lib
    dev = torch.device("cuda:0")
    L = _lib.load()
    P, W, H = cloud.xyz.shape[0], cam.image_width, cam.image_height
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    keep = []
    with torch.cuda.device(dev):
        # (the argument block holds addresses only: the tensors live in `ins` until the last call has run)
        ins = [t.to(dev).contiguous() for t in (cloud.xyz, cloud.shs, cloud.opacity, cloud.scales, cloud.rotations)]
        settings = _settings(cam, cloud, bg, dev)
        a = _make_args(settings, ins[0], ins[1], None, ins[2], ins[3], ins[4], None, keep)
        a.frame_stats = None
        sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        gb, ib = _lib.nbytes(L.gs_geom_bytes, P), _lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a))
        geom = torch.zeros(gb, dtype=torch.uint8, device=dev)
        img = torch.zeros(ib, dtype=torch.uint8, device=dev)
        radii = torch.zeros(P, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64).pin_memory()
        _lib.check(L.gs_forward_preprocess(ctypes.byref(a), geom.data_ptr(), gb, img.data_ptr(), ib, radii.data_ptr(),
                                           count.data_ptr(), sptr))
        torch.cuda.synchronize()
        D = int(count.item())
        decl = D if cap is None else cap
        bb = _lib.nbytes(L.gs_binning_bytes, decl, W, H)
        binning = torch.full((max(bb, _lib.nbytes(L.gs_binning_bytes, D, W, H)),), 0xFF, dtype=torch.uint8, device=dev)
        color = torch.full((3, H, W), 7.0, device=dev)
        _lib.check(L.gs_forward_render(ctypes.byref(a), geom.data_ptr(), gb, binning.data_ptr(), bb, img.data_ptr(), ib, decl,
                                       color.data_ptr(), sptr))
        torch.cuda.synchronize()

        def image_field(dtype, nbytes, fid):
            return _lib.field_view("gs_image_field", img, W, H, fid, nbytes=nbytes).cpu().numpy().view(dtype).copy()
        out = dict(D=D, color=color.cpu().numpy(), radii=radii.cpu().numpy(),
                   ranges=image_field(np.uint32, 8 * ntiles, _lib.GS_IMG_RANGES).reshape(-1, 2),
                   order=image_field(np.uint32, 4 * ntiles, _lib.GS_IMG_ORDER),
                   qcount=image_field(np.uint32, 16 * ntiles, _lib.GS_IMG_QCOUNT).reshape(-1, 4))
        if decl >= D > 0:
            out["point_list"] = _lib.field_view("gs_binning_field", binning, D, W, H, _lib.GS_BIN_POINT_LIST,
                                                nbytes=4 * D).cpu().numpy().view(np.uint32).copy()
        if backward:
            sb = _lib.nbytes(L.gs_backward_scratch_bytes, D, P, W, H)
            scratch = torch.full((sb,), 0xFF, dtype=torch.uint8, device=dev)
            f = dict(dtype=torch.float32, device=dev)
            d = dict(means3D=torch.empty(P, 3, **f), means2D=torch.empty(P, 3, **f), sh=torch.empty(P, cloud.shs.shape[1], 3, **f),
                     colors=torch.empty(P, 3, **f), opacity=torch.empty(P, 1, **f), scales=torch.empty(P, 3, **f),
                     rot=torch.empty(P, 4, **f), cov=torch.empty(P, 6, **f))
            gr = _lib.GsGrads(*(d[k].data_ptr() for k in ("means3D", "means2D", "sh", "colors", "opacity", "scales", "rot", "cov")))
            g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
            _lib.check(L.gs_backward(ctypes.byref(a), radii.data_ptr(), geom.data_ptr(), gb, binning.data_ptr(), bb, img.data_ptr(),
                                     ib, D, color.data_ptr(), g.data_ptr(), scratch.data_ptr(), sb, ctypes.byref(gr), sptr))
            torch.cuda.synchronize()
            # (the scratch ends with the backward's own tile order: common.h, scratch_total_bytes)
            tail = (ntiles * 4 + 255) // 256 * 256
            out["bwd_order"] = scratch[sb - tail:sb - tail + 4 * ntiles].cpu().numpy().view(np.uint32).copy()
    return out


def _lists_match(got, ob):
    """Tile lists and ranges against the oracle's binning, exactly (an empty tile's range may sit anywhere)."""
    assert got["D"] == ob["D"]
    assert np.array_equal(got["point_list"], ob["point_list"])
    nz = ob["ranges"][:, 1] > ob["ranges"][:, 0]
    assert np.array_equal(got["ranges"][nz], ob["ranges"][nz])
    assert (got["ranges"][~nz, 1] == got["ranges"][~nz, 0]).all()


@pytest.mark.parametrize("P,segments", [(1025, 2), (8193, 9), (9217, 10), (17409, 18), (66000, 64)])
def test_tile_lists_with_segment_counts_across_the_load_batches(oracle, P, segments):
    """256 x 256: 16 x 16 tiles in 4 blocks of 64 x 4, so P Gaussians are cut into min(ceil(P / 1024), 64) rank segments -- the
    last workgroup of a block adds up 1, 8, 9, 17 and 63 earlier segments' counts: below, at and beyond every batch the
    prologue loads them in (4, 8 and 16 per wave over four waves), up to TB_MAX_SEG."""
    assert min((P + 1023) // 1024, 64) == segments
    W = H = 256
    cloud, cam = helpers.cloud_and_camera(P, W, H, sh_degree=0, seed=41)
    cloud.xyz[:40, 2] = -3.5  # behind the near plane
    ob = oracle.forward(helpers.oracle_scene(cloud, cam))["binning"]
    assert ob["D"] > 4 * P / 3
    _lists_match(_frame(cloud, cam), ob)


def test_tile_lists_on_a_grid_wider_than_a_wave(oracle):
    """1056 x 64: 66 x 4 tiles, two blocks side by side, the second 2 tiles wide; a tile row's sum spans two trips of a wave."""
    cloud, cam = helpers.cloud_and_camera(3000, 1056, 64, sh_degree=0, seed=42)
    ob = oracle.forward(helpers.oracle_scene(cloud, cam))["binning"]
    nz = ob["ranges"][:, 1] > ob["ranges"][:, 0]
    assert nz[64:66].any() or nz[130:132].any()  # the narrow block is not empty
    _lists_match(_frame(cloud, cam), ob)


def test_a_frame_beyond_its_capacity_still_gets_empty_ranges():
    cloud, cam = helpers.cloud_and_camera(9217, 256, 256, sh_degree=0, seed=41)
    got = _frame(cloud, cam, cap=1024)
    assert got["D"] > 8 * 1024
    assert not got["ranges"].any()
    assert not got["color"].any()  # the empty frame (zero background)


def _work_bins(work):
    """tile_order_plain's bins, in its own fp32 steps: 1023 - min(1023, trunc(work * (1023 / max work)))."""
    mx = np.float32(work.max())
    scale = np.float32(1023.0) / mx if mx else np.float32(0.0)
    return 1023 - np.minimum(1023, (work.astype(np.float32) * scale).astype(np.uint32).astype(np.int64))


@pytest.mark.parametrize("W,H,ntiles", [(16, 16, 1), (528, 496, 1023), (512, 512, 1024), (656, 400, 1025), (272, 3856, 4097)])
def test_tile_orders_are_permutations_by_falling_work(W, H, ntiles):
    """Both orderings that keep the tiles' work in registers -- the forward's (work = the tile's pair count, workgroup 0 of the
    list-writing launch) and the backward's launch (work = the quadrants' compacted entries) -- with 1 tile, one short of,
    exactly and one beyond a round of 1024, and one beyond four rounds: every tile once, bins of work never rising along
    the order; ties fall either way."""
    assert ((W + 15) // 16) * ((H + 15) // 16) == ntiles
    cloud, cam = helpers.cloud_and_camera(3000, W, H, sh_degree=0, seed=43, scale_mul=2.0)
    got = _frame(cloud, cam, backward=True)
    assert got["D"] > 0
    lens = (got["ranges"][:, 1] - got["ranges"][:, 0]).astype(np.int64)
    for name, order, work in (("forward", got["order"] & 0x7FFFFFFF, lens),
                              ("backward", got["bwd_order"], got["qcount"].astype(np.int64).sum(1))):
        assert np.array_equal(np.sort(order), np.arange(ntiles)), name
        bins = _work_bins(work)[order]
        assert (np.diff(bins) >= 0).all(), name
        assert work.max() > 0, name


@pytest.mark.parametrize("culled_part", ["third", "all", "none"])
def test_gradients_with_culled_gaussians_at_the_workgroup_ends(oracle, culled_part):
    """The per-Gaussian sums request radius, tile count and record together, whatever a culled Gaussian's record holds: a
    third, all and none of the Gaussians culled, among them both ends of the 16-Gaussian workgroups of the row sums and of
    the 256-Gaussian workgroups of the per-Gaussian backward, and the last Gaussian of a ragged tail.  Culled Gaussians get
    exact zeros; the others the bar of test_backward_matches_oracle."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    n, W, H = 600, 160, 120
    cloud, cam = helpers.cloud_and_camera(n, W, H, sh_degree=1, seed=44, scale_mul=1.3)
    cloud.xyz *= 0.4  # everything in view
    want_culled = np.zeros(n, bool)
    if culled_part == "third":
        want_culled[::3] = True
        want_culled[[0, 15, 16, 31, 255, 256, 271, 272, n - 1]] = True
    elif culled_part == "all":
        want_culled[:] = True
    cloud.xyz[torch.from_numpy(want_culled), 2] = -3.5  # behind the near plane
    bg = (0.25, 0.5, 0.75)
    kw = {k: v.clone().requires_grad_(True) for k, v in _inputs(cloud, cam, "sh", "scale_rot", dev).items()}
    means3D = cloud.xyz.to(dev).requires_grad_(True)
    means2D = torch.zeros(n, 3, device=dev, requires_grad=True)
    opac = cloud.opacity.to(dev).requires_grad_(True)
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5))
    color, radii = GaussianRasterizer(_settings(cam, cloud, bg, dev))(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    (color * gimg.to(dev)).sum().backward()
    got = dict(means3D=means3D.grad, means2D=means2D.grad, opacities=opac.grad, sh=kw["shs"].grad, scales=kw["scales"].grad,
               rotations=kw["rotations"].grad)
    culled = radii.cpu().numpy() == 0
    assert np.array_equal(culled, want_culled)
    for name, gt in got.items():
        assert gt is not None and (gt.cpu().numpy()[culled] == 0).all(), name
    if culled_part == "all":
        return
    from gsplat_mi355 import debug
    sc = helpers.oracle_scene(cloud, cam, bg=bg)
    fw = oracle.forward(sc)
    assert np.array_equal(fw["radii"] == 0, want_culled)
    st = debug.forward_state(_settings(cam, cloud, bg, dev), cloud.xyz.to(dev), cloud.opacity.to(dev),
                             **_inputs(cloud, cam, "sh", "scale_rot", dev))
    fwc, ov = _attribute(oracle, sc, fw, st["color"], st["image"]["final_T"], st["image"]["n_contrib"], "culled " + culled_part)
    want = oracle.backward(sc, fwc, gimg.numpy(), ov)
    for name, gt in got.items():
        w = want[name].reshape(gt.shape)
        _bulk_close(gt.cpu().numpy(), w, tol=1e-5, frac=0.0, name=name)
        assert np.abs(w).max() > 0
