"""Parity-test introspection: runs the two forward phases through the C ABI and copies every
intermediate of the opaque state buffers back as numpy arrays (gs_*_field of include/gsplat_mi355.h)."""
import ctypes

import numpy as np
import torch

from gsplat_mi355 import _lib
from diff_gaussian_rasterization import GaussianRasterizationSettings, _make_args, _f32c


# a callable given dL_dcolors (P, 3) of the inverse-depth render -- the output of csrc/second_colors.hip -- by every backward
# of diff_gaussian_rasterization that computes it (None: off)
second_colors_hook = None


def forward_state(settings, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                  cov3D_precomp=None):
    """Runs preprocess + render through the C ABI; returns dict(color, radii, geom=..., binning=..., image=...)."""
    L = _lib.load()
    dev = means3D.device
    means3D = _f32c(means3D, "means3D")
    shs, colors_precomp = _f32c(shs, "shs"), _f32c(colors_precomp, "colors_precomp")
    opacities = _f32c(opacities, "opacities")
    scales, rotations, cov3D_precomp = _f32c(scales, "scales"), _f32c(rotations, "rotations"), _f32c(cov3D_precomp, "cov")
    P = int(means3D.shape[0])
    W, H = int(settings.image_width), int(settings.image_height)
    keep = []
    with torch.cuda.device(dev):
        a = _make_args(settings, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, keep)
        stream = torch.cuda.current_stream(dev)
        sptr = ctypes.c_void_p(stream.cuda_stream)
        gb = _lib.nbytes(L.gs_geom_bytes, P)
        ib = _lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a))
        geom = torch.zeros(gb, dtype=torch.uint8, device=dev)
        img = torch.zeros(ib, dtype=torch.uint8, device=dev)
        radii = torch.zeros(P, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64).pin_memory()
        _lib.check(L.gs_forward_preprocess(ctypes.byref(a), geom.data_ptr(), gb, img.data_ptr(), ib, radii.data_ptr(),
                                           count.data_ptr(), sptr))
        stream.synchronize()
        D = int(count.item())
        bb = _lib.nbytes(L.gs_binning_bytes, D, W, H)
        binning = torch.zeros(bb, dtype=torch.uint8, device=dev)
        color = torch.zeros(3, H, W, device=dev)
        _lib.check(L.gs_forward_render(ctypes.byref(a), geom.data_ptr(), gb, binning.data_ptr(), bb, img.data_ptr(), ib,
                                       D, color.data_ptr(), sptr))
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.gs_pair_stats(ctypes.byref(a), geom.data_ptr(), gb, binning.data_ptr(), bb, img.data_ptr(), ib, D,
                                   counts.data_ptr(), sptr))
        stream.synchronize()
        pairs_valid, pairs_walked = (int(v) for v in counts.cpu())

        def field(dtype, nbytes, *where):
            """numpy copy of a field of a state buffer; `where`: the entry point, the buffer, its sizes, the field's id."""
            return _lib.field_view(*where, nbytes=nbytes).cpu().numpy().view(dtype).copy()
        gx, gy = (W + 15) // 16, (H + 15) // 16
        g = dict(
            depths=field(np.float32, 4 * P, "gs_geom_field", geom, P, _lib.GS_GEOM_DEPTHS),
            tiles_touched=field(np.uint32, 4 * P, "gs_geom_field", geom, P, _lib.GS_GEOM_TILES),
            rec=field(np.float32, 48 * P, "gs_geom_field", geom, P, _lib.GS_GEOM_REC).reshape(P, 12),
            clamped=field(np.uint32, 4 * P, "gs_geom_field", geom, P, _lib.GS_GEOM_CLAMPED),
            sorted_idx=field(np.uint32, 4 * P, "gs_geom_field", geom, P, _lib.GS_GEOM_SORTED_IDX),
        ) if P > 0 else {}
        b = dict(
            point_list=field(np.uint32, 4 * D, "gs_binning_field", binning, D, W, H, _lib.GS_BIN_POINT_LIST),
            # the quadrants' compacted lists: quadrant q of tile t at [4 ranges[t, 0] + q n_t, ... + qcount[t, q])
            qlist=field(np.uint32, 16 * D, "gs_binning_field", binning, D, W, H, _lib.GS_BIN_QLIST),
        ) if D > 0 else dict(point_list=np.zeros(0, np.uint32), qlist=np.zeros(0, np.uint32))
        im = dict(
            ranges=field(np.uint32, 8 * gx * gy, "gs_image_field", img, W, H, _lib.GS_IMG_RANGES).reshape(-1, 2),
            n_contrib=field(np.uint32, 4 * W * H, "gs_image_field", img, W, H, _lib.GS_IMG_N_CONTRIB).reshape(H, W),
            final_T=field(np.float32, 4 * W * H, "gs_image_field", img, W, H, _lib.GS_IMG_FINAL_T).reshape(H, W),
            qcount=field(np.uint32, 16 * gx * gy, "gs_image_field", img, W, H, _lib.GS_IMG_QCOUNT).reshape(-1, 4),
            # launch order of the tiles (heaviest first); bit 31: rendered by four waves per quadrant (small images)
            order=field(np.uint32, 4 * gx * gy, "gs_image_field", img, W, H, _lib.GS_IMG_ORDER),
        )
    # the tile of every list entry: the lists are stored tile after tile, so the ranges say it (upstream keeps the tile
    # id in the high half of its sort keys)
    r = im["ranges"].astype(np.int64)
    lens = np.maximum(r[:, 1] - r[:, 0], 0)
    nz = lens > 0
    starts = r[nz, 0]
    ok = int(lens.sum()) == D and (starts.size == 0 or (starts[0] == 0 and np.array_equal(starts[1:], r[nz, 1][:-1])))
    # (consistent only if the non-empty ranges tile [0, D) in tile order; otherwise a pattern no comparison accepts)
    b["tile_ids"] = np.repeat(np.arange(r.shape[0], dtype=np.uint32), lens) if ok else np.full(D, 0xFFFFFFFF, np.uint32)
    return dict(color=color.cpu().numpy(), radii=radii.cpu().numpy(), D=D, geom=g, binning=b, image=im,
                pairs_valid=pairs_valid, pairs_walked=pairs_walked)


def frame_stats(cam, cloud, pipe, bg):
    """(num_rendered D, mean n_contrib per pixel, quadrant hits, pairs composited) of one frame: reported beside every
    benchmark number.  Quadrant hits = (8x8 quadrant, Gaussian) entries up to each quadrant's last contributor: what the
    backward's wave per quadrant iterates over, 64 pixels per entry; pairs composited = the (pixel, Gaussian) pairs with
    alpha >= 1/255 before the pixel is done (gs_pair_stats): the useful part of 64 x quadrant hits."""
    import math
    settings = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=cloud.sh_degree, campos=cam.camera_center, prefiltered=False,
        debug=False, antialiasing=bool(getattr(pipe, "antialiasing", False)))  # (fewer pairs with it: smaller snug boxes)
    with torch.no_grad():
        st = forward_state(settings, cloud.xyz.detach(), cloud.opacity.detach(), shs=cloud.shs.detach(),
                           scales=cloud.scales.detach(), rotations=cloud.rotations.detach())
    return (int(st["D"]), float(st["image"]["n_contrib"].mean()), int(st["image"]["qcount"].astype("int64").sum()),
            int(st["pairs_valid"]))
