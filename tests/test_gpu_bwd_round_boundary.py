"""render_bwd's round boundary and epilogue (csrc/render_bwd.hip): every 16 steps a wave folds the four rings' partial sums of
a finished chunk of 16 list entries with lane swaps and all four rings store their dwords of the entries' gradient rows;
the last two chunks are folded and stored behind the loop.  What can go wrong there depends on the length of a quadrant's
list around a multiple of 16, not on the size of the image:

* on the device (-m gpu): a 40 x 24 image (one full tile row, one partial row, a partial column: lanes outside W and H) under
  a stack of m translucent Gaussians that all reach every quadrant, m around one, two and three rounds -- a lone round, both
  parities of the last round, both branches of the epilogue -- in all four kernel modes, and one frame of lists long enough
  for the backward in chunks (full chunks of 128 entries, last chunks that end inside a round).  Every gradient against the CPU oracle (conditioned on
  the attributed threshold decisions, as everywhere in the suite) at 1e-5 of the tensor maximum, every element; two
  backwards give equal bits;
* in the generated code (no GPU): the fold no longer goes through the LDS unit, and the kernels keep their registers.
"""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import abi_header
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dgs-avatar-release_amd")
W, H = 40, 24
BG = (0.3, 0.6, 0.1)
TOL = 1e-5  # of the tensor maximum, every element


# ---------------------------------------------------------------------------------------------------------------
# generated code
# ---------------------------------------------------------------------------------------------------------------
def _backward_code_object():
    """(disassembly per kernel symbol, metadata per kernel name) of the gfx950 code object inside build/render_bwd.o."""
    obj = os.path.join(PKG, "build", "render_bwd.o")
    if not os.path.exists(obj):
        import __graft_entry__
        __graft_entry__.build()
        if not os.path.exists(obj):  # (the library was up to date, the objects are gone)
            abi_header.build_module().build(force=True)
    spec = importlib.util.spec_from_file_location("check_inflight", os.path.join(PKG, "check_inflight.py"))
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    objdump = ci._objdump("hipcc")
    readelf = os.path.join(os.path.dirname(objdump), "llvm-readelf")
    tmp = tempfile.mkdtemp(prefix="gs_bwd_code_")
    try:
        local = os.path.join(tmp, "render_bwd.o")
        shutil.copy(obj, local)
        subprocess.run([objdump, "--offloading", local], cwd=tmp, capture_output=True, check=True)
        dev = [f for f in os.listdir(tmp) if "hipv4-amdgcn" in f]
        assert dev, "no gfx950 code object in %s" % obj
        asm = subprocess.run([objdump, "-d", os.path.join(tmp, dev[0])], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([readelf, "--notes", os.path.join(tmp, dev[0])], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    code, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            code[cur] = []
        elif cur and line.startswith("\t"):
            code[cur].append(line.split("//")[0].strip())
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return code, meta


def test_the_fold_stays_off_the_lds_unit_and_the_kernels_keep_their_registers():
    """At most two ds_bpermute_b32 per kernel (74 before the lane-swap fold), lane swaps in their place, no scratch, and the
    one-image kernels (modes 0, 1, 3) within the 78 VGPRs they had: six waves per SIMD.  Mode 2 carries three more entry
    values and four more pixel constants -- 88 VGPRs before the lane-swap fold, 86 with it (five waves either way): it must not
    grow."""
    code, meta = _backward_code_object()
    kernels = [k for k in code if "render_bwd_kernel" in k]
    assert len(kernels) == 4, kernels
    for k in kernels:
        assert len(code[k]) > 500, k
        perm = sum(i.startswith("ds_bpermute_b32") for i in code[k])
        swaps = sum(i.startswith(("v_permlane16_swap_b32", "v_permlane32_swap_b32")) for i in code[k])
        print(k[:28], "ds_bpermute_b32", perm, "lane swaps", swaps, meta[k])
        assert perm <= 2, (k, perm)
        assert swaps >= 4 * 8, (k, swaps)  # a fold in each of the two round bodies, two behind the loop; eight swaps each
        assert meta[k]["private_segment_fixed_size"] == 0 and meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] <= (86 if "ILi2E" in k else 78), (k, meta[k])


# ---------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------
def _stack(m, seed, sigma_px=(20.0, 28.0), opacity=(0.04, 0.08), small=0):
    """m Gaussians in front of the benchmark camera, centres in the middle of the 40 x 24 image (x 12-28, y 6-18), sigma of
    20-28 pixels and opacity 0.04-0.08: each reaches every pixel with alpha >= 0.04 exp(-32^2 / (2 20^2)) = 0.011, well above
    1 / 255 (32 px: from a centre at (12, 6) to the far corner), and 49 of them leave T >= 0.92^49 = 0.017, far above 1e-4.
    `small`: that many of them get a sigma of 2-4 pixels instead (they reach some quadrants only)."""
    cloud, cam = helpers.cloud_and_camera(m, W, H, sh_degree=1, seed=seed)
    g = torch.Generator().manual_seed(seed)
    f = 500.0 * W / 512.0
    zc = torch.empty(m).uniform_(2.5, 3.5, generator=g)  # distinct depths: one order
    u = torch.empty(m).uniform_(12.0, 28.0, generator=g)
    v = torch.empty(m).uniform_(6.0, 18.0, generator=g)
    cloud.xyz = torch.stack([(u - (W - 1) / 2) * zc / f, (v - (H - 1) / 2) * zc / f, zc - 3.0], 1).contiguous()
    sig = torch.empty(m, 3).uniform_(*sigma_px, generator=g)
    if small:
        sig[torch.randperm(m, generator=g)[:small]] = torch.empty(small, 3).uniform_(2.0, 4.0, generator=g)
    cloud.scales = (sig * zc[:, None] / f).contiguous()
    cloud.opacity = torch.empty(m, 1).uniform_(*opacity, generator=g)
    return cloud, cam


def _run(oracle, monkeypatch, m, mode, cloud_cam=None, check_lists=True):
    """One frame through the drop-in rasterizer in kernel mode `mode` (0: one image; 1: with_opacity=True; 2: a second image
    with arbitrary constant colours; 3: a second image of colours one), gradients against the oracle's pass(es)."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355 import _lib, debug
    from helpers import _CallCounter
    from test_gpu_parity import _attribute, _bulk_close, _settings
    dev = torch.device("cuda:0")
    cloud, cam = cloud_cam or _stack(m, seed=100 + m)
    n = cloud.xyz.shape[0]
    gen = torch.Generator().manual_seed(7 + m)
    g0, g1 = torch.randn(3, H, W, generator=gen), torch.randn(3, H, W, generator=gen)
    cols2 = torch.rand(n, 3, generator=gen) if mode == 2 else torch.ones(n, 3)
    counter = _CallCounter(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counter)
    dgr.release_shared_geometry()
    cols_cpu, cov_cpu = helpers.precomp_colors(cloud, cam), helpers.covariance6_cpu(cloud)

    def device_pass(backwards):
        xyz = cloud.xyz.to(dev).requires_grad_(True)
        m2d = torch.zeros(n, 3, device=dev, requires_grad=True)
        op = cloud.opacity.to(dev).requires_grad_(True)
        cov = cov_cpu.to(dev).requires_grad_(True)
        cols = cols_cpu.to(dev).requires_grad_(True)
        leaves = dict(means3D=xyz, means2D=m2d, opacities=op, cov3D_precomp=cov, colors_precomp=cols)
        rast = dgr.GaussianRasterizer(_settings(cam, cloud, BG, dev))
        if mode == 1:
            img1, _, opa = rast(means3D=xyz, means2D=m2d, opacities=op, colors_precomp=cols, cov3D_precomp=cov, with_opacity=True)
            loss = (img1 * g0.to(dev)).sum() + (opa * g1[:1].to(dev)).sum()
        else:
            img1, _ = rast(means3D=xyz, means2D=m2d, opacities=op, colors_precomp=cols, cov3D_precomp=cov)
            loss = (img1 * g0.to(dev)).sum()
            if mode >= 2:
                img2, _ = rast(means3D=xyz, means2D=m2d, opacities=op, colors_precomp=cols2.to(dev), cov3D_precomp=cov)
                loss = loss + (img2 * g1.to(dev)).sum()
        grads = []
        for k in range(backwards):
            for t in leaves.values():
                t.grad = None
            loss.backward(retain_graph=k + 1 < backwards)
            grads.append({k2: t.grad.detach().cpu().numpy().copy() for k2, t in leaves.items()})
        torch.cuda.synchronize()
        return img1.detach().cpu().numpy(), grads

    if mode <= 1:  # two backwards of the same forward
        img, (got, again) = device_pass(2)
    else:  # (the two-image step hands its second render's state to one backward: the frame is run twice instead)
        img, (got,) = device_pass(1)
        dgr.release_shared_geometry()
        img_b, (again,) = device_pass(1)
        assert np.array_equal(img, img_b)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), "two backwards differ in " + k
    want_call = {0: "gs_backward", 1: "gs_backward_with_opacity", 2: "gs_backward_with_second", 3: "gs_backward_with_second"}[mode]
    assert counter.calls[want_call] >= 1, dict(counter.calls)

    sc = helpers.oracle_scene(cloud, cam, bg=BG, color_mode="precomp", cov_mode="cov")
    fw = oracle.forward(sc)
    st = debug.forward_state(_settings(cam, cloud, BG, dev), cloud.xyz.to(dev), cloud.opacity.to(dev),
                             colors_precomp=cols_cpu.to(dev), cov3D_precomp=cov_cpu.to(dev))
    assert np.array_equal(img, st["color"])
    qc = st["image"]["qcount"].astype(np.int64).reshape(-1)
    print("m", m, "mode", mode, "entries per quadrant:", sorted(qc.tolist()))
    if check_lists:
        # every Gaussian is in the list of every quadrant that has pixels (15 of the 24 of the 3 x 2 tiles): m entries each
        inside = np.array([(16 * (t % 3) + 8 * (q & 1) < W) and (16 * (t // 3) + 8 * (q >> 1) < H) for t in range(6) for q in range(4)])
        assert qc.shape == (24,) and (qc[inside] == m).all() and (qc[~inside] == 0).all(), qc
        assert float(st["image"]["final_T"].min()) > 1e-4  # no pixel stops early
    tag = "round boundary m=%d mode=%d" % (n, mode)
    fwc, ov = _attribute(oracle, sc, fw, st["color"], st["image"]["final_T"], st["image"]["n_contrib"], tag)
    want = {k: np.asarray(v, np.float64) for k, v in oracle.backward(sc, fwc, g0.numpy(), ov).items()}
    if mode >= 1:
        sc2 = helpers.oracle_scene(cloud, cam, bg=BG, color_mode="precomp", colors=cols2, cov_mode="cov")
        fw2 = oracle.forward(sc2)
        im2 = oracle.render_forward(sc2, fw2["geom"], fw2["binning"], ov)
        g2 = g1.numpy().copy()
        if mode == 1:
            g2[1:] = 0.0  # the opacity image is one channel of the colours-one image
        b2 = oracle.backward(sc2, dict(fw2, image=im2, color=im2["color"]), g2, ov)
        for k in ("means3D", "means2D", "opacities", "cov3D_precomp"):
            want[k] = want[k] + b2[k]
    for k in ("means3D", "means2D", "opacities", "cov3D_precomp", "colors_precomp"):
        err = _bulk_close(got[k], want[k].reshape(got[k].shape), tol=TOL, frac=0.0, name="%s: %s" % (tag, k))
        print("   ", k, "max error / tensor maximum: %.3g" % err)
    return st, got


LENGTHS = [1, 15, 16, 17, 31, 32, 33, 48, 49]


@pytest.mark.gpu
@pytest.mark.parametrize("m", LENGTHS)
def test_lists_around_a_round_one_image(oracle, monkeypatch, m):
    _run(oracle, monkeypatch, m, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3], ids=["with-opacity", "second-image-arbitrary-colours", "second-image-colours-one"])
@pytest.mark.parametrize("m", [16, 17, 33])
def test_lists_around_a_round_other_kernel_modes(oracle, monkeypatch, m, mode):
    _run(oracle, monkeypatch, m, mode)


BWD_CH = 128  # csrc/common.h: the forward cuts a quadrant's compacted list at every multiple of BWD_CH (a multiple of 16)


@pytest.mark.gpu
def test_chunked_backward_full_chunks_and_last_chunks_ending_inside_a_round(oracle, monkeypatch):
    """Lists of a few hundred entries on the same image: the backward runs one wave per (quadrant, chunk) from the forward's
    checkpoints (each lane now reads the checkpoint of the pixel it starts with).  A chunk starts at a multiple of 128
    compacted entries, so a wave of a full chunk walks exactly 128 entries -- eight rounds and the drain -- and what varies is
    the LAST chunk of a quadrant, qcount - 128 c entries: a third of the Gaussians are small and reach some quadrants only,
    so these lengths differ from quadrant to quadrant, and the test requires last chunks that end inside a round with the last
    round of either parity.  Against the oracle, and against the one-wave walk of the same frame (gs_tuning "bwd_chunks" = 0) at
    the 2e-6 of test_long_lists_on_a_small_image_backward_in_chunks -- and NOT bit for bit: the walk from a checkpoint starts
    from Gtot minus the composited colour in one step, the whole walk subtracts entry by entry, so equal bits everywhere
    would mean the chunked path did not run."""
    from gsplat_mi355 import _lib
    m = 420
    cc = _stack(m, seed=9, opacity=(0.012, 0.02), small=140)  # T >= 0.98^420 = 2e-4
    st, chunked = _run(oracle, monkeypatch, m, 0, cloud_cam=cc, check_lists=False)
    qc = st["image"]["qcount"].astype(np.int64).reshape(-1)
    long_q = qc[qc > BWD_CH]
    last = long_q - BWD_CH * ((long_q - 1) // BWD_CH)  # entries of the quadrant's last chunk
    parity = ((last + 14) // 16) & 1                   # of its last round (the loop runs last + 15 steps)
    print("quadrants of more than one chunk:", long_q.tolist(), "last chunks:", last.tolist())
    assert long_q.size >= 8 and int(long_q.max()) > 2 * BWD_CH  # several quadrants in chunks, some in three or more
    inside = last % 16 != 0
    assert (inside & (parity == 0)).any() and (inside & (parity == 1)).any(), (last.tolist(), parity.tolist())
    _lib.tuning("bwd_chunks", 0)
    try:
        _, whole = _run(oracle, monkeypatch, m, 0, cloud_cam=cc, check_lists=False)
    finally:
        _lib.tuning("bwd_chunks", 1)
    differing = 0
    for k in chunked:
        scale = np.abs(whole[k]).max()
        assert scale > 0 and np.abs(chunked[k] - whole[k]).max() <= 2e-6 * scale, (k, np.abs(chunked[k] - whole[k]).max() / scale)
        differing += int((chunked[k].view(np.uint32) != whole[k].view(np.uint32)).sum())
    print("elements whose bits differ between the chunked and the whole walk:", differing)
    assert differing > 0  # the two runs took different paths
