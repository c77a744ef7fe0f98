"""The forward's quadrant test (csrc/blend.h: stage_entry_quad) -- which tile-list entries a quadrant wave compacts into its
list -- checked three ways:

* in the generated code (no GPU): no forward kernel holds a division sequence, and the large-image kernel keeps its eight
  waves per SIMD (at most 64 VGPRs, no scratch);
* on the CPU: a float32 numpy restatement of the test against a float64 evaluation of every pixel centre, on inputs built by
  the recipe the device test uses -- which must contain what exercises the test's branches (opacities just above 1 / 255: `thr`
  and the limit it sets; thin and nearly degenerate conics: `rel`);
* on the device (-m gpu): every entry with a pixel centre of alpha >= 1 / 255 (1 + 1e-5) in a quadrant, up to the quadrant's
  last contributor, is in the quadrant's recorded list.  No exempt share: zero misses.
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
ALPHA_MIN = (1.0 / 255.0) * (1.0 + 1e-5)


# ---------------------------------------------------------------------------------------------------------------
# generated code
# ---------------------------------------------------------------------------------------------------------------
def _forward_code_object():
    """(disassembly per kernel symbol, metadata per kernel name) of the gfx950 code object inside build/render_fwd.o."""
    obj = os.path.join(PKG, "build", "render_fwd.o")
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
    tmp = tempfile.mkdtemp(prefix="gs_fwd_code_")
    try:
        local = os.path.join(tmp, "render_fwd.o")
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


def test_no_forward_kernel_divides_and_the_large_image_kernel_keeps_eight_waves():
    code, meta = _forward_code_object()
    kernels = [k for k in code if re.search(r"render_fwd(_small)?_kernel", k)]
    assert len(kernels) == 4, kernels  # two kernels, each for a first and a second render
    for k in kernels:
        assert len(code[k]) > 200, k
        bad = [i for i in code[k] if i.startswith(("v_div_scale_f32", "v_div_fixup_f32", "v_div_fmas_f32"))]
        assert not bad, "%s: %d division instructions, e.g. %s" % (k, len(bad), bad[0])
    # the test is still there: the first-render kernels take reciprocals (v_rcp_f32) and clamp with v_med3_f32
    for k in kernels:
        if "ILb0" in k:
            assert sum(i.startswith("v_rcp_f32") for i in code[k]) >= 4 and any(i.startswith("v_med3_f32") for i in code[k]), k
    main = [k for k in meta if re.search(r"render_fwd_kernel", k)]
    assert len(main) == 2, main
    for k in main:
        print(k, meta[k])
        assert meta[k]["vgpr_count"] <= 64, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0 and meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
    for k in meta:  # the other forward kernels: no scratch either (a kernel with scratch is dispatched into the scratch ring's slots)
        if "render_fwd" in k:
            assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])


# ---------------------------------------------------------------------------------------------------------------
# inputs, the float64 pixel evaluation, the float32 restatement of the test
# ---------------------------------------------------------------------------------------------------------------
def _stress_cloud(n, W, H, layout, dist2_fn=None):
    """The synthetic cloud of a benchmark shape with every 16th Gaussian made a needle (a few of them long enough for a conic
    that is degenerate in fp32) and every 16th given an opacity around 1 / 255."""
    cloud, cam = helpers.cloud_and_camera(n, W, H, sh_degree=1, seed=3, layout=layout, dist2_fn=dist2_fn)
    g = torch.Generator().manual_seed(11)
    idx = torch.arange(n)
    needle = idx % 16 == 0
    m = int(needle.sum())
    major = torch.empty(m).uniform_(0.02, 0.4, generator=g)
    major[::24] = 10.0  # thousands of pixels long: A C / det beyond what fp32 resolves
    sc = cloud.scales.clone()
    sc[needle] = torch.stack([major, torch.full((m,), 1e-4), torch.full((m,), 1e-4)], 1)
    cloud.scales = sc.contiguous()
    low = idx % 16 == 1
    op = cloud.opacity.clone()
    op[low] = torch.empty(int(low.sum()), 1).uniform_(0.002, 0.03, generator=g)
    cloud.opacity = op.contiguous()
    return cloud, cam


def _contributing(rows, tx, ty, W, H):
    """float64: [n, 4] -- has entry i a pixel centre of quadrant q of tile (tx, ty), inside the image, with
    opacity exp(power) >= 1 / 255 (1 + 1e-5)?  `rows`: [n, 6] = x, y, A, B, C, opacity."""
    r = rows.astype(np.float64)
    px = (tx * 16 + np.arange(16, dtype=np.float64))[None, None, :]
    py = (ty * 16 + np.arange(16, dtype=np.float64))[None, :, None]
    dx = r[:, 0, None, None] - px
    dy = r[:, 1, None, None] - py
    power = -0.5 * (r[:, 2, None, None] * dx * dx + r[:, 4, None, None] * dy * dy) - r[:, 3, None, None] * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        ok = r[:, 5, None, None] * np.exp(power) >= ALPHA_MIN
    ok &= (px < W) & (py < H)
    return np.stack([ok[:, 8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8].any(axis=(1, 2)) for q in range(4)], 1)


def _quad_test_f32(rows, QX0, QY0):
    """csrc/blend.h: stage_entry_quad, restated in float32 numpy (products and sums rounded one by one, reciprocals correctly
    rounded: the device contracts to FMAs and takes 1-ulp reciprocals -- differences the test's slack is there for).
    Returns (hit, branch) with branch 0: thr > 0, never; 1: A <= 0 or C <= 0, always; 2: det <= 0 or rel >= 0.5, always;
    3: the centre lies in the rectangle; 4: decided by the comparison."""
    f = np.float32
    gx, gy, A, B, C, o = (rows[:, i].astype(f) for i in range(6))
    with np.errstate(all="ignore"):
        thr = -np.log2(f(255.0) * o).astype(f) - f(1e-3)
        two_tau = f(-2.0 / 1.4426950408889634) * thr
        x0 = f(QX0) - gx
        x1 = x0 + f(7.0)
        y0 = f(QY0) - gy
        y1 = y0 + f(7.0)
        inside = (x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0)
        b2 = f(2.0) * B
        ky, kx = -B * (f(1.0) / C), -B * (f(1.0) / A)

        def edge(axx, b2x, c, k, lo, hi):
            ys = np.minimum(np.maximum(k, lo), hi)
            return axx + (b2x + c * ys) * ys
        qmin = np.minimum(np.minimum(edge(A * x0 * x0, b2 * x0, C, ky * x0, y0, y1), edge(A * x1 * x1, b2 * x1, C, ky * x1, y0, y1)),
                          np.minimum(edge(C * y0 * y0, b2 * y0, A, kx * y0, x0, x1), edge(C * y1 * y1, b2 * y1, A, kx * y1, x0, x1)))
        AC = A * C
        detc = AC - B * B
        rel = f(1e-4) + AC * (f(1.0) / detc) * f(1.9073486e-6)
        lim = (two_tau + f(1e-3)) * (f(1.0) / (f(1.0) - rel)) * f(1.0 + 2.0 ** -20)
        cmp_hit = ~(qmin > lim)
    branch = np.full(len(rows), 4, np.int32)
    branch[inside] = 3
    branch[~(detc > 0) | ~(rel < 0.5)] = 2
    branch[~((A > 0) & (C > 0))] = 1
    branch[~(thr <= 0)] = 0
    hit = np.where(branch == 4, cmp_hit, branch != 0)
    return hit, branch


def _branch_coverage(rows):
    """What the inputs hold, per list entry: (opacity under the threshold, degenerate in fp32, thin but decided, low opacity
    but decided)."""
    _, br = _quad_test_f32(rows, 0, 0)
    A, B, C, o = (rows[:, i].astype(np.float64) for i in (2, 3, 4, 5))
    with np.errstate(all="ignore"):
        ratio = A * C / (A * C - B * B)
    decided = br >= 3
    return int((br == 0).sum()), int((br == 2).sum()), int((decided & (ratio > 1e3)).sum()), int((decided & (o < 0.02)).sum())


CASES = [("config4", 200000, 512, 512, "box"), ("body", 200000, 512, 512, "body")]


@pytest.mark.parametrize("case,n,W,H,layout", [(c, 12000, W, H, lay) for c, _, W, H, lay in CASES], ids=[c[0] for c in CASES])
def test_restated_quadrant_test_keeps_every_contributing_pair_and_the_inputs_reach_its_branches(case, n, W, H, layout):
    from oracle import gs_oracle
    gs_oracle.build()
    cloud, cam = _stress_cloud(n, W, H, layout)
    sc = helpers.oracle_scene(cloud, cam)
    st = gs_oracle.preprocess(sc)
    bn = gs_oracle.binning(sc, st)
    rec = np.concatenate([st["xy"], st["conic_opacity"]], 1)  # x, y, A, B, C, opacity
    pl, ranges = bn["point_list"], bn["ranges"].astype(np.int64)
    assert bn["D"] > 20000
    cov = _branch_coverage(rec[pl])
    print(case, "entries", bn["D"], "under threshold / degenerate / thin / low opacity:", cov)
    assert min(cov[1:]) > 0, cov  # (the preprocess step lists no Gaussian whose opacity is under the threshold: cov[0] is 0)
    gx = (W + 15) // 16
    need_n = kept_n = dropped_n = misses = 0
    for t in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        rows = rec[pl[ranges[t, 0]:ranges[t, 1]]]
        tx, ty = int(t % gx), int(t // gx)
        need = _contributing(rows, tx, ty, W, H)
        for q in range(4):
            hit, _ = _quad_test_f32(rows, tx * 16 + 8 * (q & 1), ty * 16 + 8 * (q >> 1))
            misses += int((need[:, q] & ~hit).sum())
            need_n += int(need[:, q].sum())
            kept_n += int(hit.sum())
            dropped_n += int((~hit).sum())
    print(case, "contributing", need_n, "kept", kept_n, "dropped", dropped_n, "misses", misses)
    assert misses == 0
    assert need_n > 0 and dropped_n > kept_n // 4  # (a test that keeps everything would pass the line above, too)


# ---------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,n,W,H,layout", CASES, ids=[c[0] for c in CASES])
def test_device_quadrant_lists_hold_every_contributing_entry(case, n, W, H, layout):
    """Device records and lists (gsplat_mi355.debug.forward_state), float64 numpy: misses allowed = 0.  Measured on the
    MI355X (list entries / contributing (quadrant, entry) pairs up to the last contributor / entries in the quadrant lists /
    misses): config4 2 276 748 / 1 280 286 / 2 129 780 / 0; body 1 670 097 / 439 605 / 1 665 867 / 0."""
    from gsplat_mi355 import debug
    from simple_knn._C import distCUDA2
    from test_gpu_parity import _settings
    dev = torch.device("cuda:0")
    cloud, cam = _stress_cloud(n, W, H, layout, dist2_fn=lambda p: distCUDA2(p.to(dev)).cpu())
    st = debug.forward_state(_settings(cam, cloud, (0.0, 0.0, 0.0), dev), cloud.xyz.to(dev), cloud.opacity.to(dev),
                             shs=cloud.shs.to(dev), scales=cloud.scales.to(dev), rotations=cloud.rotations.to(dev))
    D = st["D"]
    assert D > 300000
    rec = st["geom"]["rec"][:, :6]  # x, y, A, B | C, opacity
    pl, qlist = st["binning"]["point_list"], st["binning"]["qlist"]
    ranges = st["image"]["ranges"].astype(np.int64)
    qcount, ncon = st["image"]["qcount"].astype(np.int64), st["image"]["n_contrib"].astype(np.int64)
    assert qlist.shape == (4 * D,)
    cov = _branch_coverage(rec[pl])
    print(case, "entries", D, "under threshold / degenerate / thin / low opacity:", cov)
    assert min(cov[1:]) > 0, cov  # (the preprocess step lists no Gaussian whose opacity is under the threshold: cov[0] is 0)
    gx = (W + 15) // 16
    must_n = listed_n = misses = 0
    for t in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        r0, r1 = ranges[t]
        nt = int(r1 - r0)
        ids = pl[r0:r1]
        tx, ty = int(t % gx), int(t // gx)
        need = _contributing(rec[ids], tx, ty, W, H)
        pos1 = np.arange(1, nt + 1)
        for q in range(4):
            qc = int(qcount[t, q])
            assert qc <= nt
            qs = qlist[4 * r0 + q * nt:4 * r0 + q * nt + qc]
            y0, x0 = ty * 16 + 8 * (q >> 1), tx * 16 + 8 * (q & 1)
            last = int(ncon[y0:y0 + 8, x0:x0 + 8].max()) if y0 < H and x0 < W else 0  # 1-based position in the tile's list
            assert (last == 0) == (qc == 0)
            if last:
                assert qs[-1] == ids[last - 1]  # the list ends with the quadrant's last contributor
            must = need[:, q] & (pos1 <= last)
            misses += int((must & ~np.isin(ids, qs)).sum())
            must_n += int(must.sum())
            listed_n += qc
    print(case, "contributing up to the last contributor", must_n, "listed", listed_n, "misses", misses)
    assert must_n > 100000 and listed_n >= must_n
    assert misses == 0
