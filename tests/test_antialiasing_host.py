"""The rasterizer's `antialiasing` option on the CPU (no GPU needed): upstream's 13-field settings tuple with the
reference's 12-field construction unchanged, the new trailing field of GsFwdArgs in the binding and in the header (in what
was tail padding: the struct's size does not change), the geometry cache key and the debug dump, and the float64
restatement tests/antialias_ref.py -- whose three added gradient terms are checked against torch float64 autograd of its
own forward, which is what fixes their signs and the factor on b."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import abi_header
import antialias_ref as ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(*tail):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(80, 96, 0.5, 0.4, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3),
                                         False, False, *tail)


def test_settings_tuple_takes_twelve_or_thirteen_fields():
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields[-3:] == ("prefiltered", "debug", "antialiasing")
    assert len(GaussianRasterizationSettings._fields) == 13
    s12 = _settings()
    assert s12.antialiasing is False and len(s12) == 13
    assert _settings(True).antialiasing is True
    assert _settings(False).antialiasing is False
    kw = s12._replace(antialiasing=True)
    assert kw.antialiasing is True and kw[:12] == s12[:12]


def test_struct_field_is_last_in_binding_and_header_and_fills_tail_padding():
    from gsplat_mi355 import _lib
    assert _lib.GsFwdArgs._fields_[-1] == ("antialiasing", ctypes.c_int32)
    assert _lib.GsFwdArgs._fields_[-2] == ("forward_only", ctypes.c_int32)
    header = abi_header.text()
    assert [f.name for f in abi_header.parse().structs["GsFwdArgs"][-2:]] == ["forward_only", "antialiasing"]
    size = ctypes.sizeof(_lib.GsFwdArgs)
    assert size % 8 == 0
    # the field sits right behind forward_only, in what was tail padding: no earlier offset and not the size changed
    assert _lib.GsFwdArgs.antialiasing.offset == _lib.GsFwdArgs.forward_only.offset + 4 == size - 4
    capture = header[header.index("Stream capture"):header.index("typedef struct GsFwdArgs {")]
    assert "GsFwdArgs.antialiasing changes nothing about capture safety" in capture
    shared = header[header.index("shared-geometry forward"):header.index("int gs_forward_shared(")]
    assert "a->antialiasing" in shared


def test_geometry_cache_key_tells_the_flag_apart_and_the_dump_carries_it(tmp_path):
    import diff_gaussian_rasterization as dgr
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    sc, rot = torch.ones(4, 3), torch.ones(4, 4)
    base = _settings()
    keys = [dgr._geom_cache.key(s, m, o, sc, rot, None, stream_handle=0)
            for s in (base, base._replace(antialiasing=False), base._replace(antialiasing=True))]
    assert keys[0]["scalars"] == keys[1]["scalars"] and keys[0]["sigs"] == keys[1]["sigs"]
    assert keys[0]["scalars"] != keys[2]["scalars"] and keys[0]["sigs"] == keys[2]["sigs"]
    path = str(tmp_path / "snapshot_fw.dump")
    dgr._dump_snapshot(path, _settings(True), (m, o))
    snap = torch.load(path)
    assert snap["settings"]["antialiasing"] is True and len(snap["settings"]) == 13


def test_pipe_carries_the_option():
    from gsplat_mi355.render import Pipe
    assert Pipe().antialiasing is False and Pipe(antialiasing=True).antialiasing is True


def test_clamp_constant_is_the_square_root_of_the_ratio_floor():
    """s = sqrt(max(0.000025, r)): the clamped value the kernels use is the constant 0.005f, the correctly rounded fp32
    square root of the fp32 floor."""
    assert np.sqrt(np.float32(ref.R_MIN)) == np.float32(ref.S_MIN)
    assert abs(math.sqrt(ref.R_MIN) - ref.S_MIN) < 1e-15


def test_added_terms_match_float64_autograd_of_the_scaling():
    """o' = o s as a function of (a0, b, c0) alone: d(sum gO o')/d(a0, b, c0) by autograd against the three closed forms
    of the header; rows inside the clamp (a degenerate det0 <= 0 among them) get exactly zero."""
    g = torch.Generator().manual_seed(5)
    n = 4096
    l1 = torch.empty(n, dtype=torch.float64).uniform_(-4, 4, generator=g).exp()   # eigenvalues from 0.02 to 55 px^2
    l2 = torch.empty(n, dtype=torch.float64).uniform_(-4, 4, generator=g).exp()
    th = torch.empty(n, dtype=torch.float64).uniform_(0, math.pi, generator=g)
    c, s = torch.cos(th), torch.sin(th)
    a0 = l1 * c * c + l2 * s * s
    c0 = l1 * s * s + l2 * c * c
    b = (l1 - l2) * c * s
    a0[:8], c0[:8], b[:8] = 1e-7, 1e-7, 0.0      # far inside the clamp
    a0[8:12], c0[8:12], b[8:12] = 1.0, 1.0, 1.2  # det0 = -0.44 < 0 < det1 = 0.25
    o = torch.empty(n, dtype=torch.float64).uniform_(0.05, 0.99, generator=g)
    gO = torch.randn(n, dtype=torch.float64, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (a0, b, c0)]
    sc, free = ref.scaling(*leaves)
    assert not free[:12].any() and free[12:].all()
    assert torch.equal(sc[:12], torch.full((12,), ref.S_MIN, dtype=torch.float64))
    want = torch.autograd.grad((gO * o * sc).sum(), leaves)
    got = ref.added_terms(gO, (o * sc).detach(), a0, b, c0)
    for name, w, x in zip("abc", want, got):
        assert torch.equal(x[:12], torch.zeros(12, dtype=torch.float64)), name
        assert float((w - x).abs().max()) <= 1e-12 * float(w.abs().max()), name
    assert float(got[1].abs().max()) > 0  # the off-diagonal term is exercised


@pytest.mark.parametrize("cov_mode", ["scale_rot", "cov3d"])
def test_chain_of_the_restatement_is_the_added_terms_pushed_through_the_projection(cov_mode):
    """antialias_ref.Scene.chain (autograd of sum(gO o') through the whole restatement) equals the three closed-form terms
    pushed through autograd of the projection alone: the closed forms and the chain the GPU tests use agree."""
    cloud, cam = helpers.cloud_and_camera(512, 96, 80, scale_mul=0.05, seed=2)
    kw = (dict(scales=cloud.scales.numpy(), rotations=cloud.rotations.numpy()) if cov_mode == "scale_rot"
          else dict(cov6=helpers.covariance6_cpu(cloud).numpy()))
    wv = cam.world_view_transform.numpy().astype(np.float64)
    z = cloud.xyz.numpy().astype(np.float64) @ wv[:3, 2] + wv[3, 2]
    vis = z > 0.2
    sc = ref.Scene(cloud.xyz.numpy(), cloud.opacity.numpy(), cam.world_view_transform.numpy(), 96, 80,
                   math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), rows=vis, **kw)
    gO = np.random.default_rng(0).standard_normal(512).astype(np.float32).astype(np.float64)  # (a device gradient: fp32 values)
    chain = sc.chain(gO)
    f = sc.forward()
    assert float(f["s"].detach().min()) < 0.5 and bool(f["free"].any())
    ga, gb, gc = ref.added_terms(torch.from_numpy(gO[vis]), f["o_eff"].detach(), f["a0"].detach(), f["b"].detach(),
                                 f["c0"].detach())
    leaves = [sc.means] + ([sc.cov6] if sc.cov6 is not None else [sc.sv, sc.rot])
    pushed = torch.autograd.grad((ga * f["a0"] + gb * f["b"] + gc * f["c0"]).sum(), leaves)
    for name, p in zip(chain, pushed):
        w = chain[name][vis]
        assert np.abs(w).max() > 0, name
        assert np.abs(w - p.numpy()).max() <= 1e-10 * np.abs(w).max(), name
        assert not chain[name][~vis].any(), name
