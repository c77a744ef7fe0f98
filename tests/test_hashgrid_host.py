"""The hash-grid encoding's C ABI, restatement and drop-in module on the CPU (no GPU needed): the symbols are declared
and exported, the level table of the reference's config is exact, argument validation works without a device, the float64
restatement tests/hashgrid_ref.py agrees with hand-worked indices and with finite differences, and tinycudann.Encoding
builds its parameters on the CPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import abi_header
import hashgrid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_hashgrid_levels", "gs_hashgrid_workspace_bytes", "gs_hashgrid_forward", "gs_hashgrid_backward")
# the reference's configs/non_rigid/hashgrid.yaml block, after HashGrid.__init__ folded max_resolution into per_level_scale
REF_CFG = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 16, "base_resolution": 16,
           "per_level_scale": float(np.exp(np.log(2048 / 16) / 15)), "max_resolution": 2048}
REF_OFFSETS = [0, 4096, 16264, 46056] + [46056 + 65536 * k for k in range(1, 14)]
BAD_ARG, TOO_LARGE = -1, -3


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


def _table(cfg):
    from gsplat_mi355 import hashgrid
    return hashgrid.levels(hashgrid.parse_config(3, cfg))


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert "gs_hashgrid_forward, gs_hashgrid_backward" in abi_header.text()  # listed as capture-safe


def test_reference_level_table(lib):
    assert abs(REF_CFG["per_level_scale"] - 1.3819128799677760) < 1e-15
    offsets, scales, res, n_params = _table(REF_CFG)
    assert list(offsets) == REF_OFFSETS
    assert n_params == 1796048
    assert list(res[:3]) == [16, 23, 31]
    assert scales[0] == 15.0
    # levels 0-2 dense (res^3 rounded up to 8 fits 2^16), 3-15 hashed (2^16 rows)
    for l in range(16):
        size = offsets[l + 1] - offsets[l]
        dense = -(-res[l] ** 3 // 8) * 8
        assert size == min(dense, 1 << 16)
        assert (size < 65536) == (l < 3)
    # the float32 host arithmetic of the spec
    log2b = np.float32(math.log2(np.float64(np.float32(REF_CFG["per_level_scale"]))))
    for l in range(16):
        s = np.float32(np.exp2(np.float32(l) * log2b, dtype=np.float32) * np.float32(16) - np.float32(1))
        assert abs(float(s) - scales[l]) <= 2 * float(np.spacing(np.float32(s))), l
        assert res[l] == int(math.ceil(scales[l])) + 1


def test_tcnn_defaults(lib):
    offsets, scales, res, n_params = _table({"otype": "HashGrid"})
    assert len(scales) == 16 and n_params == offsets[-1] * 2
    assert offsets[-1] - offsets[-2] == 1 << 19
    assert res[0] == 16 and scales[1] == 31.0 and res[1] == 32


def test_bad_configs_and_sizes(lib):
    L = lib.load()
    G = lib.GsHashGrid
    good = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=16, base_resolution=16, per_level_scale=1.38)
    out = ctypes.c_size_t(0)
    n = ctypes.c_int32(0)
    g = G(**good)
    assert L.gs_hashgrid_levels(ctypes.byref(g), None, None, None, ctypes.byref(n)) == 0 and n.value == 1796048
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), 200000, ctypes.byref(out)) == 0
    assert out.value >= 8 * 16 * 200000 * 16 + (898024 + 1) * 4 and out.value % 256 == 0
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), 0, ctypes.byref(out)) == 0
    for k, v in (("n_levels", 0), ("n_levels", 33), ("n_features_per_level", 3), ("n_features_per_level", 16),
                 ("log2_hashmap_size", 0), ("log2_hashmap_size", 31), ("base_resolution", 0), ("per_level_scale", 0.5),
                 ("per_level_scale", float("nan"))):
        bad = G(**dict(good, **{k: v}))
        assert L.gs_hashgrid_levels(ctypes.byref(bad), None, None, None, None) == BAD_ARG, (k, v)
        assert L.gs_hashgrid_workspace_bytes(ctypes.byref(bad), 10, ctypes.byref(out)) == BAD_ARG, (k, v)
        assert L.gs_hashgrid_forward(ctypes.byref(bad), 10, 16, 16, 16, None) == BAD_ARG, (k, v)
    assert L.gs_hashgrid_levels(None, None, None, None, None) == BAD_ARG
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), -1, ctypes.byref(out)) == BAD_ARG
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), 10, None) == BAD_ARG
    # 8 L N >= 2^31: the sort's pair index
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), (1 << 31) // 128, ctypes.byref(out)) == TOO_LARGE
    assert L.gs_hashgrid_workspace_bytes(ctypes.byref(g), (1 << 31) // 128 - 1, ctypes.byref(out)) == 0
    assert L.gs_hashgrid_backward(ctypes.byref(g), (1 << 31) // 128, 16, 16, 16, None, 16, 16, 1 << 40, None) == TOO_LARGE
    # n_params >= 2^31
    huge = G(**dict(good, n_levels=32, n_features_per_level=8, log2_hashmap_size=30))
    assert L.gs_hashgrid_levels(ctypes.byref(huge), None, None, None, None) == TOO_LARGE
    # NULL operands, misaligned pointers (no device needed: rejected before any launch)
    assert L.gs_hashgrid_forward(ctypes.byref(g), 10, None, 16, 16, None) == BAD_ARG
    assert L.gs_hashgrid_forward(ctypes.byref(g), 10, 16, None, 16, None) == BAD_ARG
    assert L.gs_hashgrid_forward(ctypes.byref(g), 10, 16, 20, 16, None) == BAD_ARG
    assert L.gs_hashgrid_forward(ctypes.byref(g), 10, 16, 16, 20, None) == BAD_ARG
    assert L.gs_hashgrid_forward(ctypes.byref(g), -1, 16, 16, 16, None) == BAD_ARG
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, None, 16, 16, 16, 16, 16, 1 << 30, None) == BAD_ARG
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, 16, None, 16, 16, 16, 1 << 30, None) == BAD_ARG
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, None, 16, 16, None, None, 0, None) == BAD_ARG  # dL_dx needs params
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, 16, 16, None, 16, None, 0, None) == BAD_ARG  # no workspace
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, 16, 16, None, 16, 16, 64, None) == -5  # workspace too small
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, 16, 16, None, 20, 16, 1 << 30, None) == BAD_ARG
    # nothing wanted: nothing to do
    assert L.gs_hashgrid_forward(ctypes.byref(g), 10, 16, 16, None, None) == 0
    assert L.gs_hashgrid_backward(ctypes.byref(g), 10, 16, 16, 16, None, None, None, 0, None) == 0


def test_restatement_hand_worked_indices(lib):
    offsets, scales, res, _ = _table(REF_CFG)
    size = [offsets[l + 1] - offsets[l] for l in range(16)]
    # dense level 1 (res 23): corner (3, 4, 5) -> 3 + 4 * 23 + 5 * 529
    assert ref.corner_index(np.array([3, 4, 5], np.uint32), res[1], size[1]) == 3 + 4 * 23 + 5 * 529
    # x = (1, 1, 1) at level 0: pos = 15.5, far corner (16, 16, 16) -> 16 + 256 + 4096 = 4368 -> entry 272
    ent, w, t = ref.corners(np.ones((1, 3), np.float32), scales[0], res[0], size[0])
    assert list(ref.cells(np.ones((1, 3), np.float32), scales[0])[0][0]) == [15, 15, 15]
    assert np.all(t == 0.5)
    assert ent[0, 7] == 4368 - 4096 == 272
    assert ent[0, 0] == 15 + 15 * 16 + 15 * 256
    # x = (-0.05, 0, 0) at level 0: pos_0 = -0.25, cell coordinate 2^32 - 1 -> corner 0 lands on entry 4095
    xn = np.array([[-0.05, 0.0, 0.0]], np.float32)
    c, t = ref.cells(xn, scales[0])
    assert int(c[0, 0]) == 2 ** 32 - 1 and t[0, 0] == 0.75
    ent, w, _ = ref.corners(xn, scales[0], res[0], size[0])
    assert ent[0, 0] == 4095
    assert ent[0, 1] == 0  # v_0 wraps to 0
    # a hashed level (3: res 43, 43^3 > 2^16): the primes
    v = np.array([7, 11, 13], np.uint64)
    h = (7 * 1) ^ ((11 * 2654435761) & 0xFFFFFFFF) ^ ((13 * 805459861) & 0xFFFFFFFF)
    assert res[3] == 43 and size[3] == 65536
    assert ref.corner_index(v, res[3], size[3]) == h % 65536
    # a coarse hashed level where only two dims fit the stride test (res 2048: stride 2048^2 > 2^16 skips d = 2)
    assert res[15] == 2048
    assert ref.corner_index(v, res[15], size[15]) == h % 65536


def test_restatement_weights_and_continuity(lib):
    table = _table(REF_CFG)
    offsets, scales, res, n_params = table
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    for l in (0, 5, 15):
        _, w, _ = ref.corners(x, scales[l], res[l], offsets[l + 1] - offsets[l])
        assert np.allclose(w.sum(1), 1.0, atol=1e-12) and (w >= 0).all()
    params = rng.uniform(-1, 1, n_params)
    # across a face of level 0's cells (pos_0 = 8: x_0 = 7.5 / 15): the value is continuous
    x0 = np.float32(7.5 / 15)
    lo, hi = np.nextafter(x0, np.float32(0)), np.nextafter(x0, np.float32(1))
    pts = np.array([[lo, 0.3, 0.6], [x0, 0.3, 0.6], [hi, 0.3, 0.6]], np.float32)
    c, _ = ref.cells(pts, scales[0])
    assert c[0, 0] == 7 and c[2, 0] == 8
    out = ref.encode(pts, params, table, 2)
    assert np.abs(out[0, :2] - out[2, :2]).max() < 1e-5


def test_restatement_finite_difference(lib):
    cfg = dict(REF_CFG, n_levels=6, log2_hashmap_size=12)
    table = _table(cfg)
    rng = np.random.default_rng(1)
    n = 40
    x = rng.uniform(0.05, 0.95, (n, 3)).astype(np.float64)
    params = rng.uniform(-1, 1, table[3])
    G = rng.normal(size=(n, 12))
    dx, _ = ref.backward(x.astype(np.float32), params, G, table, 2)

    xf = x.astype(np.float32).astype(np.float64)

    def loss64(xx):  # the trilinear form in float64 around xf (cell and t of the float32 point, moved by scale (xx - xf))
        offsets, scales, res, _ = table
        th = params.reshape(-1, 2)
        tot = np.zeros(n)
        for l in range(len(scales)):
            _, t0 = ref.cells(xf, scales[l])
            t = t0 + np.float64(np.float32(scales[l])) * (xx - xf)
            ent, _, _ = ref.corners(xf, scales[l], res[l], offsets[l + 1] - offsets[l])
            for k in range(8):
                w = np.ones(n)
                for d in range(3):
                    w = w * (t[:, d] if (k >> d) & 1 else 1 - t[:, d])
                tot += w * (th[offsets[l] + ent[:, k]] * G[:, 2 * l:2 * l + 2]).sum(1)
        return tot
    h = 1e-6
    for d in range(3):
        e = np.zeros((n, 3))
        e[:, d] = h
        fd = (loss64(xf + e) - loss64(xf - e)) / (2 * h)
        assert np.allclose(fd, dx[:, d], rtol=1e-7, atol=1e-7 * np.abs(dx[:, d]).max()), d
    # and the parameter gradient is the transpose of the encoding: <G, encode(params)> is linear in params
    _, dp = ref.backward(x.astype(np.float32), params, G, table, 2)
    p2 = rng.uniform(-1, 1, table[3])
    lhs = (ref.encode(x.astype(np.float32), p2, table, 2) * G).sum()
    assert abs(lhs - (dp * p2).sum()) < 1e-9 * max(1.0, abs(lhs))


def test_tinycudann_encoding_on_cpu(lib):
    import torch
    import tinycudann as tcnn
    cfg = {k: v for k, v in REF_CFG.items()}  # no otype, as in the reference's hashgrid: block
    enc = tcnn.Encoding(3, cfg)
    assert enc.n_input_dims == 3 and enc.n_output_dims == 32 and enc.dtype == torch.float32
    assert list(dict(enc.named_parameters())) == ["params"]
    assert enc.params.numel() == 1796048 and enc.params.dtype == torch.float32 and enc.params.device.type == "cpu"
    p = enc.params.detach()
    assert float(p.abs().max()) <= 1e-4 and float(p.std()) > 3e-5
    assert torch.equal(p, tcnn.Encoding(3, cfg, seed=1337).params.detach())
    assert not torch.equal(p, tcnn.Encoding(3, cfg, seed=7).params.detach())
    assert list(enc.state_dict()) == ["params"]
    assert tcnn.Encoding(3, dict(cfg, otype="hashgrid")).n_output_dims == 32
    assert tcnn.Encoding(3, dict(cfg, otype="Grid", type="hash")).n_output_dims == 32
    assert tcnn.Encoding(3, cfg, dtype=torch.float16).dtype == torch.float16
    with pytest.raises(RuntimeError, match="GPU"):
        enc(torch.zeros(4, 3))
    for bad, key in ((dict(cfg, otype="Frequency"), "otype"), (dict(cfg, otype="Grid", type="Dense"), "type"),
                     (dict(cfg, interpolation="Smoothstep"), "interpolation"), (dict(cfg, hash="Prime"), "hash"),
                     (dict(cfg, n_features_per_level=3), "n_features_per_level")):
        with pytest.raises(NotImplementedError, match=key):
            tcnn.Encoding(3, bad)
    with pytest.raises(NotImplementedError, match="n_input_dims"):
        tcnn.Encoding(2, cfg)
    with pytest.raises(ImportError, match="not provided"):
        from tinycudann import Network  # noqa: F401
    assert not hasattr(tcnn, "SomethingElse")
