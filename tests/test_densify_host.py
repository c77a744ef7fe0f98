"""The densification cycle's C ABI and fixture on the CPU (no GPU needed): the new symbols are declared and exported,
argument validation and workspace sizes work without a device, and tests/golden/densify.npz is self-consistent (row
counts and row order follow from the masks, children's scalings from their sources', the values that travel with the
rows are formed again exactly)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_densify_golden as mdg  # noqa: E402
NEW = ("gs_densify_workspace_bytes", "gs_densify_plan", "gs_densify_apply", "gs_reset_opacity")


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    import gsplat_mi355.densify as d
    assert callable(d.densify_and_prune) and callable(d.reset_opacity) and callable(d.prune_points)


def test_workspace_sizes(lib):
    L = lib.load()
    sizes = [lib.nbytes(L.gs_densify_workspace_bytes, n) for n in (0, 1, 1000, 200000, 500000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    for n, s in zip((1, 1000, 200000, 500000), sizes[1:]):
        assert s >= n * (1 + 2 * 4) + 16  # flags, the map of up to 2 N rows, the totals
        assert s % 256 == 0
    out = ctypes.c_size_t(0)
    assert L.gs_densify_workspace_bytes(-1, ctypes.byref(out)) == -1
    assert L.gs_densify_workspace_bytes(1 << 30, ctypes.byref(out)) == -1
    assert L.gs_densify_workspace_bytes(10, None) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    fake = 0x1000  # never dereferenced: validation fails first
    ws_bytes = lib.nbytes(L.gs_densify_workspace_bytes, 10)
    p = lib.GsDensifyPlan(N=10, scaling=fake, opacity=fake, grad_accum=fake, denom=None)
    assert L.gs_densify_plan(ctypes.byref(p), fake, ws_bytes, None, None) == -1        # densify mode needs denom
    p.denom = fake
    assert L.gs_densify_plan(None, fake, ws_bytes, None, None) == -1                   # no plan
    assert L.gs_densify_plan(ctypes.byref(p), None, ws_bytes, None, None) == -1        # no workspace
    assert L.gs_densify_plan(ctypes.byref(p), fake, ws_bytes - 1, None, None) == -5    # workspace too small
    p.N = -1
    assert L.gs_densify_plan(ctypes.byref(p), fake, ws_bytes, None, None) == -1
    T = lib.GsDensifyTensor
    good = T(fake, fake, 3, lib.GS_DENSIFY_COPY)
    arr = lambda *ts: (T * len(ts))(*ts)
    apply = lambda n, n_new, ts, ws=fake, nb=ws_bytes, k=None, sc=fake, ro=fake, no=fake: L.gs_densify_apply(
        n, n_new, ws, nb, len(ts) if k is None else k, arr(*ts) if ts else None, sc, ro, no, None)
    assert apply(10, 21, [good]) == -1                                                # N' > 2 N
    assert apply(-1, 0, [good]) == -1
    assert apply(10, 5, [T(fake, fake, 0, lib.GS_DENSIFY_COPY)]) == -1               # row width 0
    assert apply(10, 5, [T(fake, fake, 3, 7)]) == -1                                 # unknown kind
    assert apply(10, 5, [T(None, fake, 3, lib.GS_DENSIFY_COPY)]) == -1               # NULL source
    assert apply(10, 5, [T(fake, None, 3, lib.GS_DENSIFY_COPY)]) == -1               # NULL destination
    assert apply(10, 5, [T(fake, fake, 4, lib.GS_DENSIFY_CHILD_POSITION)]) == -1     # child position has width 3
    assert apply(10, 5, [T(fake, fake, 3, lib.GS_DENSIFY_CHILD_POSITION)], no=None) == -1  # ... and needs the noise
    assert apply(10, 5, [good] * 25) == -1                                           # more than GS_DENSIFY_MAX_TENSORS
    assert apply(10, 5, [good], k=-1) == -1
    assert apply(10, 5, [good], ws=None) == -1
    assert apply(10, 5, [good], nb=ws_bytes - 1) == -5
    # N' = 0 and N = 0 are legal no-ops (nothing is enqueued)
    assert apply(10, 0, [T(fake, None, 3, lib.GS_DENSIFY_COPY)]) == 0
    assert apply(0, 0, [T(None, None, 3, lib.GS_DENSIFY_ZERO)], nb=lib.nbytes(L.gs_densify_workspace_bytes, 0)) == 0
    assert L.gs_reset_opacity(-1, fake, fake, None, None, None) == -1
    assert L.gs_reset_opacity(10, None, fake, None, None, None) == -1
    assert L.gs_reset_opacity(10, fake, None, None, None, None) == -1
    assert L.gs_reset_opacity(0, None, None, None, None, None) == 0


@pytest.mark.parametrize("tag", ["d1", "d2", "d3"])
def test_fixture_is_self_consistent(fx, tag):
    clone, split, prune = fx[tag + "/clone"], fx[tag + "/split"], fx[tag + "/prune"]
    src, slot = fx[tag + "/src"], fx[tag + "/slot"]
    n = clone.shape[0]
    assert fx["in_%s/xyz" % tag].shape[0] == n and fx[tag + "/z"].shape == (int(split.sum()), 2, 3)
    assert not (clone & split).any() and clone.any() and split.any()
    # the concatenated set: originals not split, clones, first children, second children
    n_cat = int((~split).sum() + clone.sum() + 2 * split.sum())
    assert prune.shape == (n_cat,)
    assert src.shape[0] == n_cat - prune.sum()
    assert fx[tag + "/xyz"].shape == fx[tag + "/scaling"].shape == (int((slot >= 2).sum()), 3)
    assert np.all(np.diff(slot.astype(int)) >= 0)  # segments in order
    for s, sel in ((0, ~split), (1, clone), (2, split), (3, split)):
        assert np.all(np.isin(src[slot == s], np.nonzero(sel)[0]))
        assert np.all(np.diff(src[slot == s]) > 0)  # source order inside a segment
    assert np.array_equal(src[slot == 2], src[slot == 3])  # a source's two children share their fate
    # the children's scaling is log(exp(s) / 1.6) of their source's, both copies alike
    s_in = fx["in_%s/scaling" % tag][src[slot >= 2]].astype(np.float64)
    assert np.allclose(fx[tag + "/scaling"], np.log(np.exp(s_in) / 1.6), rtol=0, atol=1e-5)
    half = int((slot == 2).sum())
    assert np.array_equal(fx[tag + "/scaling"][:half], fx[tag + "/scaling"][half:])
    assert np.abs(fx[tag + "/z"]).max() > 0
    # the values that travel with the rows are formed again from (phase, N), exactly and with the right shapes
    pas = mdg.passengers(tag, n)
    assert all(np.array_equal(v, w) for v, w in zip(pas.values(), mdg.passengers(tag, n).values()))
    for k, shp in mdg.shapes(n).items():
        assert pas["exp_avg." + k].shape == pas["exp_avg_sq." + k].shape == shp and (pas["exp_avg_sq." + k] >= 0).all()
        assert fx["in_%s/step.%s" % (tag, k)] > 0
    assert pas["f_rest"].shape == (n, 15, 3)
    # the quirk: max_radii2D is large where the prune test would read it, and nothing was pruned for it
    if float(fx[tag + "/max_screen_size"]) > 0:
        assert (fx["in_%s/max_radii2D" % tag] > float(fx[tag + "/max_screen_size"])).mean() > 0.9


def test_fixture_reset_opacity(fx):
    n = fx["d2/src"].shape[0]
    o = fx["r/opacity"]
    assert o.shape == (n, 1)
    assert np.all(1.0 / (1.0 + np.exp(-o.astype(np.float64))) <= 0.01 + 1e-7)


# ---- the numpy restatement (oracle/densify_ref.py) the GPU sweep compares against, tied to the reference's own results

KW = dict(grad_threshold=mdg.GRAD_THRESHOLD, percent_dense=mdg.PERCENT_DENSE, min_opacity=mdg.MIN_OPACITY)


def _close(got, want, rel=1e-6):  # test_gpu_densify.py's bar
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.all(np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("tag", ["d1", "d2", "d3"])
def test_restatement_reproduces_the_fixture(fx, tag):
    """Masks, row map and children of the restatement against what the reference's own densify_and_prune did."""
    from oracle import densify_ref
    p = "in_%s/" % tag
    size = float(fx[tag + "/max_screen_size"]) or None
    w = densify_ref.densify_and_prune(fx[p + "scaling"], fx[p + "opacity"], fx[p + "xyz_gradient_accum"], fx[p + "denom"],
                                      extent=float(fx[tag + "/extent"]), max_screen_size=size, **KW)
    assert np.array_equal(w["clone"], fx[tag + "/clone"]) and np.array_equal(w["split"], fx[tag + "/split"])
    assert np.array_equal(w["cat_prune"], fx[tag + "/prune"])
    assert np.array_equal(w["src"], fx[tag + "/src"]) and np.array_equal(w["slot"], fx[tag + "/slot"])
    assert w["n_new"] == len(fx[tag + "/src"])
    split = fx[tag + "/split"]
    noise = np.zeros((len(split), 2, 3), np.float32)
    noise[split] = fx[tag + "/z"]
    pos, scl = densify_ref.children(fx[p + "xyz"], fx[p + "scaling"], fx[p + "rotation"], noise, w["src"], w["slot"])
    assert _close(pos, fx[tag + "/xyz"]) and _close(scl, fx[tag + "/scaling"])
    # max_screen_size None and 0 are the same call
    if size is None:
        w0 = densify_ref.densify_and_prune(fx[p + "scaling"], fx[p + "opacity"], fx[p + "xyz_gradient_accum"],
                                           fx[p + "denom"], extent=float(fx[tag + "/extent"]), max_screen_size=0, **KW)
        assert np.array_equal(w0["src"], w["src"]) and np.array_equal(w0["slot"], w["slot"])


def test_restatement_reset_opacity_and_prune_points(fx):
    from oracle import densify_ref
    o = fx["in_d2/opacity"][fx["d2/src"]]  # the state reset_opacity saw: right after d2
    assert _close(densify_ref.reset_opacity(o), fx["r/opacity"])
    mask = np.zeros(10, bool)
    mask[[0, 3, 9]] = True
    src, slot = densify_ref.prune_points(mask)
    assert src.tolist() == [1, 2, 4, 5, 6, 7, 8] and not slot.any()


def test_row_map_is_the_last_workspace_region(lib):
    """Plan.row_map reads the map at ws_bytes - dn_align(8 N): pin the workspace layout of csrc/densify.hip (flags u8[N] |
    counts u32[3, blocks] | offsets u32[3, blocks] | totals u32[4] | map u32[2 N], each padded to 256 bytes)."""
    from gsplat_mi355.densify import Plan
    L = lib.load()
    al = lambda x: (x + 255) // 256 * 256
    for n in (0, 1, 1023, 1024, 1025, 262145, 1100001):
        nb = (n + 1023) // 1024
        ws = lib.nbytes(L.gs_densify_workspace_bytes, n)
        assert ws == al(n) + 2 * al(12 * nb) + al(16) + al(8 * n), n
        assert Plan.map_offset(n, ws) == ws - al(8 * n) == al(n) + 2 * al(12 * nb) + al(16)


@pytest.mark.parametrize("kind,n", [("mixed", 5000), ("stretches", 1100001)])
def test_synthetic_states_have_their_layout_and_margins(kind, n):
    """The generator's rows land in their categories under max_screen_size None and 20, no input is within the fixture's
    margins of a threshold, and the layouts hold what the GPU sweep relies on."""
    from oracle import densify_ref as dr
    cat = dr.layout(n, kind, seed=n)
    st = dr.synthetic_state(cat, seed=n)
    assert dr.check_margins(st, extent=1.0, **KW)
    want = {dr.KEEP: {"keep"}, dr.CLONE: {"keep", "clone_kept"}, dr.SPLIT: {"children_kept"}, dr.PRUNED: set(),
            dr.CHILD_PRUNED: set()}
    for size in (None, 20):
        c = dr.classify(st["scaling"], st["opacity"], st["xyz_gradient_accum"], st["denom"], extent=1.0,
                        max_screen_size=size, **KW)
        for k, fl in want.items():
            for f in ("keep", "clone_kept", "children_kept"):
                assert np.all(c[f][cat == k] == (f in fl)), (size, k, f)
        # pruned clones; split sources over the world size (pruned originals, kept children) only with a size
        assert c["clone"][cat == dr.PRUNED].any() and c["prune"][cat == dr.SPLIT].any() == bool(size)
    nb = (n + 1023) // 1024
    blocks = np.pad(cat, (0, nb * 1024 - n), constant_values=-1).reshape(nb, 1024)
    per_block = np.stack([(blocks == k).any(1) for k in range(5)], 1)
    if kind == "mixed":
        assert per_block.all()
    else:
        assert n % 1024 and nb > 4 * 256  # a partly filled last block, five scan rounds
        quiet = blocks[240:530]  # a whole scan round (blocks 256..511) with no clone and no kept child
        assert not np.isin(quiet, (dr.CLONE, dr.SPLIT)).any() and (quiet == dr.KEEP).any()
        dead = blocks[760:1040]  # a whole round (768..1023) with every row pruned
        assert np.isin(dead, (dr.PRUNED, dr.CHILD_PRUNED)).all()
        assert per_block[:240].all() and per_block[530:760].all() and per_block[1040:-1].all()


def test_alignment_helper_on_cpu_tensors():
    import torch
    from gsplat_mi355 import _lib
    img = torch.arange(3 * 5 * 7, dtype=torch.float32).reshape(3, 5, 7)
    assert _lib.is_aligned(img) and _lib.contiguous_aligned(img) is img
    view = img[1:]  # 35 floats in: 4 bytes past a 16-byte boundary
    assert view.is_contiguous() and not _lib.is_aligned(view) and _lib.is_aligned(view, 4)
    fixed = _lib.contiguous_aligned(view)
    assert _lib.is_aligned(fixed) and fixed.data_ptr() != view.data_ptr() and torch.equal(fixed, view)
    assert _lib.is_aligned(img.reshape(-1)[4:]) and not _lib.is_aligned(img.reshape(-1)[2:], 16)
    assert _lib.is_aligned(img[:0]) and _lib.is_aligned(img.reshape(-1)[1:1])
    strided = img[:, :, 1:]  # not contiguous: copied by .contiguous() into fresh storage
    assert _lib.is_aligned(_lib.contiguous_aligned(strided)) and torch.equal(_lib.contiguous_aligned(strided), strided)
