"""The fused ColorMLP input (gsplat_mi355.texture -> csrc/texture.hip) on the GPU: parity with the reference's own fp32 and
fp64 results (tests/golden/texture.npz) and with the float64 restatement tests/texture_ref.py across block edges, odd
widths, the width limits, degree 4 and a degenerate direction; partial gradients, strides, bitwise determinism, no host
synchronisation, graph capture, and texture_forward end to end with a torch MLP against the same chain in plain fp64
torch.

Tolerance: the project's bar (BAR in test_gpu_skinning.py): no element beyond 1e-5 of its tensor's largest magnitude."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import texture_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
FX = ref.load_fixture(os.path.join(ROOT, "tests", "golden", "texture.npz"))
DEFAULT = dict(widths_before=(1, 31), widths_after=(16,), lt=16)  # the default config: D = 79 at degree 3
D_DEFAULT = 79


def _tx():
    from gsplat_mi355 import texture
    return texture


def _close(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.reshape(want.shape) - want).max()) / scale
    print("%s: %.3g of the largest magnitude" % (what, err))
    assert np.isfinite(got).all() and err <= BAR, "%s: %.3g of the largest magnitude" % (what, err)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _leaves(r, need=None):
    """Device leaves of a texture_ref.random_inputs dict: (before, after, xyz, latent) with requires_grad per `need`
    (None = all)."""
    def leaf(a, key):
        t = _dev(a)
        return t.requires_grad_(True) if (t is not None and (need is None or key in need)) else t
    before = [leaf(b, "before%d" % k) for k, b in enumerate(r["before"])]
    after = [leaf(b, "after%d" % k) for k, b in enumerate(r["after"])]
    return before, after, leaf(r["xyz"], "xyz"), leaf(r["latent"], "latent")


def _run(r, deg, g, need=None, fwd_transform="auto"):
    """(inp, {name: gradient or None}) of color_mlp_input on the inputs `r` for the upstream gradient g."""
    before, after, xyz, latent = _leaves(r, need)
    T = _dev(r["fwd_transform"]) if isinstance(fwd_transform, str) else fwd_transform
    inp = _tx().color_mlp_input(before, xyz, _dev(r["campos"]), deg, fwd_transform=T, view_noise=r["noise"], after=after, latent=latent)
    named = [("before%d" % k, b) for k, b in enumerate(before)] + [("after%d" % k, b) for k, b in enumerate(after)] + \
        [("xyz", xyz), ("latent", latent)]
    wanted = [(k, t) for k, t in named if t is not None and t.requires_grad]
    grads = {k: None for k, _ in named}
    if wanted:
        for (k, _), gr in zip(wanted, torch.autograd.grad((inp * _dev(g)).sum(), [t for _, t in wanted], allow_unused=True)):
            grads[k] = gr
    return inp, grads


def _restate(r, deg, g):
    kw = dict(before=r["before"], xyz=r["xyz"], campos=r["campos"], deg=deg, fwd_transform=r["fwd_transform"], noise=r["noise"],
              after=r["after"], latent=r["latent"])
    b = ref.compose_backward(g, **kw)
    want = {"before%d" % k: v for k, v in enumerate(b["before"])}
    want.update({"after%d" % k: v for k, v in enumerate(b["after"])})
    want.update(xyz=b["xyz"], latent=b["latent"])
    return ref.compose(**kw), want


def _check(r, deg, seed, what, **kw):
    D = sum(b.shape[1] for b in r["before"] + r["after"]) + ref.n_sh(deg) + (r["latent"].size if r["latent"] is not None else 0)
    g = np.random.default_rng(seed).normal(size=(r["xyz"].shape[0], D)).astype(np.float32)
    inp, grads = _run(r, deg, g, **kw)
    want_inp, want = _restate(r, deg, g)
    assert tuple(inp.shape) == want_inp.shape and inp.is_contiguous()
    _close(inp, want_inp, what + " inp")
    for k, w in want.items():
        if w is None or (k == "xyz" and deg == 0):
            assert grads[k] is None, k
        else:
            assert tuple(grads[k].shape) == np.shape(w), k
            _close(grads[k], w, "%s d%s" % (what, k))
    return inp, grads


# ---------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_fixture_parity(case):
    """Every case against the reference's fp32, its fp64 and the restatement."""
    c, p = ref.CASES[case], case + "/"
    leaf = lambda k: _dev(FX[p + k]).requires_grad_(True)
    dc, rest, xyz, feat, weight = leaf("features_dc"), leaf("features_rest"), leaf("xyz"), leaf("non_rigid_feature"), leaf("latent_weight")
    before = [dc, rest]
    if c["use_xyz"]:  # the reference's aabb.normalize(xyz, sym=True), in torch
        lo, hi = _dev(FX[p + "aabb"])
        before.append(2 * ((xyz - lo) / (hi - lo)) - 1.)
    row = int(FX[p + "latent_row"])
    inp = _tx().color_mlp_input(before, xyz, _dev(FX[p + "campos"]), c["sh_degree"],
                                fwd_transform=_dev(FX[p + "T_fwd"]) if c["cano"] else None,
                                view_noise=FX[p + "noise"] if (c["cano"] and c["train"]) else None, after=[feat],
                                latent=weight[row:row + 1] if c["latent_dim"] else None)
    grads = torch.autograd.grad((inp * _dev(FX[p + "g"])).sum(), [dc, rest, xyz, feat, weight], allow_unused=True)
    got = dict(zip(ref.GRADS, grads), inp=inp)
    for name, want in (("f32", lambda k: FX["%s%s_f32" % (p, k)]), ("f64", lambda k: FX["%s%s_f64" % (p, k)]),
                       ("restatement", ref.case_results(FX, case).__getitem__)):
        for k in ("inp",) + ref.GRADS:
            w = want(k)
            if not np.abs(w).max():
                assert got[k] is None or not got[k].any(), (case, k)
            else:
                _close(got[k], w, "%s %s vs %s" % (case, k, name))


def _large_n():
    """Rows for which the latent gradient's final sum has more than one term at every level: every thread of its
    FINAL_THREADS takes at least two block partials, so every wave ladder and the sum over the waves do too."""
    return _tx().rows_per_block(D_DEFAULT) * 2 * _tx().FINAL_THREADS + 1


def test_row_edges_and_block_counts():
    R = _tx().rows_per_block(D_DEFAULT)
    assert R == 100 and _large_n() == 51201
    for k, n in enumerate((1, R - 1, R, R + 1, 2 * R + 1, 4099, _large_n())):
        r = ref.random_inputs(n, seed=100 + k, dist=(0.3, 3.0)[k % 2], **DEFAULT)
        _check(r, 3, 200 + k, "N=%d" % n)


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_odd_widths(deg):
    """Widths that break every alignment assumption: D odd, block widths 1, 3 and 31, an odd latent width."""
    r = ref.random_inputs(257, (1, 3, 31), (3,), 7, seed=300 + deg, dist=0.3)
    D = 45 + ref.n_sh(deg)
    if D % 2 == 0:
        r["after"].append(np.random.default_rng(deg).normal(size=(257, 1)).astype(np.float32))
        D += 1
    assert D % 2 == 1 and _tx().rows_per_block(D) < 257
    _check(r, deg, 310 + deg, "odd widths deg %d" % deg)


def test_width_limits():
    tx = _tx()
    # six blocks in front and two behind, D = GS_TEXTURE_MAX_D, 128 latent columns (two runs per column and block)
    r = ref.random_inputs(2 * tx.rows_per_block(tx.MAX_D) + 1, (1, 2, 3, 5, 7, 100), (100, 142), 128, seed=320)
    inp, _ = _check(r, 4, 321, "D = cap")
    assert inp.shape[1] == tx.MAX_D == 512
    # a latent code wider than a workgroup
    r = ref.random_inputs(70, (10,), (), 499, seed=322, rot="3x3")
    inp, _ = _check(r, 1, 323, "wide latent")
    assert inp.shape[1] == tx.MAX_D
    r = ref.random_inputs(8, (10,), (1,), 499, seed=324)
    before, after, xyz, latent = _leaves(r)
    with pytest.raises(ValueError, match="513"):
        tx.color_mlp_input(before, xyz, _dev(r["campos"]), 1, after=after, latent=latent)
    with pytest.raises(ValueError, match="at most 6"):
        tx.color_mlp_input(before * 7, xyz, _dev(r["campos"]), 1)
    with pytest.raises(ValueError, match="at most 2"):
        tx.color_mlp_input(before, xyz, _dev(r["campos"]), 1, after=after * 3)


def test_degree_4():
    for k, dist in enumerate((0.3, 3.0)):
        _check(ref.random_inputs(257, seed=330 + k, dist=dist, **DEFAULT), 4, 332 + k, "deg 4 dist %g" % dist)


def test_degenerate_direction():
    """A row whose point is the camera centre: d = 0, unit = 0; finite outputs, the restatement's gradients."""
    r = ref.random_inputs(130, seed=340, dist=0.3, **DEFAULT)
    r["xyz"][[7, 129]] = r["campos"]
    for deg in (1, 3, 4):
        inp, grads = _check(r, deg, 341 + deg, "d = 0, deg %d" % deg)
        assert torch.isfinite(inp).all() and torch.isfinite(grads["xyz"]).all()
        # the two rows' gradients are ~1e12 and set the scale above: the other rows on their own
        keep = np.ones(130, bool)
        keep[[7, 129]] = False
        g = np.random.default_rng(341 + deg).normal(size=(130, inp.shape[1])).astype(np.float32)
        _close(grads["xyz"][torch.from_numpy(keep).to(DEV)], _restate(r, deg, g)[1]["xyz"][keep], "the other rows' dxyz")
        assert not inp[7, 32:32 + min(ref.n_sh(deg), 15)].any()  # the bases of degrees 1..3 vanish at u = 0


def test_no_rows():
    r = ref.random_inputs(0, seed=350, **DEFAULT)
    inp, grads = _run(r, 3, np.zeros((0, D_DEFAULT), np.float32))
    assert tuple(inp.shape) == (0, D_DEFAULT)
    assert tuple(grads["xyz"].shape) == (0, 3) and tuple(grads["before1"].shape) == (0, 31)
    assert tuple(grads["latent"].shape) == (16,) and not grads["latent"].any()


# ---------------------------------------------------------------------------------------------
# what is asked for, strides, determinism, capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", [("before0",), ("before1",), ("after0",), ("xyz",), ("latent",), ("before1", "latent"), ()])
def test_partial_requires_grad(need):
    n = 333
    r = ref.random_inputs(n, seed=360, **DEFAULT)
    g = np.random.default_rng(361).normal(size=(n, D_DEFAULT)).astype(np.float32)
    inp, grads = _run(r, 3, g, need=need)
    want_inp, want = _restate(r, 3, g)
    _close(inp, want_inp, "inp")
    if not need:
        assert inp.grad_fn is None and not inp.requires_grad
    for k, gr in grads.items():
        if k in need:
            _close(gr, want[k], "d" + k)
        else:
            assert gr is None, k


def test_strides_give_the_same_bits():
    n = 301
    r = ref.random_inputs(n, seed=370, **DEFAULT)
    g = np.random.default_rng(371).normal(size=(n, D_DEFAULT)).astype(np.float32)
    base, base_grads = _run(r, 3, g)
    # a non-contiguous block, an unaligned one, (N, 4, 4) transforms inside a larger tensor, (N, 3, 3) ones
    before, after, xyz, latent = _leaves(r)
    wide = torch.zeros(n, 40, device=DEV)
    wide[:, 3:34] = before[1].detach()
    before[1] = wide[:, 3:34].requires_grad_(True)
    shifted = torch.zeros(n * 16 + 1, device=DEV)
    shifted[1:] = after[0].detach().reshape(-1)
    after[0] = shifted[1:].reshape(n, 16).requires_grad_(True)
    big = torch.zeros(n + 5, 6, 4, device=DEV)
    big[2:n + 2, 1:5] = _dev(r["fwd_transform"])
    T33 = _dev(r["fwd_transform"])[:, :3, :3]
    assert not before[1].is_contiguous() and after[0].data_ptr() % 16 != 0 and not T33.is_contiguous()
    for what, T in (("sliced 4x4", big[2:n + 2, 1:5]), ("3x3 view", T33), ("3x3", T33.contiguous()), ("transposed storage", T33.transpose(1, 2).contiguous().transpose(1, 2))):
        inp = _tx().color_mlp_input(before, xyz, _dev(r["campos"]), 3, fwd_transform=T, view_noise=r["noise"], after=after, latent=latent)
        grads = torch.autograd.grad((inp * _dev(g)).sum(), before + after + [xyz, latent])
        assert torch.equal(inp, base), what
        for got, k in zip(grads, ("before0", "before1", "after0", "xyz", "latent")):
            assert torch.equal(got, base_grads[k]), (what, k)
    # (1, Lt) and (Lt,) latents; a features pair as the Gaussian model stores it
    before, after, xyz, latent = _leaves(r)
    inp = _tx().color_mlp_input([before[0].detach().reshape(n, 1, 1), before[1].detach().reshape(n, 31, 1)], xyz, _dev(r["campos"]).reshape(1, 3), 3,
                                fwd_transform=_dev(r["fwd_transform"]), view_noise=torch.from_numpy(r["noise"]), after=after,
                                latent=latent.detach().reshape(1, 16))
    assert torch.equal(inp, base)


def test_bitwise_determinism():
    n = _large_n()
    r = ref.random_inputs(n, seed=380, dist=0.3, **DEFAULT)
    g = np.random.default_rng(381).normal(size=(n, D_DEFAULT)).astype(np.float32)
    first, first_grads = _run(r, 3, g)
    for _ in range(2):
        again, again_grads = _run(r, 3, g)
        assert torch.equal(first, again)
        for k, v in first_grads.items():
            assert torch.equal(v, again_grads[k]), k
    # the latent gradient is the column sum
    _close(first_grads["latent"], g[:, -16:].astype(np.float64).sum(0), "dlatent at N=%d" % n)


def _step_fn(n=5000, seed=390):
    r = ref.random_inputs(n, seed=seed, **DEFAULT)
    g = _dev(np.random.default_rng(seed + 1).normal(size=(n, D_DEFAULT)).astype(np.float32))
    campos, T, noise = _dev(r["campos"]), _dev(r["fwd_transform"]), torch.from_numpy(r["noise"])

    def fresh():
        before, after, xyz, latent = _leaves(r)
        return before + after + [xyz, latent]

    def step(leaves):
        inp = _tx().color_mlp_input(leaves[:2], leaves[3], campos, 3, fwd_transform=T, view_noise=noise, after=leaves[2:3], latent=leaves[4])
        return (inp,) + tuple(torch.autograd.grad((inp * g).sum(), leaves))

    return fresh, step


def test_no_host_sync():
    fresh, step = _step_fn()
    leaves = fresh()
    step(leaves)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(leaves)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)


def test_graph_capture_replays_bit_identical():
    """torch's whole-network recipe (as tests/test_gpu_pose.py): fresh leaves first used on the side stream, then
    captured on it."""
    fresh, step = _step_fn()
    eager = [t.detach().clone() for t in step(fresh())]
    leaves = fresh()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step(leaves)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step(leaves)
    for _ in range(2):
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


def test_dtype_and_device_errors():
    r = ref.random_inputs(9, seed=395, **DEFAULT)
    before, after, xyz, latent = _leaves(r)
    campos = _dev(r["campos"])
    with pytest.raises(RuntimeError, match="GPU"):
        _tx().color_mlp_input(before, xyz.detach().cpu(), campos, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        _tx().color_mlp_input(before, xyz, campos, 3, latent=latent.detach().cpu())
    with pytest.raises(TypeError):
        _tx().color_mlp_input(before, xyz, campos, 3, after=[after[0].detach().double()])
    with pytest.raises(ValueError):
        _tx().color_mlp_input(before, xyz, campos, 5)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
FRAMES = (3, 5, 8, 13)


class _Cfg(dict):
    pass


class _AABB(object):
    def __init__(self, lo, hi):
        self.coord_min, self.coord_max = lo, hi

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1. if sym else x


class _Texture(torch.nn.Module):
    """ColorMLP's attributes with a torch MLP of the default shape; `chain` is compose_input, the MLP and the sigmoid in
    plain torch operators, in the parameters' dtype."""

    def __init__(self, cfg, seed, use_xyz=False):
        super().__init__()
        nn = torch.nn
        self.cfg, self.use_xyz, self.use_cov, self.use_normal = _Cfg(cfg), use_xyz, False, False
        self.sh_degree, self.cano_view_dir = cfg.get("sh_degree", 3), cfg.get("cano_view_dir", True)
        self.non_rigid_dim, self.latent_dim = 16, 16
        self.metadata = {"aabb": _AABB(torch.tensor([-1.25, -1.5, -1.125]), torch.tensor([1.5, 1.25, 1.75]))}
        self.frame_dict = {f: k for k, f in enumerate(FRAMES)}
        self.latent = nn.Embedding(len(FRAMES), 16)
        d_in = 32 + 3 * use_xyz + ref.n_sh(self.sh_degree) + 32
        self.mlp = nn.Sequential(nn.Linear(d_in, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 3))
        self.color_activation = nn.Sigmoid()
        rng = np.random.default_rng(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.from_numpy(rng.uniform(-1, 1, size=tuple(p.shape)) / np.sqrt(p.shape[-1])))

    def chain(self, gaussians, camera, noise, pre=None):
        feats = [torch.cat((gaussians._features_dc, gaussians._features_rest), dim=1).squeeze(-1)]
        xyz = gaussians.get_xyz
        if self.use_xyz:
            aabb = self.metadata["aabb"]
            feats.append(_AABB(aabb.coord_min.to(xyz), aabb.coord_max.to(xyz)).normalize(xyz, sym=True))
        if self.sh_degree > 0:
            d = xyz - camera.camera_center.reshape(1, 3)
            if self.cano_view_dir:
                d = torch.matmul(gaussians.fwd_transform[:, :3, :3].transpose(1, 2), d.unsqueeze(-1)).squeeze(-1)
                if noise is not None:
                    d = torch.matmul(d, noise.to(d))
            u = d / (d.norm(dim=1, keepdim=True) + 1e-12)
            x, y, z = u.unbind(-1)
            feats.append(torch.stack([sum(c * x ** e[0] * y ** e[1] * z ** e[2] for c, e in terms)
                                      for terms in ref.BASES[:ref.n_sh(self.sh_degree)]], dim=1))
        feats.append(gaussians.non_rigid_feature)
        row = self.frame_dict.get(camera.frame_id, len(self.frame_dict) - 1)
        feats.append(self.latent.weight[row:row + 1].expand(xyz.shape[0], -1))
        h = torch.cat(feats, dim=1)
        for layer in self.mlp:
            h = layer(h)
            if pre is not None and isinstance(layer, torch.nn.Linear):
                pre.append(h.detach())
        return self.color_activation(h)


class _Gaussians(torch.nn.Module):
    def __init__(self, r):
        super().__init__()
        P = lambda a: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a)))
        n = r["xyz"].shape[0]
        self._features_dc, self._features_rest = P(r["before"][0].reshape(n, 1, 1)), P(r["before"][1].reshape(n, 31, 1))
        self._xyz, self.non_rigid_feature = P(r["xyz"]), P(r["after"][0])
        self.register_buffer("fwd_transform", torch.from_numpy(r["fwd_transform"]))

    @property
    def get_xyz(self):
        return self._xyz


def _clear_inputs(cfg, use_xyz, frame, noise, n=130, seed=400):
    """The first seed whose fp64 chain keeps every LeakyReLU pre-activation 1e-5 away from its kink, so that the fp32 run
    (whose GEMMs err by ~1e-6 of such values) decides every unit the same way."""
    while True:
        r = ref.random_inputs(n, seed=seed, dist=3.0, **DEFAULT)
        module, gs = _Texture(cfg, seed, use_xyz).double(), _Gaussians(r).double()
        camera = types.SimpleNamespace(camera_center=torch.from_numpy(r["campos"]).double(), frame_id=frame)
        pre = []
        module.chain(gs, camera, None if noise is None else torch.from_numpy(noise).double(), pre)
        if min(float(p.abs().min()) for p in pre[:2]) > 1e-5:
            return r, seed
        seed += 1000


@pytest.mark.parametrize("mode", ["train_noise", "eval", "world", "use_xyz", "augm_rots"])
def test_texture_forward_end_to_end(mode, monkeypatch):
    """texture_forward as ColorMLP.forward on a stub module: colours and the gradients of every parameter and leaf
    against the same chain in fp64 torch."""
    cfg = dict(sh_degree=3, cano_view_dir=mode != "world", view_noise=45.0)
    training, frame = mode != "eval", (8 if mode != "eval" else 77)  # (77: a frame the module does not know)
    noise = ref.random_inputs(1, (1,), (), 0, seed=410)["noise"] if mode in ("train_noise", "use_xyz", "augm_rots") else None
    r, seed = _clear_inputs(cfg, mode == "use_xyz", frame, noise)
    g = np.random.default_rng(seed + 1).normal(size=(r["xyz"].shape[0], 3))
    results = []
    for dtype, dev in ((torch.float64, torch.device("cpu")), (torch.float32, DEV)):
        module, gs = _Texture(cfg, seed, mode == "use_xyz").to(dtype).to(dev), _Gaussians(r).to(dtype).to(dev)
        aabb = module.metadata["aabb"]  # (plain attributes: moved by hand)
        module.metadata = {"aabb": _AABB(aabb.coord_min.to(dtype).to(dev), aabb.coord_max.to(dtype).to(dev))}
        module.train(training)
        camera = types.SimpleNamespace(camera_center=torch.from_numpy(r["campos"]).to(dtype).to(dev), frame_id=frame)
        if dtype == torch.float64:
            colors = module.chain(gs, camera, None if noise is None else torch.from_numpy(noise))
        elif mode == "augm_rots":  # the lazy import of the reference's own generator: the matrix comes back untransposed
            calls = []
            stub = types.ModuleType("utils.sh_utils")
            stub.augm_rots = lambda *a: calls.append(a) or noise.astype(np.float64).T
            pkg = types.ModuleType("utils")
            pkg.sh_utils = stub
            monkeypatch.setitem(sys.modules, "utils", pkg)
            monkeypatch.setitem(sys.modules, "utils.sh_utils", stub)
            colors = _tx().texture_forward(module, gs, camera)
            assert calls == [(45.0, 45.0, 45.0)]
        else:
            # (an explicit matrix outside training, or without cano_view_dir, is not applied: as the reference)
            given = noise if noise is not None else ref.random_inputs(1, (1,), (), 0, seed=411)["noise"]
            colors = _tx().texture_forward(module, gs, camera, view_noise=torch.from_numpy(given))
        params = list(module.parameters()) + list(gs.parameters())
        grads = torch.autograd.grad((colors * torch.from_numpy(g).to(dtype).to(dev)).sum(), params)
        results.append([colors] + list(grads))
    names = ["colours"] + [n for n, _ in module.named_parameters()] + [n for n, _ in gs.named_parameters()]
    assert "latent.weight" in names and "_features_dc" in names and "_xyz" in names
    for name, want, got in zip(names, *results):
        _close(got, want.detach().numpy(), "%s %s" % (mode, name))
    row = module.frame_dict.get(frame, len(FRAMES) - 1)
    dW = results[1][1 + names[1:].index("latent.weight")]
    assert dW[row].any() and not dW[[k for k in range(len(FRAMES)) if k != row]].any()
    assert "_gsplat_latent_rows" in module.__dict__ and module.__dict__["_gsplat_latent_rows"].device.type == "cuda"


def test_texture_forward_use_flags_column_order(monkeypatch):
    """use_xyz, use_cov and use_normal: their blocks, computed in torch by the reference's own operations (build_rotation
    comes from the reference's utils.general_utils: a stand-in here), sit in front of the bases in the reference's order."""
    n = 37
    r = ref.random_inputs(n, seed=420, **DEFAULT)
    rng = np.random.default_rng(421)
    module, gs = _Texture(dict(sh_degree=3, cano_view_dir=True), 420, use_xyz=True).to(DEV), _Gaussians(r).to(DEV)
    aabb = module.metadata["aabb"]
    module.metadata = {"aabb": _AABB(aabb.coord_min.to(DEV), aabb.coord_max.to(DEV))}
    module.use_cov = module.use_normal = True
    module.eval()
    cov, quat, scaling = _dev(rng.normal(size=(n, 6)).astype(np.float32)), _dev(rng.normal(size=(n, 4)).astype(np.float32)), \
        _dev(rng.normal(size=(n, 3)).astype(np.float32))
    gs.get_covariance = lambda: cov
    gs._rotation, gs._scaling = quat, scaling

    def build_rotation(q):
        q = q / q.norm(dim=1, keepdim=True)
        w, x, y, z = q.unbind(1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                            1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                            1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)

    stub = types.ModuleType("utils.general_utils")
    stub.build_rotation = build_rotation
    pkg = types.ModuleType("utils")
    pkg.general_utils = stub
    monkeypatch.setitem(sys.modules, "utils", pkg)
    monkeypatch.setitem(sys.modules, "utils.general_utils", stub)
    seen = []

    class Tap(torch.nn.Module):  # keeps the composed input, hands three of its columns on
        def forward(self, x):
            seen.append(x)
            return x[:, :3]

    module.mlp = Tap()
    camera = types.SimpleNamespace(camera_center=_dev(r["campos"]), frame_id=5)
    colors = _tx().texture_forward(module, gs, camera)
    inp = seen[0]
    assert tuple(inp.shape) == (n, 32 + 3 + 6 + 3 + 15 + 16 + 16) and tuple(colors.shape) == (n, 3)
    xyz = gs.get_xyz.detach()
    normal = torch.gather(build_rotation(quat), dim=2, index=scaling.argmin(1).reshape(-1, 1, 1).expand(-1, 3, 1)).squeeze(-1)
    assert torch.equal(inp[:, 32:35], module.metadata["aabb"].normalize(xyz, sym=True))
    assert torch.equal(inp[:, 35:41], cov) and torch.equal(inp[:, 41:44], normal)
    want = ref.compose([r["before"][0], r["before"][1]], r["xyz"], r["campos"], 3, fwd_transform=r["fwd_transform"],
                       after=r["after"], latent=module.latent.weight[1].detach().cpu().numpy())
    _close(torch.cat([inp[:, :32], inp[:, 44:]], dim=1), want, "the other columns")
