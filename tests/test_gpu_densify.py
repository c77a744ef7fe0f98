"""The fused densification cycle (gsplat_mi355.densify, csrc/densify.hip) on the GPU against the reference's own
densify_and_prune / reset_opacity (tests/golden/densify.npz, executed on the CPU by make_densify_golden.py), with
FusedAdam and with torch.optim.Adam; edge cases; determinism; and a training loop across changes of N through the
unmodified render()."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_densify_golden as mdg  # noqa: E402

GROUPS = mdg.GROUPS
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))
    return {k: d[k] for k in d.files}


def _optimizer(kind, params, state=None):
    from gsplat_mi355.optim import FusedAdam
    cls = FusedAdam if kind == "fused" else torch.optim.Adam
    opt = cls([{"params": [params[k]], "lr": mdg.LRS[k], "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
    for k, st in (state or {}).items():
        opt.state[params[k]] = {"step": torch.tensor(float(st[2]), dtype=torch.float32), "exp_avg": st[0].clone(),
                                "exp_avg_sq": st[1].clone()}
    return opt


def _load_state(fx, tag):
    """A phase's input: the stored deciding tensors, the passengers (f_dc, f_rest, moments) formed as the generator formed
    them.  Returns (params, state, stats) on the GPU and the same values as numpy arrays."""
    prefix = "in_%s/" % tag
    pas = mdg.passengers(tag, fx[prefix + "xyz"].shape[0])
    host = {k: (pas[k] if k in pas else fx[prefix + k]) for k in GROUPS}
    for k in GROUPS:
        host["exp_avg." + k], host["exp_avg_sq." + k] = pas["exp_avg." + k], pas["exp_avg_sq." + k]
    params = {k: torch.nn.Parameter(torch.from_numpy(host[k]).to(DEV)) for k in GROUPS}
    state = {k: (torch.from_numpy(host["exp_avg." + k]).to(DEV), torch.from_numpy(host["exp_avg_sq." + k]).to(DEV),
                 float(fx[prefix + "step." + k])) for k in GROUPS}
    stats = {k: torch.from_numpy(fx[prefix + k]).to(DEV) for k in STATS}
    return params, state, stats, host


def _cat_prune(flags):
    """The final prune mask over the reference's concatenated set, from the plan's per-source flags."""
    from gsplat_mi355 import _lib
    f = flags.cpu().numpy().astype(np.int32)
    split = (f & _lib.GS_DENSIFY_F_SPLIT) != 0
    clone = (f & _lib.GS_DENSIFY_F_CLONE) != 0
    pr = (f & _lib.GS_DENSIFY_F_PRUNE) != 0
    cpr = (f & _lib.GS_DENSIFY_F_CHILD_PRUNE) != 0
    return np.concatenate([pr[~split], pr[clone], cpr[split], cpr[split]])


def _close(got, want, rel=1e-6):
    got, want = got.astype(np.float64), want.astype(np.float64)
    return np.all(np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want)))


def _densify_phase(fx, tag, kind):
    from gsplat_mi355 import densify
    params, state, stats, host = _load_state(fx, tag)
    opt = _optimizer(kind, params, state)
    old_steps = {k: opt.state[params[k]]["step"] for k in GROUPS}
    size = float(fx[tag + "/max_screen_size"]) or None
    kw = dict(grad_threshold=mdg.GRAD_THRESHOLD, percent_dense=mdg.PERCENT_DENSE, extent=float(fx[tag + "/extent"]),
              min_opacity=mdg.MIN_OPACITY, max_screen_size=size)
    plan = densify.plan_densify(params, stats, **kw)
    masks = plan.masks()
    assert np.array_equal(masks["clone"].cpu().numpy(), fx[tag + "/clone"]), tag
    assert np.array_equal(masks["split"].cpu().numpy(), fx[tag + "/split"]), tag
    assert np.array_equal(_cat_prune(plan.flags), fx[tag + "/prune"]), tag
    src, slot = fx[tag + "/src"], fx[tag + "/slot"]
    assert plan.n_new == len(src)
    noise = np.zeros((len(fx[tag + "/split"]), 2, 3), np.float32)
    noise[fx[tag + "/split"]] = fx[tag + "/z"]
    noise = torch.from_numpy(noise).to(DEV)
    new, new_stats = densify.apply_plan(plan, params, opt, stats, noise)
    torch.cuda.synchronize()
    old = slot < 2
    for k in GROUPS:
        got = new[k].detach().cpu().numpy()
        assert isinstance(new[k], torch.nn.Parameter) and new[k].requires_grad
        want = host[k][src]
        if k in ("xyz", "scaling"):
            assert np.array_equal(got[old], want[old]), (tag, k)
            assert _close(got[~old], fx["%s/%s" % (tag, k)]), (tag, k)
        else:
            assert np.array_equal(got, want), (tag, k)
        grp = [g for g in opt.param_groups if g["name"] == k][0]
        assert grp["params"][0] is new[k] and params[k] not in opt.state
        st = opt.state[new[k]]
        assert st["step"] is old_steps[k]
        for m in ("exp_avg", "exp_avg_sq"):
            got_m = st[m].cpu().numpy()
            want_m = host["%s.%s" % (m, k)][src]
            want_m[slot != 0] = 0.0  # clones and children start at zero
            assert np.array_equal(got_m, want_m), (tag, k, m)
    for k in STATS:
        assert new_stats[k].shape == (len(src),) + tuple(stats[k].shape[1:]) and not new_stats[k].any()
    return new, opt, new_stats


def _adam_steps(params, opt, seed, count, lift=None):
    for t in range(count):
        gr = mdg.step_grads({k: tuple(params[k].shape) for k in GROUPS}, seed, t, lift)
        for k in GROUPS:
            params[k].grad = torch.from_numpy(gr[k]).to(params[k].device)
        opt.step()
    opt.zero_grad(set_to_none=True)


def _adam_against_cpu(params, opt, seed, count, lift=None):
    """`count` steps of the optimizer the cycle handed its new parameters to, against torch.optim.Adam on the CPU from a
    copy of the same parameters and state: the Adam test's bar, 2e-6 of the tensor maximum; step numbers equal."""
    cpu = {k: torch.nn.Parameter(params[k].detach().cpu().clone()) for k in GROUPS}
    ref = torch.optim.Adam([{"params": [cpu[k]], "lr": mdg.LRS[k], "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
    for k in GROUPS:
        st = opt.state[params[k]]
        ref.state[cpu[k]] = {"step": st["step"].detach().cpu().clone(), "exp_avg": st["exp_avg"].cpu().clone(),
                             "exp_avg_sq": st["exp_avg_sq"].cpu().clone()}
    _adam_steps(params, opt, seed, count, lift)
    _adam_steps(cpu, ref, seed, count, lift)
    for k in GROUPS:
        want = cpu[k].detach().numpy().astype(np.float64)
        got = params[k].detach().cpu().numpy().astype(np.float64)
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max(), k
        st, rst = opt.state[params[k]], ref.state[cpu[k]]
        assert float(st["step"]) == float(rst["step"])
        for m in ("exp_avg", "exp_avg_sq"):
            w = rst[m].numpy().astype(np.float64)
            assert np.abs(st[m].cpu().numpy() - w).max() <= 2e-6 * max(np.abs(w).max(), 1e-30), (k, m)


@pytest.mark.parametrize("kind", ["fused", "torch"])
def test_fixture_replay(fx, kind):
    """d1 -> Adam steps -> d2 -> reset_opacity -> 40 Adam steps -> d3 (prune-heavy), each densify from the reference's
    own input state; the Adam stretches run on this library's own densify / reset results, against torch.optim.Adam on
    the CPU from the same state."""
    from gsplat_mi355 import densify
    new, opt, _ = _densify_phase(fx, "d1", kind)
    _adam_against_cpu(new, opt, int(fx["steps_d2/seed"]), 3)
    new, opt, _ = _densify_phase(fx, "d2", kind)
    steps = {k: opt.state[new[k]]["step"] for k in GROUPS}
    moments_before = {k: (opt.state[new[k]]["exp_avg"].clone(), opt.state[new[k]]["exp_avg_sq"].clone()) for k in GROUPS}
    after = densify.reset_opacity(new, opt)
    torch.cuda.synchronize()
    assert _close(after["opacity"].detach().cpu().numpy(), fx["r/opacity"])
    st = opt.state[after["opacity"]]
    assert new["opacity"] not in opt.state and st["step"] is steps["opacity"]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    for k in GROUPS:
        assert (after[k] is new[k]) == (k != "opacity")
        if k != "opacity":
            assert torch.equal(opt.state[after[k]]["exp_avg"], moments_before[k][0])
    n = after["xyz"].shape[0]
    s3 = int(fx["steps_d3/seed"])
    _adam_against_cpu(after, opt, s3, 40, lift=mdg.lift_bias(n, s3))
    _densify_phase(fx, "d3", kind)


def _random_state(n, seed, sh_rest=15, opacity=0.0, scale=-4.5, g=1e-3):
    rs = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rs.normal(size=s).astype(np.float32)).to(DEV)
    params = {"xyz": f(n, 3), "f_dc": f(n, 1, 3), "f_rest": f(n, sh_rest, 3), "opacity": f(n, 1) * 0.5 + opacity,
              "scaling": f(n, 3) * 0.3 + scale, "rotation": f(n, 4)}
    params = {k: torch.nn.Parameter(v) for k, v in params.items()}
    stats = {"xyz_gradient_accum": torch.full((n, 1), g, device=DEV) * (1.0 + f(n, 1).abs()),
             "denom": torch.ones(n, 1, device=DEV), "max_radii2D": torch.full((n,), 100.0, device=DEV)}
    return params, stats


def _with_state(params, kind, skip=()):
    opt = _optimizer(kind, params)
    for k in GROUPS:
        if k not in skip:
            opt.state[params[k]] = {"step": torch.tensor(7.0), "exp_avg": torch.randn_like(params[k]),
                                    "exp_avg_sq": torch.rand_like(params[k])}
    return opt


KW = dict(grad_threshold=0.0002, percent_dense=0.01, extent=1.0, min_opacity=0.05)


def test_edge_cases():
    from gsplat_mi355 import densify
    # nothing selected: gradients under the threshold, opacities high -> the same rows, the same moments
    params, stats = _random_state(3000, 1, opacity=4.0, g=1e-5)
    opt = _with_state(params, "fused")
    before = {k: (params[k].detach().clone(), opt.state[params[k]]["exp_avg"].clone()) for k in GROUPS}
    new, ns = densify.densify_and_prune(params, opt, stats, max_screen_size=20, **KW)
    for k in GROUPS:
        assert torch.equal(new[k].detach(), before[k][0]) and torch.equal(opt.state[new[k]]["exp_avg"], before[k][1])
    assert not ns["denom"].any() and ns["denom"].shape == (3000, 1)
    # everything split: large scales, large gradients -> 2 N children, zero moments, reduced scaling
    params, stats = _random_state(1000, 2, opacity=4.0, scale=-3.0, g=1.0)
    opt = _with_state(params, "torch")
    new, _ = densify.densify_and_prune(params, opt, stats, **KW)
    assert new["xyz"].shape == (2000, 3)
    assert not opt.state[new["f_rest"]]["exp_avg"].any()
    want = torch.log(torch.exp(params["scaling"].detach()) / 1.6)
    assert torch.allclose(new["scaling"].detach()[:1000], want, rtol=0, atol=1e-6)
    assert torch.equal(new["scaling"].detach()[:1000], new["scaling"].detach()[1000:])
    # everything pruned: N' = 0, empty tensors shaped as torch's, the state moved
    params, stats = _random_state(500, 3, opacity=-8.0)
    opt = _with_state(params, "fused")
    new, ns = densify.densify_and_prune(params, opt, stats, **KW)
    for k in GROUPS:
        assert new[k].shape == (0,) + tuple(params[k].shape[1:]) and opt.state[new[k]]["exp_avg"].shape == new[k].shape
    assert ns["max_radii2D"].shape == (0,) and ns["denom"].shape == (0, 1)
    # N = 1, cloned (small scale, large gradient)
    params, stats = _random_state(1, 4, opacity=4.0, scale=-7.0, g=1.0)
    opt = _with_state(params, "fused")
    m0 = opt.state[params["xyz"]]["exp_avg"].clone()
    new, _ = densify.densify_and_prune(params, opt, stats, **KW)
    assert new["xyz"].shape == (2, 3) and torch.equal(new["xyz"][0], new["xyz"][1])
    assert torch.equal(opt.state[new["xyz"]]["exp_avg"][0], m0[0]) and not opt.state[new["xyz"]]["exp_avg"][1].any()
    # a group without state gets none; prune_points alone keeps the surviving statistics
    params, stats = _random_state(2000, 5, opacity=4.0)
    opt = _with_state(params, "torch", skip=("rotation",))
    mask = torch.zeros(2000, dtype=torch.bool, device=DEV)
    mask[::3] = True
    stats["denom"].copy_(torch.arange(2000, device=DEV, dtype=torch.float32)[:, None])
    new, ns = densify.prune_points(params, opt, stats, mask)
    assert new["rotation"] not in opt.state and new["xyz"] in opt.state
    keep = ~mask
    for k in GROUPS:
        assert torch.equal(new[k].detach(), params[k].detach()[keep])
    assert torch.equal(ns["denom"], stats["denom"][keep])
    out = densify.reset_opacity(new, opt)
    assert (torch.sigmoid(out["opacity"]) <= 0.0100001).all()
    # a NaN gradient (0 / 0) is not selected; a positive accum over a zero denominator (inf) is
    params, stats = _random_state(4, 6, opacity=4.0, scale=-7.0, g=1.0)
    stats["denom"][:2] = 0.0
    stats["xyz_gradient_accum"][0] = 0.0
    plan = densify.plan_densify(params, stats, **KW)
    assert plan.masks()["clone"].tolist() == [False, True, True, True]


def test_determinism():
    from gsplat_mi355 import densify
    outs = []
    for _ in range(2):
        params, stats = _random_state(200000, 7, opacity=-2.5, scale=-4.6, g=0.7e-4)
        torch.manual_seed(0)
        opt = _with_state(params, "fused")
        noise = torch.randn(200000, 2, 3, device=DEV)
        new, _ = densify.densify_and_prune(params, opt, stats, max_screen_size=20, noise=noise, **KW)
        outs.append([new[k].detach().clone() for k in GROUPS] + [opt.state[new[k]]["exp_avg_sq"].clone() for k in GROUPS])
    n = outs[0][0].shape[0]
    assert 150000 < n < 250000 and n != 200000
    for a, b in zip(*outs):
        assert torch.equal(a, b)


class _Pc(object):
    def __init__(self, p, sh_degree):
        self.xyz = p["xyz"]
        self.opacity = torch.sigmoid(p["opacity"])
        self.scales = torch.exp(p["scaling"])
        self.rotations = torch.nn.functional.normalize(p["rotation"])
        self.shs = torch.cat((p["f_dc"], p["f_rest"]), dim=1)
        self.sh_degree = sh_degree


def test_training_across_changes_of_n(monkeypatch):
    """200 steps on 4k Gaussians at 128 x 128 with the reference's parametrisation, the two-call render(), FusedAdam and
    DensifyStats; densify at 50 (grows) and 100 (shrinks), reset_opacity at 150.  At every boundary the first frame equals,
    bit for bit, a render of cloned tensors with the wrapper's per-shape memory emptied."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355 import densify
    from gsplat_mi355.camera import orbit_camera
    from gsplat_mi355.optim import FusedAdam
    from gsplat_mi355.render import DensifyStats, Pipe, l1_loss, render
    from gsplat_mi355.scenes import GaussianCloud
    cloud, _ = helpers.cloud_and_camera(4000, 128, 128, sh_degree=1, seed=7)
    cam = orbit_camera(0, 128, 128, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        tc = GaussianCloud(*[getattr(cloud, f).to(DEV) for f in GaussianCloud.FIELDS], 1)
        pkg = render(cam, tc, Pipe(), bg, return_opacity=True)
        gt, gt_mask = pkg.render.clone(), pkg.opacity_render.clone()
    g = torch.Generator().manual_seed(0)
    shs = cloud.shs + 0.3 * torch.randn(cloud.shs.shape, generator=g)
    op = (cloud.opacity * 0.6).clamp(0.02, 0.98)
    raw = {"xyz": cloud.xyz, "f_dc": shs[:, :1], "f_rest": shs[:, 1:], "opacity": torch.log(op / (1 - op)).reshape(-1, 1),
           "scaling": torch.log(cloud.scales), "rotation": cloud.rotations}
    params = {k: torch.nn.Parameter(v.contiguous().to(DEV)) for k, v in raw.items()}
    lrs = dict(xyz=1e-4, f_dc=2e-2, f_rest=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3)
    opt = FusedAdam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
    st = DensifyStats(4000, DEV)
    pipe = Pipe()

    def frame(p):
        pkg = render(cam, _Pc(p, 1), pipe, bg, return_opacity=True)
        loss = l1_loss(pkg.render, gt) + 0.1 * l1_loss(pkg.opacity_render, gt_mask)
        loss.backward()
        return loss, pkg

    losses, sizes = [], []
    for it in range(200):
        if it in (50, 100, 150):
            n0 = params["xyz"].shape[0]
            if it == 150:
                params = densify.reset_opacity(params, opt)
            else:
                gg = (st.xyz_gradient_accum / st.denom).nan_to_num(0.0).reshape(-1)
                thr = float(torch.quantile(gg, 0.9 if it == 50 else 0.995))
                min_op = 0.01 if it == 50 else float(torch.quantile(torch.sigmoid(params["opacity"].detach()).reshape(-1), 0.3))
                ext = float(torch.exp(params["scaling"].detach()).max(1).values.median()) / 0.01
                s = {k: getattr(st, k) for k in STATS}
                params, s = densify.densify_and_prune(params, opt, s, grad_threshold=thr, percent_dense=0.01, extent=ext,
                                                      min_opacity=min_op, max_screen_size=20)
                for k in STATS:
                    setattr(st, k, s[k])
                n1 = params["xyz"].shape[0]
                assert (n1 > n0) if it == 50 else (n1 < n0), (it, n0, n1)
            sizes.append(params["xyz"].shape[0])
        opt.zero_grad(set_to_none=True)
        loss, pkg = frame(params)
        if it in (50, 100, 150):
            img, vgrad = pkg.render.detach().clone(), pkg.viewspace_points.grad.clone()
            # the same frame from cloned tensors, with nothing the wrapper remembers about earlier shapes
            dgr.release_shared_geometry()
            monkeypatch.setattr(dgr, "_last_count", {})
            clone = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
            _, pkg2 = frame(clone)
            torch.cuda.synchronize()
            assert torch.equal(img, pkg2.render.detach()), it
            assert torch.equal(vgrad, pkg2.viewspace_points.grad), it
        with torch.no_grad():
            st.update(pkg)
            opt.step()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(l) for l in losses)
    for k in GROUPS:
        assert torch.isfinite(params[k]).all()
    assert losses[149] < losses[0], losses[::10]
    assert losses[199] < losses[150], losses[150::10]
    assert len(set(sizes)) >= 2


# ---- sweep across block, scan-round and tail edges against the numpy restatement (oracle/densify_ref.py).  A block is
# 1024 sources, the scan carries its totals across rounds of 256 blocks: N = 262 145 is the first N with a carry, ~1.1 M
# has five rounds and a partly filled last block.  Compared through the row map and a gather on the device.

SWEEP_N = [1, 1023, 1024, 1025, 4097, 262143, 262144, 262145, 263169, 1100001]
SWEEP_KW = dict(grad_threshold=0.0002, percent_dense=0.01, extent=1.0, min_opacity=0.05)


def _sweep_state(n, kind="fused"):
    """A synthetic state of N rows (oracle/densify_ref.py: stretches layout where N has the rounds for it) on the device,
    with FusedAdam state on every group; f_dc, f_rest and the moments are device noise that only travels with the rows."""
    from oracle import densify_ref as dr
    host = dr.synthetic_state(dr.layout(n, "stretches" if n > 530 * 1024 else "mixed", seed=n), seed=n)
    assert dr.check_margins(host, **SWEEP_KW)
    gen = torch.Generator(device=DEV).manual_seed(n)
    rnd = lambda *s: torch.randn(s, device=DEV, generator=gen)
    params = {k: torch.nn.Parameter(torch.from_numpy(host[k]).to(DEV)) for k in ("xyz", "opacity", "scaling", "rotation")}
    params["f_dc"], params["f_rest"] = torch.nn.Parameter(rnd(n, 1, 3)), torch.nn.Parameter(rnd(n, 15, 3))
    opt = _optimizer(kind, params)
    for k in GROUPS:
        opt.state[params[k]] = {"step": torch.tensor(7.0), "exp_avg": rnd(*params[k].shape),
                                "exp_avg_sq": rnd(*params[k].shape).abs()}
    stats = {k: torch.from_numpy(host[k]).to(DEV) for k in STATS}
    return host, params, opt, stats


def _check_rows(new, opt, params, moments, src, slot, new_stats=None, stats=None):
    """Every copied value bit for bit through the map: parameters (children's xyz / scaling excepted), surviving moments,
    zeros for new rows' moments; statistics zero (densify) or gathered (prune_points)."""
    src_d, old_d = torch.from_numpy(src).to(DEV), torch.from_numpy(slot == 0).to(DEV)
    moved = torch.from_numpy(slot < 2).to(DEV)
    for k in GROUPS:
        got, want = new[k].detach(), params[k].detach()[src_d]
        assert got.shape == want.shape, k
        if k in ("xyz", "scaling"):
            assert torch.equal(got[moved], want[moved]), k
        else:
            assert torch.equal(got, want), k
        st = opt.state[new[k]]
        assert st["step"] is moments[k][2] and float(st["step"]) == 7.0
        for j, m in enumerate(("exp_avg", "exp_avg_sq")):
            w = moments[k][j][src_d]
            w[~old_d] = 0.0
            assert torch.equal(st[m], w), (k, m)
    for k in STATS:
        if stats is None:
            assert new_stats[k].shape == ((len(src),) if k == "max_radii2D" else (len(src), 1)), k
            assert not new_stats[k].any(), k
        else:
            assert torch.equal(new_stats[k], stats[k][src_d]), k


@pytest.mark.parametrize("size", [None, 20])
@pytest.mark.parametrize("n", SWEEP_N)
def test_densify_sweep_against_the_restatement(n, size):
    from gsplat_mi355 import densify
    from oracle import densify_ref as dr
    host, params, opt, stats = _sweep_state(n)
    want = dr.densify_and_prune(host["scaling"], host["opacity"], host["xyz_gradient_accum"], host["denom"],
                                max_screen_size=size, **SWEEP_KW)
    plan = densify.plan_densify(params, stats, max_screen_size=size, **SWEEP_KW)
    masks = {k: v.cpu().numpy() for k, v in plan.masks().items()}
    for k in ("clone", "split", "keep", "prune", "child_prune"):
        assert np.array_equal(masks[k], want[k]), (n, size, k)
    assert plan.n_new == want["n_new"]
    # the row map, before anything gathers by it
    src, slot = (t.cpu().numpy() for t in plan.row_map())
    assert np.array_equal(slot, want["slot"]), (n, size, "slot")
    assert np.array_equal(src, want["src"]), (n, size, "src")
    moments = {k: (opt.state[params[k]]["exp_avg"], opt.state[params[k]]["exp_avg_sq"], opt.state[params[k]]["step"])
               for k in GROUPS}
    noise = torch.randn((n, 2, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n + 1))
    new, new_stats = densify.apply_plan(plan, params, opt, stats, noise)
    torch.cuda.synchronize()
    _check_rows(new, opt, params, moments, src, slot, new_stats=new_stats)
    child = slot >= 2
    pos, scl = dr.children(host["xyz"], host["scaling"], host["rotation"], noise.cpu().numpy(), src, slot)
    ch = torch.from_numpy(child).to(DEV)
    assert _close(new["xyz"].detach()[ch].cpu().numpy(), pos) and _close(new["scaling"].detach()[ch].cpu().numpy(), scl)


def _prune_masks(n):
    masks = {"every third kept": np.arange(n) % 3 != 0, "last row": np.arange(n) == n - 1}
    if n > 257 * 1024:
        m = np.zeros(n, bool)
        m[1000:1000 + 257 * 1024 + 7] = True  # a run over more than a scan round
        masks["run of 257 blocks"] = m
    return masks


@pytest.mark.parametrize("n", SWEEP_N)
def test_prune_points_sweep_against_the_restatement(n):
    from gsplat_mi355 import densify
    from oracle import densify_ref as dr
    for name, mask in _prune_masks(n).items():
        _, params, opt, stats = _sweep_state(n)
        src, slot = dr.prune_points(mask)
        plan = densify.plan_prune(params, torch.from_numpy(mask).to(DEV))
        assert plan.n_new == len(src), name
        got_src, got_slot = (t.cpu().numpy() for t in plan.row_map())
        assert np.array_equal(got_slot, slot) and np.array_equal(got_src, src), (n, name)
        moments = {k: (opt.state[params[k]]["exp_avg"], opt.state[params[k]]["exp_avg_sq"], opt.state[params[k]]["step"])
                   for k in GROUPS}
        new, new_stats = densify.apply_plan(plan, params, opt, stats)
        torch.cuda.synchronize()
        _check_rows(new, opt, params, moments, src, slot, new_stats=new_stats, stats=stats)


@pytest.mark.parametrize("n", [1025, 1100001])
def test_reset_opacity_sweep_against_the_restatement(n):
    from gsplat_mi355 import densify
    from oracle import densify_ref as dr
    host, params, opt, _ = _sweep_state(n)
    steps = opt.state[params["opacity"]]["step"]
    out = densify.reset_opacity(params, opt)
    torch.cuda.synchronize()
    assert _close(out["opacity"].detach().cpu().numpy(), dr.reset_opacity(host["opacity"]))
    st = opt.state[out["opacity"]]
    assert st["step"] is steps and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert st["exp_avg"].shape == st["exp_avg_sq"].shape == (n, 1)
