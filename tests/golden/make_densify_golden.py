"""Generates tests/golden/densify.npz by EXECUTING the reference's own densification methods (scene/gaussian_model.py:
replace_tensor_to_optimizer, _prune_optimizer, prune_points, cat_tensors_to_optimizer, densification_postfix,
densify_and_split, densify_and_clone, densify_and_prune, reset_opacity; build_rotation / inverse_sigmoid of
utils/general_utils.py) on the CPU, on a stub model that carries a real torch.optim.Adam(l, lr=0.0, eps=1e-15) over the
reference's six parameter groups.  Only these function definitions are taken from the files' syntax trees (make_golden.py's
helpers); they allocate on "cuda", which the `torch` name in their scope maps to the CPU.  `torch.normal` in that scope
returns mean + std * z and keeps z, so the split children's noise is pinned.  Nothing of the reference's text is stored.

Sequence (SH degree 3, N = 1000 at the start; the config's thresholds 0.0002 / 0.01 / 0.05):
  Adam steps -> seeded statistics (some denom = 0, large max_radii2D) -> densify_and_prune(max_screen_size=None) [d1] ->
  Adam steps -> statistics -> densify_and_prune(20) [d2] -> reset_opacity [r] -> 40 Adam steps whose opacity gradients
  lift some Gaussians back over the threshold -> statistics -> densify_and_prune(20), most Gaussians pruned [d3].
Stored per densify phase p: the input state `in_<p>/...` that decides the cycle and positions the children (xyz,
opacity, scaling, rotation, the three statistics, every group's Adam `step`), the arguments, the split sources' z
(`<p>/z`, [n_split, 2, 3]), the selection masks (clone, split over the N sources; prune over the concatenated set), and
the result as its row map (`<p>/src`, `<p>/slot`: 0 original, 1 clone, 2 / 3 first / second child) with the children's
new xyz and scaling -- every other value of the result IS the input row its map names (or zero for a new row's moments
and for the statistics), which this script asserts against the reference's own output before storing.  For the reset:
the new opacity.
The values that only travel with the rows -- f_dc, f_rest and all twelve Adam moments -- are not stored: right before
each phase they are set to `passengers(p, N)` below (integer hashing, exact in fp32), which the GPU test forms again;
that keeps the file small (f_rest and its moments are 135 of the 177 floats of a row).  The Adam steps' gradients are
`step_grads` below, formed the same way.

Inputs within a relative margin of any threshold (scale 1e-5, opacity 1e-6) are rejected (asserted, with the extent or
the seed of the preceding steps changed until none is), so that a one-ulp difference between CPU exp / sigmoid and the
device's expf cannot flip a decision.

Run:  python tests/golden/make_densify_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
GRAD_THRESHOLD, PERCENT_DENSE, MIN_OPACITY = 0.0002, 0.01, 0.05
SCALE_MARGIN, OPACITY_MARGIN = 1e-5, 1e-6
SH_REST = 15  # SH degree 3


def _hash(n, key):
    """n uniform values in [-0.5, 0.5), exact multiples of 2^-24, from an integer hash of (index, key)."""
    with np.errstate(over="ignore"):
        h = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(key) * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(31)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(29)
    return ((h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)) - np.float32(0.5)


def step_grads(shapes, seed, t, lift=None):
    """Gradients of Adam step t (fp32 numpy, per group).  `lift`: per-row opacity bias in [-1, 1) multiplied in, which
    makes the opacity gradient's sign row-consistent across steps (the prune-heavy phase)."""
    out = {}
    for k, name in enumerate(GROUPS):
        n = int(np.prod(shapes[name]))
        g = _hash(n, seed * 100003 + t * 101 + k) * np.float32(2.0 ** -6)
        if name == "opacity" and lift is not None:
            g = g + lift.reshape(-1)
        out[name] = g.reshape(shapes[name])
    return out


def shapes(n):
    return {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, SH_REST, 3), "opacity": (n, 1), "scaling": (n, 3), "rotation": (n, 4)}


def passengers(tag, n):
    """The values a phase's rows carry without deciding anything: f_dc, f_rest ({name: array}) and every group's moments
    ("exp_avg.<name>", "exp_avg_sq.<name>"; exp_avg_sq >= 0).  Deterministic in (tag, n)."""
    key = 1000 * sum(ord(c) * 31 ** i for i, c in enumerate(tag))
    out = {}
    for j, (k, shp) in enumerate(shapes(n).items()):
        cnt = int(np.prod(shp))
        if k in ("f_dc", "f_rest"):
            out[k] = _hash(cnt, key + j).reshape(shp)
        out["exp_avg." + k] = (_hash(cnt, key + 10 + j) * np.float32(2.0 ** -10)).reshape(shp)
        out["exp_avg_sq." + k] = ((_hash(cnt, key + 20 + j) + np.float32(0.5)) * np.float32(2.0 ** -20)).reshape(shp)
    return out


def lift_bias(n, seed):
    return (_hash(n, seed * 7 + 5) * np.float32(2.0)).reshape(n, 1)  # [-1, 1): negative = opacity rises


def main():
    import make_golden as mg
    from torch import nn

    captured = {"z": [], "and": [], "prune": []}

    class _RecTorch(mg._CpuTorch):
        def normal(self, mean, std):
            z = torch.randn(std.shape, generator=self.gen)
            captured["z"].append(z)
            return mean + std * z

        def logical_and(self, *a, **kw):
            r = torch.logical_and(*a, **kw)
            captured["and"].append(r.clone())
            return r

    T = _RecTorch()
    T.gen = torch.Generator().manual_seed(4242)
    gu = mg._load_functions("utils/general_utils.py", ["build_rotation", "inverse_sigmoid"], dict(torch=T))
    scope = dict(torch=T, nn=nn, build_rotation=gu["build_rotation"], inverse_sigmoid=gu["inverse_sigmoid"])
    names = ["replace_tensor_to_optimizer", "_prune_optimizer", "prune_points", "cat_tensors_to_optimizer",
             "densification_postfix", "densify_and_split", "densify_and_clone", "densify_and_prune", "reset_opacity"]
    nodes, path = [], None
    for nm in names:
        node, path = mg._method("scene/gaussian_model.py", "GaussianModel", nm)
        nodes.append(node)
    ns = mg._exec_nodes(nodes, path, scope)

    class Model(object):
        get_xyz = property(lambda self: self._xyz)
        get_scaling = property(lambda self: torch.exp(self._scaling))
        get_opacity = property(lambda self: torch.sigmoid(self._opacity))
        scaling_inverse_activation = staticmethod(torch.log)

    for nm in names:
        setattr(Model, nm, ns[nm])
    orig_prune = ns["prune_points"]

    def prune_rec(self, mask):
        captured["prune"].append(mask.clone())
        return orig_prune(self, mask)
    Model.prune_points = prune_rec

    g = torch.Generator().manual_seed(2024)
    N0, K = 1000, SH_REST
    m = Model()
    m._xyz = nn.Parameter(torch.randn(N0, 3, generator=g))
    m._features_dc = nn.Parameter(torch.randn(N0, 1, 3, generator=g) * 0.5)
    m._features_rest = nn.Parameter(torch.randn(N0, K, 3, generator=g) * 0.1)
    m._opacity = nn.Parameter(torch.randn(N0, 1, generator=g) * 2.0 - 1.0)
    m._scaling = nn.Parameter(torch.randn(N0, 3, generator=g) * 1.2 - 4.5)
    m._rotation = nn.Parameter(torch.randn(N0, 4, generator=g))
    m.percent_dense = PERCENT_DENSE
    attrs = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
             "scaling": "_scaling", "rotation": "_rotation"}
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, attrs[k])], "lr": LRS[k], "name": k} for k in GROUPS],
                                   lr=0.0, eps=1e-15)
    out = {}

    def params():
        return {k: getattr(m, attrs[k]).detach().clone() for k in GROUPS}

    def state():
        s = {}
        for grp in m.optimizer.param_groups:
            st = m.optimizer.state[grp["params"][0]]
            s[grp["name"]] = (st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"]))
        return s

    def steps(seed, count, lift=None):
        for t in range(count):
            gr = step_grads({k: tuple(getattr(m, attrs[k]).shape) for k in GROUPS}, seed, t, lift)
            for k in GROUPS:
                getattr(m, attrs[k]).grad = torch.from_numpy(gr[k])
            m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)

    def seed_stats(seed):
        n = m._xyz.shape[0]
        rs = np.random.default_rng(seed)
        denom = rs.integers(0, 20, size=(n, 1)).astype(np.float32)
        gt = np.exp(rs.uniform(np.log(1e-5), np.log(1e-2), size=(n, 1))).astype(np.float32)
        accum = (gt * denom).astype(np.float32)
        z = denom[:, 0] == 0
        accum[z] = np.where(rs.random(int(z.sum())) < 0.5, 0.0, 1e-3).astype(np.float32)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            gg = accum / denom
        near = np.isfinite(gg) & (np.abs(gg.astype(np.float64) / GRAD_THRESHOLD - 1.0) < SCALE_MARGIN)
        accum[near] *= np.float32(1.01)
        m.xyz_gradient_accum = torch.from_numpy(accum)
        m.denom = torch.from_numpy(denom)
        m.max_radii2D = torch.from_numpy(rs.uniform(50, 2000, size=n).astype(np.float32))  # would prune if read

    def margins_ok(extent, size):
        s = m._scaling.detach().double()
        smax = torch.exp(s).max(1).values
        cmax = (torch.exp(s) / 1.6).max(1).values
        rel = lambda a, b: (a / b - 1.0).abs().min().item()
        ok = rel(smax, PERCENT_DENSE * extent) > SCALE_MARGIN
        if size:
            ok = ok and rel(smax, 0.1 * extent) > SCALE_MARGIN and rel(cmax, 0.1 * extent) > SCALE_MARGIN
        op = torch.sigmoid(m._opacity.detach().double())
        return ok and rel(op, MIN_OPACITY) > OPACITY_MARGIN

    def set_passengers(tag):
        pas = passengers(tag, m._xyz.shape[0])
        with torch.no_grad():
            for k in GROUPS:
                par = getattr(m, attrs[k])
                if k in pas:
                    par.copy_(torch.from_numpy(pas[k]))
                st = m.optimizer.state[par]
                st["exp_avg"].copy_(torch.from_numpy(pas["exp_avg." + k]))
                st["exp_avg_sq"].copy_(torch.from_numpy(pas["exp_avg_sq." + k]))

    def record_state(prefix):
        p, st = params(), state()
        for k in GROUPS:
            if k not in ("f_dc", "f_rest"):
                out[prefix + k] = p[k].numpy()
            out[prefix + "step." + k] = np.float32(st[k][2])
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            out[prefix + k] = getattr(m, k).numpy().copy()

    def densify(tag, size, extents):
        extent = next((e for e in extents if margins_ok(e, size)), None)
        assert extent is not None, "%s: every extent has an input within the threshold margins" % tag
        set_passengers(tag)
        record_state("in_%s/" % tag)
        before_p, before_s = params(), state()
        n = before_p["xyz"].shape[0]
        captured["z"].clear(), captured["and"].clear(), captured["prune"].clear()
        opt = mg._Stub(densify_grad_threshold=GRAD_THRESHOLD, opacity_threshold=MIN_OPACITY)
        m.densify_and_prune(opt, mg._Stub(cameras_extent=extent), size)
        clone = captured["and"][0].numpy()
        split_pad = captured["and"][1].numpy()
        assert not split_pad[n:].any()
        split = split_pad[:n]
        assert not (clone & split).any()
        prune = captured["prune"][-1].numpy()
        sel = np.nonzero(split)[0]
        src = np.concatenate([np.nonzero(~split)[0], np.nonzero(clone)[0], sel, sel]).astype(np.int32)
        slot = np.concatenate([np.zeros((~split).sum()), np.ones(clone.sum()), np.full(len(sel), 2), np.full(len(sel), 3)])
        assert len(prune) == len(src)
        src, slot = src[~prune], slot[~prune].astype(np.int8)
        after_p, after_s = params(), state()
        assert after_p["xyz"].shape[0] == len(src)
        new = slot != 0
        for k in GROUPS:
            a, b = after_p[k].numpy(), before_p[k].numpy()[src]
            if k in ("xyz", "scaling"):
                assert np.array_equal(a[slot < 2], b[slot < 2])
            else:
                assert np.array_equal(a, b), k
            for j in (0, 1):
                mom = after_s[k][j].numpy()
                assert np.array_equal(mom[~new], before_s[k][j].numpy()[src][~new]) and not mom[new].any()
            assert after_s[k][2] == before_s[k][2]
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            assert getattr(m, k).shape[0] == len(src) and not getattr(m, k).any()
        z = np.zeros((len(sel), 2, 3), np.float32)
        if len(sel):
            zz = captured["z"][0].numpy()
            z[:, 0], z[:, 1] = zz[:len(sel)], zz[len(sel):]
        child = slot >= 2
        out.update({"%s/src" % tag: src, "%s/slot" % tag: slot, "%s/clone" % tag: clone, "%s/split" % tag: split,
                    "%s/prune" % tag: prune, "%s/z" % tag: z, "%s/xyz" % tag: after_p["xyz"].numpy()[child],
                    "%s/scaling" % tag: after_p["scaling"].numpy()[child], "%s/extent" % tag: np.float64(extent),
                    "%s/max_screen_size" % tag: np.float64(size or 0)})
        print("%s: N %d -> %d (clone %d, split %d, pruned %d), extent %g" % (tag, n, len(src), clone.sum(), split.sum(),
                                                                             prune.sum(), extent))

    extents = [1.0, 0.97, 1.03, 0.93, 1.07, 0.9, 1.1]
    steps(1, 3)
    seed_stats(11)
    densify("d1", None, extents)
    seeds = iter(range(20, 40))
    for s in seeds:  # steps from the state after d1; out["steps_d2"] = the seed that left no input near a threshold
        snap = (params(), state())
        steps(s, 3)
        if margins_ok(1.0, 20) or s == 39:
            out["steps_d2/seed"] = np.int64(s)
            break
        _restore(m, attrs, snap)
    seed_stats(12)
    densify("d2", 20, extents)
    m.reset_opacity()
    out["r/opacity"] = m._opacity.detach().numpy().copy()
    for grp in m.optimizer.param_groups:
        if grp["name"] == "opacity":
            st = m.optimizer.state[grp["params"][0]]
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    n = m._xyz.shape[0]
    for s in range(40, 60):
        snap = (params(), state())
        steps(s, 40, lift=lift_bias(n, s))
        if margins_ok(1.0, 20):
            out["steps_d3/seed"] = np.int64(s)
            break
        _restore(m, attrs, snap)
    seed_stats(13)
    densify("d3", 20, extents)
    np.savez_compressed(os.path.join(HERE, "densify.npz"), **out)
    print("densify.npz: %.2f MB" % (os.path.getsize(os.path.join(HERE, "densify.npz")) / 1e6))


def _restore(m, attrs, snap):
    p, s = snap
    with torch.no_grad():
        for k in GROUPS:
            par = getattr(m, attrs[k])
            par.copy_(p[k])
            st = m.optimizer.state[par]
            st["exp_avg"].copy_(s[k][0])
            st["exp_avg_sq"].copy_(s[k][1])
            st["step"].fill_(s[k][2])


if __name__ == "__main__":
    main()
