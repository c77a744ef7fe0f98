"""The converter's fused optimizer step on the GPU: the deterministic global gradient norm, the stand-alone
clip_grad_norm_, and FusedAdam with clipping, weight decay and device-resident step numbers, against the float64
restatement tests/optim_ref.py -- at tensor sizes that cross a chunk (2048) and a float4 tail, and tensor counts that
cross the by-value batches of the update (GS_ADAM_EX_BATCH) and of the norm (GS_GRAD_NORM_BATCH)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import optim_ref
from gsplat_mi355 import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SIZES = [1, 3, 1023, 1024, 1025, 4097]
COUNTS = [1, _lib.GS_ADAM_EX_BATCH, _lib.GS_ADAM_EX_BATCH + 1, 130, _lib.GS_GRAD_NORM_BATCH, _lib.GS_GRAD_NORM_BATCH + 1]
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0),
          dict(lr=5e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05)]
BAR = 2e-6  # of each tensor's maximum: the bar test_gpu_edges.py holds FusedAdam to


class Case(object):
    """`count` tensors cycling through SIZES; from three tensors on: tensor 1 is empty, tensor 2 has no gradient, and
    tensors 3 and 4 start at step 7 and 29 999 with moments in place.  Every third tensor is in the second group."""

    def __init__(self, count, seed=0, zero_wd=False):
        rs = np.random.default_rng(1000 * count + seed)
        self.rs = rs
        self.sizes = [SIZES[k % len(SIZES)] for k in range(count)]
        self.group_of = [1 if k % 3 == 2 else 0 for k in range(count)]
        self.no_grad = set()
        self.start = [0] * count
        if count >= 3:
            self.sizes[1] = 0
            self.no_grad.add(2)
        if count >= 5:
            self.start[3], self.start[4] = 7, 29999
        if count >= 12:
            self.start[11] = 29999   # one in the second group too
        self.groups = [dict(g, weight_decay=0.0) for g in GROUPS] if zero_wd else [dict(g) for g in GROUPS]
        self.init = [rs.normal(size=n).astype(np.float32) for n in self.sizes]
        self.pre = [(rs.normal(size=n).astype(np.float32) * 1e-2, rs.random(n).astype(np.float32) * 1e-4) if s else None
                    for n, s in zip(self.sizes, self.start)]
        self.hyper = [self.groups[g] for g in self.group_of]

    def grads(self):
        """Per tensor a magnitude over 1e-3 .. 10, with exact zeros; None where the tensor has no gradient."""
        out = []
        for k, n in enumerate(self.sizes):
            g = (self.rs.normal(size=n) * 10.0 ** self.rs.uniform(-3, 1)).astype(np.float32)
            g[4::5] = 0.0
            out.append(None if k in self.no_grad else g)
        return out

    def make(self, cls, dev=DEV, device_steps=False, lr_tensors=False, **kw):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in self.init]
        groups = []
        for gi, h in enumerate(self.groups):
            members = [p for p, g in zip(ps, self.group_of) if g == gi]
            if members:
                h = dict(h)
                if lr_tensors:
                    h["lr"] = torch.tensor(h["lr"], dtype=torch.float32, device=dev)
                groups.append(dict(params=members, **h))
        opt = cls(groups, lr=0.0, **kw)
        for p, s, st in zip(ps, self.start, self.pre):
            if s:
                opt.state[p] = {"step": torch.tensor(float(s), device=dev if device_steps else "cpu"),
                                "exp_avg": torch.from_numpy(st[0].copy()).to(dev), "exp_avg_sq": torch.from_numpy(st[1].copy()).to(dev)}
        return ps, opt

    def reference_state(self):
        P = [a.astype(np.float64) for a in self.init]
        M = [np.zeros(n) if st is None else st[0].astype(np.float64) for n, st in zip(self.sizes, self.pre)]
        V = [np.zeros(n) if st is None else st[1].astype(np.float64) for n, st in zip(self.sizes, self.pre)]
        return P, M, V


def _set_grads(ps, grads, dev=DEV):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state_bits_equal(ps_a, opt_a, ps_b, opt_b):
    for k, (pa, pb) in enumerate(zip(ps_a, ps_b)):
        assert _same_bits(pa, pb), k
        sa, sb = opt_a.state.get(pa, {}), opt_b.state.get(pb, {})
        assert set(sa.keys()) == set(sb.keys()), k
        for name in sa:
            if name == "step":
                assert float(sa[name]) == float(sb[name]), k
            else:
                assert _same_bits(sa[name], sb[name]), (k, name)


def _close(got, want, what):
    want = np.asarray(want, np.float64)
    if want.size == 0:
        return
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max()
    assert err <= BAR * max(np.abs(want).max(), 1e-30), (what, err, np.abs(want).max())


# ---- the norm and the stand-alone clip

@pytest.mark.parametrize("count", COUNTS)
def test_total_norm_matches_float64_and_repeats_bit_for_bit(count):
    """2e-6 relative: the sum of squares goes through at most 8 sequential adds per thread, the 6 + 2 levels of the
    workgroup tree and the same again over the partials -- under 30 roundings of 2^-24 on the sum, half of that on its
    root -- so the bound is a worst case, not what the kernel happens to give (observed: under 1e-7)."""
    from gsplat_mi355.optim import clip_grad_norm_
    case = Case(count)
    ps, _ = case.make(torch.optim.Adam)
    grads = case.grads()
    want = optim_ref.total_norm(grads)
    _set_grads(ps, grads)
    n1 = clip_grad_norm_(ps, 1e30)
    print("count %d: total_norm %.9g, float64 %.9g, rel %.3g" % (count, float(n1), want, abs(float(n1) - want) / want))
    assert n1.device == DEV and n1.dim() == 0 and n1.dtype == torch.float32
    assert abs(float(n1) - want) <= 2e-6 * want
    # a max_norm above the norm: the gradients keep their bits
    for p, g in zip(ps, grads):
        assert g is None and p.grad is None or np.array_equal(p.grad.cpu().numpy(), g)
    n2 = clip_grad_norm_(ps, 1e30)
    assert _same_bits(n1, n2)
    # ... and from fresh allocations at other addresses
    keep = [torch.empty(37, device=DEV) for _ in range(3)]
    _set_grads(ps, grads)
    assert _same_bits(n1, clip_grad_norm_(ps, 1e30)) and len(keep) == 3


@pytest.mark.parametrize("count", [1, 130, _lib.GS_GRAD_NORM_BATCH + 1])
def test_clip_grad_norm_scales_in_place_as_torch_does(count):
    from gsplat_mi355.optim import clip_grad_norm_
    case = Case(count, seed=1)
    ps, _ = case.make(torch.optim.Adam)
    grads = case.grads()
    norm = optim_ref.total_norm(grads)
    max_norm = 0.25 * norm
    want, _ = optim_ref.clip_grads(grads, max_norm)
    _set_grads(ps, grads)
    versions = [None if p.grad is None else p.grad._version for p in ps]
    got = clip_grad_norm_(ps, max_norm)
    assert abs(float(got) - norm) <= 2e-6 * norm
    for k, (p, w, v) in enumerate(zip(ps, want, versions)):
        if w is None:
            assert p.grad is None
            continue
        _close(p.grad, w, ("grad", k))
        assert p.grad._version > v  # the raw write is visible to autograd's version counter
    # an unaligned view is clipped through the scalar path, and a single tensor is accepted
    base = torch.from_numpy(case.rs.normal(size=1030).astype(np.float32)).to(DEV)
    t = torch.nn.Parameter(torch.zeros(1029, device=DEV))
    t.grad = base[1:]
    first = float(base[0])
    assert t.grad.data_ptr() % 16 != 0
    w, n = optim_ref.clip_grads([base[1:].cpu().numpy()], 0.5)
    got = clip_grad_norm_(t, 0.5)
    assert abs(float(got) - n) <= 2e-6 * n
    _close(t.grad, w[0], "unaligned")
    assert float(base[0]) == first   # the element in front of the view is not touched
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(ps, 1.0, norm_type=1)
    assert float(clip_grad_norm_(ps, 1e30, error_if_nonfinite=True)) > 0
    ps[0].grad[0] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


# ---- the fused step

@pytest.mark.parametrize("count", COUNTS)
def test_three_fused_steps_follow_the_restatement(count):
    """Clip (active: the norm is far above 0.1) + weight decay + Adam, three steps: parameters and both moments."""
    from gsplat_mi355.optim import FusedAdam
    case = Case(count, seed=2)
    ps, opt = case.make(FusedAdam, max_grad_norm=0.1)
    P, M, V = case.reference_state()
    steps = list(case.start)
    for t in range(3):
        grads = case.grads()
        _set_grads(ps, grads)
        opt.step()
        steps = [s + (g is not None) for s, g in zip(steps, grads)]
        P, M, V, norm = optim_ref.clip_adam_step(P, grads, M, V, case.hyper, steps, 0.1)
        assert count < 3 or norm > 0.1   # the clip is active
        assert abs(float(opt.total_norm) - norm) <= 2e-6 * norm
        assert opt.total_norm.device == DEV and opt.total_norm.dim() == 0
        for k, p in enumerate(ps):
            if grads[k] is None:
                assert p.grad is None and np.array_equal(p.detach().cpu().numpy(), case.init[k])
                assert p not in opt.state or float(opt.state[p]["step"]) == case.start[k]
                continue
            assert np.array_equal(p.grad.cpu().numpy(), grads[k]), k   # the fused step leaves the gradients unscaled
            st = opt.state[p]
            assert set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == steps[k], k
            _close(p, P[k], ("param", k, t))
            _close(st["exp_avg"], M[k], ("exp_avg", k, t))
            _close(st["exp_avg_sq"], V[k], ("exp_avg_sq", k, t))


@pytest.mark.parametrize("count", [_lib.GS_ADAM_EX_BATCH + 1, 130])
def test_without_clip_and_decay_the_fused_step_is_todays_fused_adam_bit_for_bit(count):
    from gsplat_mi355.optim import FusedAdam
    case = Case(count, seed=3, zero_wd=True)
    ps_a, a = case.make(FusedAdam)                        # the gs_adam_step path
    ps_b, b = case.make(FusedAdam, max_grad_norm=1e30)    # gs_grad_norm + gs_adam_step_ex, coefficient 1
    for _ in range(3):
        grads = case.grads()
        _set_grads(ps_a, grads)
        _set_grads(ps_b, grads)
        a.step()
        b.step()
        assert float(b._clip_out[1]) == 1.0
        _state_bits_equal(ps_a, a, ps_b, b)


@pytest.mark.parametrize("count", [_lib.GS_ADAM_EX_BATCH + 1, 130])
def test_capturable_is_the_eager_path_bit_for_bit(count):
    from gsplat_mi355.optim import FusedAdam
    case = Case(count, seed=4)
    ps_a, a = case.make(FusedAdam, max_grad_norm=0.1)
    ps_b, b = case.make(FusedAdam, max_grad_norm=0.1, capturable=True, device_steps=True, lr_tensors=True)
    for _ in range(3):
        grads = case.grads()
        _set_grads(ps_a, grads)
        _set_grads(ps_b, grads)
        a.step()
        b.step()
        _state_bits_equal(ps_a, a, ps_b, b)
    for k, p in enumerate(ps_b):
        if p in b.state:
            s = b.state[p]["step"]
            assert s.device == DEV and s.dtype == torch.float32 and s.dim() == 0
            assert float(s) == case.start[k] + (0 if k in case.no_grad else 3)


def test_in_kernel_clip_agrees_with_clip_then_unclipped_step():
    from gsplat_mi355.optim import FusedAdam, clip_grad_norm_
    case = Case(130, seed=5)
    ps_a, a = case.make(FusedAdam, max_grad_norm=0.1)
    ps_b, b = case.make(FusedAdam)
    for _ in range(3):
        grads = case.grads()
        _set_grads(ps_a, grads)
        _set_grads(ps_b, grads)
        a.step()
        nb = clip_grad_norm_(ps_b, 0.1)
        b.step()
        assert _same_bits(a.total_norm, nb)
        for k, (pa, pb) in enumerate(zip(ps_a, ps_b)):
            if grads[k] is None or case.sizes[k] == 0:
                continue
            _close(pa, pb.detach().cpu().numpy(), ("param", k))
            _close(a.state[pa]["exp_avg"], b.state[pb]["exp_avg"].cpu().numpy(), ("exp_avg", k))
            _close(a.state[pa]["exp_avg_sq"], b.state[pb]["exp_avg_sq"].cpu().numpy(), ("exp_avg_sq", k))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradients_end_where_torchs_end(bad):
    from gsplat_mi355.optim import FusedAdam
    case = Case(7, seed=6)
    ps, opt = case.make(FusedAdam, max_grad_norm=0.1)
    ref, o_ref = case.make(torch.optim.Adam, dev="cpu")
    grads = case.grads()
    grads[5][1000] = bad
    _set_grads(ps, grads)
    _set_grads(ref, grads, "cpu")
    opt.step()
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 0.1)
    o_ref.step()
    n = opt.total_norm.cpu()
    assert bool(torch.isnan(n)) == bool(torch.isnan(n_ref)) and bool(torch.isinf(n)) == bool(torch.isinf(n_ref))
    for k, (p, r) in enumerate(zip(ps, ref)):
        got, want = p.detach().cpu().numpy(), r.detach().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), k


# ---- capture

def test_captured_step_replays_bit_identical_to_eager_steps():
    """torch.cuda.graph around opt.step() (capturable, clipping), replayed three times with fresh gradients copied into
    the static gradient tensors and the device lr scaled between replays, against three eager steps; inside the same
    capture a non-capturable FusedAdam and a host step number at the C entry point are refused with nothing enqueued."""
    from gsplat_mi355.optim import FusedAdam
    gamma = 0.97
    case = Case(130, seed=7)
    kw = dict(max_grad_norm=0.1, capturable=True, device_steps=True, lr_tensors=True)
    ps_a, a = case.make(FusedAdam, **kw)
    ps_b, b = case.make(FusedAdam, **kw)
    ps_c, c = case.make(FusedAdam, max_grad_norm=0.1)   # not capturable
    warm = case.grads()
    _set_grads(ps_a, warm)
    _set_grads(ps_b, warm)
    _set_grads(ps_c, warm)
    static = [p.grad for p in ps_a]
    cur = torch.cuda.current_stream(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(3):
            a.step()
    cur.wait_stream(side)
    for _ in range(3):
        b.step()
    torch.cuda.synchronize()
    _state_bits_equal(ps_a, a, ps_b, b)
    L = _lib.load()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="capturable=True"):
            c.step()
        p0 = ps_a[0]
        rec = (_lib.GsAdamTensorEx * 1)(_lib.GsAdamTensorEx(p0.data_ptr(), p0.grad.data_ptr(), a.state[p0]["exp_avg"].data_ptr(),
                                                            a.state[p0]["exp_avg_sq"].data_ptr(), p0.numel(), 1e-3, 0.0, None, None))
        rc = L.gs_adam_step_ex(1, rec, 0.9, 0.999, 1e-15, 5, None, _lib.stream_ptr(DEV))
        a.step()
    assert rc == _lib.GS_E_CAPTURE
    assert all(len(c.state.get(p, {})) == 0 or float(c.state[p]["step"]) == s for p, s in zip(ps_c, case.start))
    torch.cuda.synchronize()
    _state_bits_equal(ps_a, a, ps_b, b)   # capturing ran nothing
    for _ in range(3):
        grads = case.grads()
        for s, gr in zip(static, grads):
            if gr is not None:
                s.copy_(torch.from_numpy(gr))
        _set_grads(ps_b, grads)
        g.replay()
        b.step()
        for opt in (a, b):
            for group in opt.param_groups:
                group["lr"].mul_(gamma)
        torch.cuda.synchronize()
        assert _same_bits(a.total_norm, b.total_norm)
        _state_bits_equal(ps_a, a, ps_b, b)
    for k, p in enumerate(ps_a):
        if p in a.state:
            assert float(a.state[p]["step"]) == case.start[k] + (0 if k in case.no_grad else 6)


# ---- the Python surface

def test_state_dicts_travel_between_fused_adam_and_torch_adam():
    from gsplat_mi355.optim import FusedAdam
    case = Case(9, seed=8)
    ps_f, f = case.make(FusedAdam)
    ps_t, t = case.make(torch.optim.Adam)
    for _ in range(2):
        grads = case.grads()
        _set_grads(ps_f, grads)
        _set_grads(ps_t, grads)
        f.step()
        t.step()
    # (deep copies, as a save / load makes them: state_dict() hands out the live state tensors)
    sd_f, sd_t = copy.deepcopy(f.state_dict()), copy.deepcopy(t.state_dict())
    assert set(sd_f.keys()) == set(sd_t.keys()) == {"state", "param_groups"}
    assert set(sd_f["state"].keys()) == set(sd_t["state"].keys())
    for idx in sd_f["state"]:
        assert set(sd_f["state"][idx].keys()) == set(sd_t["state"][idx].keys()) == {"step", "exp_avg", "exp_avg_sq"}
        for name in ("step", "exp_avg", "exp_avg_sq"):
            x, y = sd_f["state"][idx][name], sd_t["state"][idx][name]
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, (idx, name)
    for gf, gt in zip(sd_f["param_groups"], sd_t["param_groups"]):
        assert gf["params"] == gt["params"] and set(gf.keys()) <= set(gt.keys())
    # each loads the other's and goes on from it
    ps_f2, f2 = case.make(FusedAdam)
    ps_t2, t2 = case.make(torch.optim.Adam)
    f2.load_state_dict(sd_t)
    t2.load_state_dict(sd_f)
    with torch.no_grad():
        for dst, src in zip(ps_f2 + ps_t2, ps_t + ps_f):
            dst.copy_(src)
    grads = case.grads()
    for group in (ps_f, ps_t, ps_f2, ps_t2):
        _set_grads(group, grads)
    for opt in (f, t, f2, t2):
        opt.step()
    for k in range(len(ps_f)):
        if grads[k] is None or case.sizes[k] == 0:
            continue
        _close(ps_f2[k], ps_t[k].detach().cpu().numpy(), ("FusedAdam going on from torch's state", k))
        _close(ps_t2[k], ps_f[k].detach().cpu().numpy(), ("torch going on from FusedAdam's state", k))
        assert float(f2.state[ps_f2[k]]["step"]) == float(t2.state[ps_t2[k]]["step"]) == case.start[k] + 3


class _Opt(dict):
    pass


class _Cfg(object):
    def __init__(self, grad_clip):
        self.opt = _Opt(grad_clip=grad_clip)


class _Converter(torch.nn.Module):
    """What converter_optimize touches of GaussianConverter: cfg.opt.grad_clip, parameters(), optimizer, scheduler."""

    def __init__(self, cls, dev, grad_clip=0.1):
        super().__init__()
        rs = np.random.default_rng(9)
        self.cfg = _Cfg(grad_clip)
        self.mlp = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(rs.normal(size=s).astype(np.float32)).to(dev))
                                           for s in ((64, 33), (64,), (3, 64), (3,))])
        self.latent = torch.nn.Parameter(torch.from_numpy(rs.normal(size=(17, 16)).astype(np.float32)).to(dev))
        self.optimizer = cls([dict(params=list(self.mlp), lr=1e-3), dict(params=[self.latent], lr=5e-3, weight_decay=0.05)],
                             lr=1e-3, eps=1e-15)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=0.9)


@pytest.mark.parametrize("grad_clip", [0.1, 0.0])
def test_converter_optimize_follows_the_reference_sequence(grad_clip):
    from gsplat_mi355.optim import FusedAdam, converter_optimize
    mine = _Converter(FusedAdam, DEV, grad_clip)
    other = _Converter(torch.optim.Adam, DEV, grad_clip)      # not a FusedAdam: the reference's sequence, on the GPU
    ref = _Converter(torch.optim.Adam, "cpu", grad_clip)
    rs = np.random.default_rng(10)
    for _ in range(3):
        for pm, po, pr in zip(mine.parameters(), other.parameters(), ref.parameters()):
            g = rs.normal(size=tuple(pr.shape)).astype(np.float32)
            pm.grad, po.grad, pr.grad = torch.from_numpy(g).to(DEV), torch.from_numpy(g).to(DEV), torch.from_numpy(g)
        converter_optimize(mine)
        converter_optimize(other)
        if grad_clip > 0:
            torch.nn.utils.clip_grad_norm_(ref.parameters(), grad_clip)
        ref.optimizer.step()
        ref.optimizer.zero_grad()
        ref.scheduler.step()
        for pm, po, pr in zip(mine.parameters(), other.parameters(), ref.parameters()):
            assert pm.grad is None and po.grad is None
            _close(pm, pr.detach().numpy(), "fused")
            _close(po, pr.detach().numpy(), "fallback")
    assert mine.scheduler.last_epoch == other.scheduler.last_epoch == ref.scheduler.last_epoch == 3
    assert [g["lr"] for g in mine.optimizer.param_groups] == [g["lr"] for g in ref.optimizer.param_groups]
    assert (mine.optimizer.total_norm is not None) == (grad_clip > 0)
