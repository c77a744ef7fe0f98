"""The fused non-rigid deformer (gsplat_mi355.nonrigid -> csrc/nonrigid.hip) on the GPU: parity of the pose encoder and of
the delta application with the reference's own fp32 and fp64 results (tests/golden/nonrigid.npz) and with the float64
restatement tests/nonrigid_ref.py across block edges, row widths, all mode pairs and the kinks (dead ReLUs, zero-length
bones, zero offset rows, the clamp of `exp`); partial gradients, strides, row independence, bitwise determinism, no host
synchronisation, graph capture, and nonrigid_forward end to end with the project's hash grid and a torch MLP against the
same chain in plain fp64 torch.

Tolerance: the project's bar (BAR in test_gpu_skinning.py): no element beyond 1e-5 of its tensor's largest magnitude; the
hash grid's end-to-end test grants its gradients the same figure."""
import os

import numpy as np
import pytest
import torch

import hashgrid_ref
import nonrigid_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5
FX = ref.load_fixture(os.path.join(ROOT, "tests", "golden", "nonrigid.npz"))
PAIRS = [(s, r) for s in ref.SCALE_OFFSETS for r in ref.ROT_OFFSETS]
HASH_CFG = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 16, "base_resolution": 16,
            "per_level_scale": float(np.exp(np.log(2048 / 16) / 15)), "max_resolution": 2048}  # the reference's config


def _nr():
    from gsplat_mi355 import nonrigid
    return nonrigid


def _close(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.reshape(want.shape) - want).max()) / scale
    print("%s: %.3g of the largest magnitude" % (what, err))
    assert np.isfinite(got).all() and err <= BAR, "%s: %.3g of the largest magnitude" % (what, err)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------
# the pose encoder
# ---------------------------------------------------------------------------------------------
def _module(d, packed=None, **kw):
    m = ref.PoseEncoder(dim_per_joint=d, **kw)
    if packed is not None:
        with torch.no_grad():
            for p, v in zip(m.encoder_parameters(), ref.unpack(np.asarray(packed), d)):
                p.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return m.to(DEV)


def _restated(module, rots, Jtrs, g):
    """The float64 restatement's results for a module's encoder parameters; the inputs must keep every ReLU pre-activation
    further than 1e-4 from 0, where fp32 and fp64 cannot decide differently (as the fixture's generator asserts)."""
    d = module.layer_0.out_features
    packed = ref.pack([p.detach().cpu().numpy() for p in module.encoder_parameters()])
    want = ref.encoder_forward_backward(packed, d, rots, Jtrs, module.ktree_parents, g)
    assert np.abs(want["pre"]).min() > 1e-4, np.abs(want["pre"]).min()
    return want


def _run_enc(module, rots, Jtrs, g, need=(True, True)):
    """Fused forward and backward: (out, drots, dJtrs, [98 parameter gradients])."""
    module.zero_grad(set_to_none=True)
    r, J = _dev(rots).requires_grad_(need[0]), _dev(Jtrs).requires_grad_(need[1])
    out = _nr().pose_encode(module, r, J)
    (out * _dev(g)).sum().backward()
    return out.detach(), r.grad, J.grad, [p.grad for p in module.encoder_parameters()]


def _check_enc(got, want, d, what):
    out, dr, dJ, dp = got
    _close(out, want["out"], what + " out")
    if dr is not None:
        _close(dr, want["drots"], what + " drots")
    if dJ is not None:
        _close(dJ, want["dJtrs"], what + " dJtrs")
    for k, (g, w) in enumerate(zip(dp, ref.unpack(np.asarray(want["dparams"]), d))):
        if g is not None:
            _close(g, w, "%s parameter %d" % (what, k))


@pytest.mark.parametrize("case", ref.ENC_CASES)
def test_encoder_fixture_parity(case):
    p = case + "/"
    d = int(FX[p + "d"])
    got = _run_enc(_module(d, FX[p + "params"]), FX[p + "rots"], FX[p + "Jtrs"], FX[p + "g"])
    assert tuple(got[0].shape) == (1, 24 * d) and all(g is not None for g in got[3])
    for prec in ("f32", "f64"):
        _check_enc(got, {k: FX["%s%s_%s" % (p, k, prec)] for k in ("out", "drots", "dJtrs", "dparams")}, d, "%s vs %s" % (case, prec))
    want = ref.encoder_forward_backward(FX[p + "params"], d, FX[p + "rots"], FX[p + "Jtrs"], ref.SMPL_PARENTS, FX[p + "g"])
    _check_enc(got, want, d, case + " vs restatement")
    if case == "k":  # dead joints: exactly zero first-layer gradients
        for j in (5, 16):
            assert not got[3][2 + 4 * j].any() and not got[3][3 + 4 * j].any() and not got[3][4 + 4 * j].any()
    if case == "z":
        assert torch.isfinite(got[2]).all()


TREES = {"chain": np.arange(-1, 23), "star": np.zeros(24, np.int64)}


@pytest.mark.parametrize("tree", sorted(TREES))
@pytest.mark.parametrize("d", [3, 16])
def test_encoder_other_trees(tree, d):
    """A chain (24 levels of one joint) and a star (one level of 23): the result does not depend on how many joints share
    a level."""
    parents = TREES[tree]
    module = _module(d, parents=parents, seed=31 + d)
    rots, Jtrs = ref.random_pose(44)
    g = np.random.default_rng(5).normal(size=(1, 24 * d)).astype(np.float32)
    _check_enc(_run_enc(module, rots, Jtrs, g), _restated(module, rots, Jtrs, g), d, tree)


@pytest.fixture(scope="module")
def enc_small():
    d = 6
    module = _module(d, seed=3)
    rots, Jtrs = ref.random_pose(4)
    g = np.random.default_rng(6).normal(size=(1, 24 * d)).astype(np.float32)
    return module, rots, Jtrs, g, _restated(module, rots, Jtrs, g)


@pytest.mark.parametrize("need", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("frozen", [False, True])
def test_encoder_partial_requires_grad(enc_small, need, frozen):
    module, rots, Jtrs, g, want = enc_small
    if frozen and not any(need):
        out = _nr().pose_encode(module.requires_grad_(False), _dev(rots), _dev(Jtrs))
        module.requires_grad_(True)
        assert not out.requires_grad
        return
    module.requires_grad_(not frozen)
    try:
        got = _run_enc(module, rots, Jtrs, g, need=need)
    finally:
        module.requires_grad_(True)
    assert (got[1] is not None) == need[0] and (got[2] is not None) == need[1]
    assert all((p is None) == frozen for p in got[3])
    _check_enc(got, want, 6, "need %s frozen %s" % (need, frozen))


def test_encoder_single_parameter_alone(enc_small):
    module, rots, Jtrs, g, want = enc_small
    module.requires_grad_(False)
    try:
        for k in (0, 1, 2 + 4 * 9, 2 + 4 * 23 + 3):
            params = module.encoder_parameters()
            params[k].requires_grad_(True)
            got = _run_enc(module, rots, Jtrs, g, need=(False, False))
            params[k].requires_grad_(False)
            assert [i for i, p in enumerate(got[3]) if p is not None] == [k]
            _check_enc(got, want, 6, "parameter %d alone" % k)
    finally:
        module.requires_grad_(True)


@pytest.mark.parametrize("out_dim", [-1, 20])
def test_encoder_drop_in(out_dim):
    """hierarchical_pose_encoder_forward on a HierarchicalPoseEncoder-shaped module against the same module in fp64 torch:
    every parameter's .grad is set and equal; out_dim > 0 goes through its nn.Linear."""
    d = 6
    module = ref.PoseEncoder(dim_per_joint=d, out_dim=out_dim, seed=9).to(DEV)
    twin = ref.PoseEncoder(dim_per_joint=d, out_dim=out_dim, seed=9, dtype=torch.float64)
    rots, Jtrs = ref.random_pose(10)
    g = np.random.default_rng(11).normal(size=(1, module.n_output_dims)).astype(np.float32)
    _restated(module, rots, Jtrs, np.zeros((1, 24 * d), np.float32))  # (clear of the ReLU kinks)
    r, J = _dev(rots).requires_grad_(True), _dev(Jtrs).requires_grad_(True)
    out = _nr().hierarchical_pose_encoder_forward(module, r, J)
    assert tuple(out.shape) == (1, 20 if out_dim > 0 else 24 * d)
    (out * _dev(g)).sum().backward()
    r64 = torch.from_numpy(rots).double().requires_grad_(True)
    J64 = torch.from_numpy(Jtrs).double().requires_grad_(True)
    out64 = twin(r64, J64)
    (out64 * torch.from_numpy(g).double()).sum().backward()
    _close(out, out64.detach().numpy(), "out")
    _close(r.grad, r64.grad.numpy(), "drots")
    _close(J.grad, J64.grad.numpy(), "dJtrs")
    names = [n for n, _ in module.named_parameters()]
    assert len(names) == 98 + (2 if out_dim > 0 else 0)
    for (name, p), (_, q) in zip(module.named_parameters(), twin.named_parameters()):
        assert p.grad is not None, name
        _close(p.grad, q.grad.numpy(), name)


def test_encoder_errors(enc_small):
    module, rots, Jtrs, _, _ = enc_small
    nr = _nr()
    with pytest.raises(NotImplementedError):
        nr.pose_encode(ref.PoseEncoder(rel_joints=True).to(DEV), _dev(rots), _dev(Jtrs))
    with pytest.raises(NotImplementedError):
        nr.pose_encode(module, _dev(rots).repeat(2, 1, 1), _dev(Jtrs).repeat(2, 1, 1))
    with pytest.raises(NotImplementedError):
        nr.pose_encode(ref.PoseEncoder(dim_per_joint=17).to(DEV), _dev(rots), _dev(Jtrs))
    with pytest.raises(TypeError):
        nr.pose_encode(module, _dev(rots).double(), _dev(Jtrs))
    with pytest.raises(RuntimeError, match="GPU"):
        nr.pose_encode(module, _dev(rots), torch.from_numpy(Jtrs))
    with pytest.raises(TypeError):
        nr.pose_encode(ref.PoseEncoder(dtype=torch.float64).to(DEV), _dev(rots), _dev(Jtrs))


# ---------------------------------------------------------------------------------------------
# the delta application
# ---------------------------------------------------------------------------------------------
LEAVES = ("deltas", "xyz", "scaling", "rotation")


def _run_apply(inp, ups, so, ro, need=(True,) * 4, compute_loss=True, deltas_view=None):
    """Fused forward and backward: ({name: output}, {name: gradient of the leaves that want one})."""
    leaves = [_dev(inp[k]).requires_grad_(r) for k, r in zip(LEAVES, need)]
    first = leaves[0] if deltas_view is None else deltas_view(leaves[0])
    xyz_o, scal_o, rot_o, feat, losses = _nr().nonrigid_apply(first, *leaves[1:], scale_offset=so, rot_offset=ro,
                                                               compute_loss=compute_loss)
    n, D = first.shape
    assert tuple(xyz_o.shape) == (n, 3) and tuple(scal_o.shape) == (n, 3) and tuple(rot_o.shape) == (n, 4)
    assert (feat is None) == (D == 10) and (feat is None or (tuple(feat.shape) == (n, D - 10) and feat.is_contiguous()))
    assert sorted(losses) == (["nr_rot", "nr_scale", "nr_xyz"] if compute_loss else [])
    outs = dict(xyz_o=xyz_o, scal_o=scal_o, rot_o=rot_o)
    if feat is not None:
        outs["feat"] = feat
    if compute_loss:
        outs["nr"] = torch.stack([losses["nr_xyz"], losses["nr_scale"], losses["nr_rot"]])
    total = None
    for name, key in (("xyz_o", "g_xyz"), ("scal_o", "g_scal"), ("rot_o", "g_rot"), ("feat", "g_feat"), ("nr", "g_nr")):
        if ups.get(key) is not None and name in outs and outs[name].numel() and outs[name].requires_grad:
            term = (outs[name] * _dev(ups[key])).sum()
            total = term if total is None else total + term
    grads = {}
    wanted = [l for l in leaves if l.requires_grad]
    if wanted and total is not None:
        it = iter(torch.autograd.grad(total, wanted, allow_unused=True))
        for name, leaf in zip(ref.APPLY_GRADS, leaves):
            if leaf.requires_grad:
                grads[name] = next(it)
    return outs, grads


def _check_apply(outs, grads, want, what, inp=None):
    for name, v in outs.items():
        if name == "feat":
            assert torch.equal(v, _dev(inp["deltas"][:, 10:])), what + " feat"  # a copy: exact
        else:
            _close(v, want[name], "%s %s" % (what, name))
    for name, v in grads.items():
        w = want[name]
        if v is None:
            assert not np.abs(w).max(), "%s %s" % (what, name)
        else:
            _close(v, w, "%s %s" % (what, name))


@pytest.mark.parametrize("case", ref.APPLY_CASES)
def test_apply_fixture_parity(case):
    p = case + "/"
    so, ro, _ = case.split("_")
    inp = {k: FX[p + k] for k in LEAVES}
    ups = {k: FX.get(p + k) for k in ref.APPLY_UPS}
    outs, grads = _run_apply(inp, ups, so, ro)
    assert sorted(grads) == sorted(ref.APPLY_GRADS)
    for prec in ("f32", "f64"):
        _check_apply(outs, grads, {k: FX["%s%s_%s" % (p, k, prec)] for k in ref.APPLY_OUTS + ref.APPLY_GRADS},
                     "%s vs %s" % (case, prec), inp)
    if so == "zero":
        assert torch.equal(outs["scal_o"], _dev(inp["scaling"]))
    if so == "exp":  # the clamp rows: log(1e-6) and exactly zero gradients
        clamp = _dev((np.exp(inp["scaling"].astype(np.float64)) + inp["deltas"][:, 3:6] <= 0))
        assert clamp.sum() >= 9 and not grads["dscaling"][clamp].any()
        _close(outs["scal_o"][clamp], np.full(int(clamp.sum()), np.log(1e-6)), case + " clamped scaling'")
    if ro == "mult":
        assert not grads["ddeltas"][:, 6].any()
    assert torch.isfinite(grads["ddeltas"][3]).all()  # the zero offset row


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 64 * 256 + 1]
WIDTHS = [10, 11, 26, 74]


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_apply_sizes_against_restatement(n, D):
    so, ro = PAIRS[(n + D) % 6]
    inp, ups = ref.apply_inputs(n, D, seed=n + D, scale_offset=so)
    outs, grads = _run_apply(inp, ups, so, ro)
    if n == 0:
        assert all(v.numel() == 0 for k, v in outs.items() if k != "nr")
        assert tuple(grads["ddeltas"].shape) == (0, D) and torch.isnan(outs["nr"]).all()  # the mean of no rows, as torch has it
        return
    _check_apply(outs, grads, ref.apply_forward_backward(*[inp[k] for k in LEAVES], so, ro, **ups), "n=%d D=%d %s/%s" % (n, D, so, ro), inp)


@pytest.mark.parametrize("n,D", [(257, 11), (513, 26), (1000, 74), (255, 10)])
@pytest.mark.parametrize("so,ro", PAIRS)
@pytest.mark.parametrize("compute_loss", [True, False])
def test_apply_modes(n, D, so, ro, compute_loss):
    inp, ups = ref.apply_inputs(n, D, seed=3 * n + D, scale_offset=so)
    outs, grads = _run_apply(inp, ups, so, ro, compute_loss=compute_loss)
    want = ref.apply_forward_backward(*[inp[k] for k in LEAVES], so, ro, **dict(ups, g_nr=ups["g_nr"] if compute_loss else None))
    assert ("nr" in outs) == compute_loss
    _check_apply(outs, grads, want, "%s/%s n=%d D=%d loss=%s" % (so, ro, n, D, compute_loss), inp)


@pytest.mark.parametrize("key", ref.APPLY_UPS)
@pytest.mark.parametrize("so,ro", [("logit", "add"), ("exp", "mult"), ("zero", "mult")])
def test_apply_only_one_upstream_gradient(key, so, ro):
    inp, ups = ref.apply_inputs(700, 26, seed=17, scale_offset=so)
    one = {key: ups[key]}
    outs, grads = _run_apply(inp, one, so, ro)
    _check_apply({}, grads, ref.apply_forward_backward(*[inp[k] for k in LEAVES], so, ro, **one), "%s/%s only %s" % (so, ro, key))


@pytest.mark.parametrize("need", [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                                  (False, False, False, True), (False, True, True, True)])
def test_apply_partial_requires_grad(need):
    inp, ups = ref.apply_inputs(600, 26, seed=19, scale_offset="exp")
    outs, grads = _run_apply(inp, ups, "exp", "mult", need=need)
    assert sorted(grads) == sorted(n for n, r in zip(ref.APPLY_GRADS, need) if r)
    _check_apply(outs, grads, ref.apply_forward_backward(*[inp[k] for k in LEAVES], "exp", "mult", **ups), "need %s" % (need,), inp)


@pytest.mark.parametrize("so,ro", PAIRS)
def test_apply_kinks(so, ro):
    """Zero offset rows give finite, zero norm gradients; `exp` rows at or below zero give log(1e-6) and exactly zero
    gradients through the clamp."""
    n, D = 300, 26
    inp, ups = ref.apply_inputs(n, D, seed=23, scale_offset=so)
    inp["deltas"][::5, :10] = 0.0
    if so == "exp":
        inp["deltas"][1::5, 3:6] = -np.exp(inp["scaling"][1::5])  # exactly zero under the clamp
        inp["deltas"][2::5, 3:6] = -2.0
    only_nr = dict(g_nr=ups["g_nr"])
    outs, grads = _run_apply(inp, only_nr, so, ro)
    dd = grads["ddeltas"]
    assert torch.isfinite(dd).all() and not dd[::5].any()
    outs, grads = _run_apply(inp, ups, so, ro)
    _check_apply(outs, grads, ref.apply_forward_backward(*[inp[k] for k in LEAVES], so, ro, **ups), "kinks %s/%s" % (so, ro), inp)
    if so == "exp":
        for rows in (slice(1, None, 5), slice(2, None, 5)):
            got = outs["scal_o"][rows]
            _close(got, np.full(tuple(got.shape), np.log(1e-6)), "clamped scaling'")
            assert (got == got.flatten()[0]).all() and not grads["dscaling"][rows].any()
            w = float(ups["g_nr"][1]) / n  # the regulariser's term alone is left
            _close(grads["ddeltas"][rows, 3:6], w * np.sign(inp["deltas"][rows, 3:6].astype(np.float64)), "clamped dL/ddeltas")


def test_apply_non_contiguous_deltas():
    n, D = 777, 26
    inp, ups = ref.apply_inputs(n, D, seed=29)
    wide = np.zeros((n, 40), np.float32)
    wide[:, 3:3 + D] = inp["deltas"]
    outs, grads = _run_apply(dict(inp, deltas=wide), ups, "logit", "mult", deltas_view=lambda t: t[:, 3:3 + D])
    want = ref.apply_forward_backward(*[inp[k] for k in LEAVES], "logit", "mult", **ups)
    dd = grads.pop("ddeltas")
    assert not dd[:, :3].any() and not dd[:, 3 + D:].any()
    _close(dd[:, 3:3 + D], want["ddeltas"], "ddeltas through the view")
    _check_apply(outs, grads, want, "strided", inp)
    xyz_t = _dev(np.ascontiguousarray(inp["xyz"].T)).t()  # a transposed (N, 3)
    got = _nr().nonrigid_apply(_dev(inp["deltas"]), xyz_t, _dev(inp["scaling"]), _dev(inp["rotation"]))
    _close(got[0], want["xyz_o"], "xyz' from a transposed xyz")


def test_apply_large_against_restatement():
    inp, ups = ref.apply_inputs(200000, 26, seed=31)
    outs, grads = _run_apply(inp, ups, "logit", "mult")
    _check_apply(outs, grads, ref.apply_forward_backward(*[inp[k] for k in LEAVES], "logit", "mult", **ups), "200k", inp)


@pytest.mark.parametrize("so,ro", [("exp", "mult"), ("logit", "add")])
def test_apply_row_results_do_not_depend_on_the_batch(so, ro):
    n, D, r = 64 * 256 + 1, 26, 64 * 256
    inp, ups = ref.apply_inputs(n, D, seed=37, scale_offset=so)
    big = _run_apply(inp, ups, so, ro)
    one_inp = {k: v[r:r + 1] for k, v in inp.items()}
    one_ups = {k: v[r:r + 1] for k, v in ups.items() if k != "g_nr"}
    one_ups["g_nr"] = ups["g_nr"] * (np.float32(1.0) / np.float32(n))  # the kernel's own product: the mean's 1 / N is 1 for one row
    one = _run_apply(one_inp, one_ups, so, ro)
    for name in ("xyz_o", "scal_o", "rot_o", "feat"):
        assert torch.equal(big[0][name][r:r + 1], one[0][name]), name
    for name in ref.APPLY_GRADS:
        assert torch.equal(big[1][name][r:r + 1], one[1][name]), name


def test_apply_dtype_and_device_errors():
    inp, _ = ref.apply_inputs(10, 26, seed=1)
    t = {k: _dev(v) for k, v in inp.items()}
    with pytest.raises(TypeError):
        _nr().nonrigid_apply(**dict(t, deltas=t["deltas"].double()))
    with pytest.raises(RuntimeError, match="GPU"):
        _nr().nonrigid_apply(**dict(t, rotation=t["rotation"].cpu()))


# ---------------------------------------------------------------------------------------------
# both ops
# ---------------------------------------------------------------------------------------------
def test_bitwise_reproducible(enc_small):
    module, rots, Jtrs, g, _ = enc_small
    first = _run_enc(module, rots, Jtrs, g)
    for _ in range(2):
        again = _run_enc(module, rots, Jtrs, g)
        for a, b in zip(first[:3] + tuple(first[3]), again[:3] + tuple(again[3])):
            assert torch.equal(a, b)
    inp, ups = ref.apply_inputs(100001, 26, seed=41, scale_offset="exp")
    first = _run_apply(inp, ups, "exp", "mult")
    again = _run_apply(inp, ups, "exp", "mult")
    for a, b in zip(first, again):
        for name in a:
            assert torch.equal(a[name], b[name]), name


def _both_ops_step(module, n=5000, D=26, seed=43):
    """A step through both ops on persistent leaves: returns (leaves, step) with step() -> outputs and gradients."""
    rots, Jtrs = ref.random_pose(seed)
    inp, ups = ref.apply_inputs(n, D, seed=seed, scale_offset="exp")
    g_enc = _dev(np.random.default_rng(seed).normal(size=(1, module.n_output_dims)).astype(np.float32))
    gs = {k: _dev(v) for k, v in ups.items()}
    nr = _nr()
    params = module.encoder_parameters()

    def fresh():
        return [_dev(rots).requires_grad_(True), _dev(Jtrs).requires_grad_(True)] + [_dev(inp[k]).requires_grad_(True) for k in LEAVES]

    def step(leaves):
        out = nr.pose_encode(module, leaves[0], leaves[1])
        x, s, q, feat, losses = nr.nonrigid_apply(*leaves[2:], scale_offset="exp", rot_offset="mult")
        total = (out * g_enc).sum() + (x * gs["g_xyz"]).sum() + (s * gs["g_scal"]).sum() + (q * gs["g_rot"]).sum() + \
            (feat * gs["g_feat"]).sum() + gs["g_nr"][0] * losses["nr_xyz"] + gs["g_nr"][1] * losses["nr_scale"] + \
            gs["g_nr"][2] * losses["nr_rot"]
        grads = torch.autograd.grad(total, leaves + params)
        return (out, x, s, q, feat, losses["nr_xyz"], losses["nr_scale"], losses["nr_rot"]) + tuple(grads)

    return fresh, step


def test_no_host_sync(enc_small):
    fresh, step = _both_ops_step(enc_small[0])
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


def test_graph_capture_replays_bit_identical(enc_small):
    """torch's whole-network recipe (as tests/test_gpu_pose.py): fresh leaves first used on the side stream, then
    captured on it."""
    fresh, step = _both_ops_step(enc_small[0])
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


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
class _AABB(torch.nn.Module):  # utils/dataset_utils.py AABB.normalize, restated
    def __init__(self, cmax, cmin, dtype):
        super().__init__()
        self.register_buffer("coord_max", torch.tensor(cmax, dtype=dtype))
        self.register_buffer("coord_min", torch.tensor(cmin, dtype=dtype))

    def normalize(self, x, sym=False):
        x = (x - self.coord_min) / (self.coord_max - self.coord_min)
        return 2 * x - 1.0 if sym else x


class _HashGrid(torch.nn.Module):  # models/network_utils.py HashGrid: (x + 1) / 2 into the encoding
    def __init__(self, encode):
        super().__init__()
        self.encode = encode

    def forward(self, x):
        return self.encode((x + 1.0) * 0.5)


class _CondMLP(torch.nn.Module):
    """VanillaCondMLP's shape at a small size: the condition is concatenated to the input of the first layer."""

    def __init__(self, d_in, d_cond, d_out, dtype, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.l0, self.l1 = torch.nn.Linear(d_in + d_cond, 64).to(dtype), torch.nn.Linear(64, d_out).to(dtype)
        with torch.no_grad():
            for m in (self.l0, self.l1):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)

    def forward(self, x, cond=None):
        return self.l1(torch.nn.functional.softplus(self.l0(torch.cat([x, cond.expand(x.shape[0], -1)], 1)))) * 0.1


class _Gaussians(object):
    def __init__(self, xyz, scaling, rotation):
        self._xyz, self._scaling, self._rotation = xyz, scaling, rotation

    @property
    def get_xyz(self):
        return self._xyz

    def clone(self):
        return _Gaussians(self._xyz, self._scaling, self._rotation)


class _Deformer(torch.nn.Module):
    """A stand-in for HashGridwithMLP with the reference's attribute names."""

    def __init__(self, encode, n_feat, dtype, F, latent_dim, frames, cfg):
        super().__init__()
        self.cfg, self.delay, self.feature_dim, self.latent_dim = cfg, cfg.get("delay", 0), F, latent_dim
        self.pose_encoder = ref.PoseEncoder(dim_per_joint=6, seed=51, dtype=dtype)
        self.frame_dict = {f: k for k, f in enumerate(frames)}
        self.latent = torch.nn.Embedding(len(frames), latent_dim).to(dtype)
        with torch.no_grad():
            self.latent.weight.copy_(torch.from_numpy(np.random.default_rng(52).normal(size=(len(frames), latent_dim))))
        self.hashgrid = _HashGrid(encode)
        self.mlp = _CondMLP(n_feat, 24 * 6 + latent_dim, 10 + F, dtype, seed=53)
        self.aabb = _AABB([0.5, 1.0, 0.75], [-0.5, -1.0, -0.25], dtype)  # power-of-two extents: exact in fp32


@pytest.mark.parametrize("so,ro", [("logit", "add"), ("exp", "mult")])
def test_nonrigid_forward_end_to_end(so, ro):
    import tinycudann as tcnn
    from gsplat_mi355 import hashgrid as hg
    n, F, frames, frame = 400, 8, [2, 4, 6, 9], 6
    rng = np.random.default_rng(61)
    xyz0 = (rng.integers(0, 1024, (n, 3)) / 1024.0 * np.array([1.0, 2.0, 1.0]) + np.array([-0.5, -1.0, -0.25])).astype(np.float32)
    inp, ups = ref.apply_inputs(n, 10 + F, seed=62)
    inp["scaling"] += 4.0  # scales of order 1: the MLP's offsets (order 0.1) stay clear of the clamp of `exp`
    rots, Jtrs = ref.random_pose(63)
    cfg = dict(scale_offset=so, rot_offset=ro, delay=5)
    camera = type("Camera", (), {})()

    enc = tcnn.Encoding(3, HASH_CFG, seed=3)
    with torch.no_grad():
        enc.params.mul_(5000.0)  # table values of order 0.5, as the hash grid's own end-to-end test
    model = _Deformer(enc, 32, torch.float32, F, 4, frames, cfg).to(DEV)
    table = hg.levels(enc.cfg)
    p64 = torch.nn.Parameter(enc.params.detach().double().clone())
    twin = _Deformer(lambda x: hashgrid_ref.encode_torch(x, p64, table, 2), 32, torch.float64, F, 4, frames, cfg).to(DEV)

    def run(fused):
        dt = torch.float32 if fused else torch.float64
        t = lambda a: _dev(a).to(dt)
        gs = _Gaussians(t(xyz0).requires_grad_(True), t(inp["scaling"]).requires_grad_(True), t(inp["rotation"]).requires_grad_(True))
        camera.rots, camera.Jtrs, camera.frame_id = t(rots).requires_grad_(True), t(Jtrs).requires_grad_(True), frame
        if fused:
            early, none = _nr().nonrigid_forward(model, gs, 4, camera)  # below `delay`
            assert none == {} and early is not gs and not early.non_rigid_feature.any() and early._xyz is gs._xyz
            d, losses = _nr().nonrigid_forward(model, gs, 5, camera)
            assert sorted(losses) == ["nr_rot", "nr_scale", "nr_xyz"]
            assert _nr().nonrigid_forward(model, gs, 5, camera, compute_loss=False)[1] == {}
            out = dict(xyz=d._xyz, scaling=d._scaling, rotation=d._rotation, feature=d.non_rigid_feature, **losses)
            mod, table_param = model, enc.params
        else:  # the same chain in plain torch
            mod, table_param = twin, p64
            pose_feat = twin.pose_encoder(camera.rots, camera.Jtrs)
            idx = torch.tensor([twin.frame_dict[frame]], device=DEV)
            pose_feat = torch.cat([pose_feat, twin.latent(idx).expand(1, -1)], dim=1)
            deltas = twin.mlp(twin.hashgrid(twin.aabb.normalize(gs.get_xyz, sym=True)), cond=pose_feat)
            x, s, q, feat, nr3 = ref.apply(deltas, gs._xyz, gs._scaling, gs._rotation, so, ro)
            out = dict(xyz=x, scaling=s, rotation=q, feature=feat, nr_xyz=nr3[0], nr_scale=nr3[1], nr_rot=nr3[2])
        w = ups["g_nr"]
        ((out["xyz"] * t(ups["g_xyz"])).sum() + (out["scaling"] * t(ups["g_scal"])).sum() + (out["rotation"] * t(ups["g_rot"])).sum()
         + (out["feature"] * t(ups["g_feat"])).sum() + float(w[0]) * out["nr_xyz"] + float(w[1]) * out["nr_scale"]
         + float(w[2]) * out["nr_rot"]).backward()
        res = dict(out)
        res.update(dxyz=gs._xyz.grad, dscaling=gs._scaling.grad, drotation=gs._rotation.grad, drots=camera.rots.grad,
                   dJtrs=camera.Jtrs.grad, dtable=table_param.grad)
        res.update({"p." + name: p.grad for name, p in mod.named_parameters() if not name.startswith("hashgrid")})
        assert all(v is not None for v in res.values())
        return {k: v.detach().double().cpu().numpy() for k, v in res.items()}

    got, want = run(True), run(False)
    assert sorted(got) == sorted(want) and sum(k.startswith("p.pose_encoder") for k in want) == 98
    for name in want:
        _close(got[name], want[name], "end to end " + name)
    row = frames.index(frame)
    assert not np.delete(got["p.latent.weight"], row, axis=0).any() and got["p.latent.weight"][row].any()
