"""The converter's fused optimizer step on the CPU (no GPU needed): the new symbols are declared and exported, every
entry point validates its arguments before any HIP call, the Python front constructs and rejects what it must, and the
float64 restatement tests/optim_ref.py agrees with torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(weight_decay=...)
in float64 to 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_grad_norm_workspace_bytes", "gs_grad_norm", "gs_grad_scale", "gs_adam_step_ex")
GS_OK, GS_E_BAD_ARG, GS_E_WORKSPACE = 0, -1, -5


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


def test_symbols_declared_and_exported(lib):
    header = abi_header.text()
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert lib.GS_OPTIM_MAX_TENSORS >= 1024
    # the old entry point and its limit are untouched
    assert lib.GS_ADAM_MAX_TENSORS == 16
    # by-value tables stay under the 4 KB of kernel arguments
    assert ctypes.sizeof(lib.GsAdamTensorEx) == 64 and ctypes.sizeof(lib.GsGradTensor) == 16
    assert lib.GS_ADAM_EX_BATCH * (64 + 4) + 64 <= 4096 and lib.GS_GRAD_NORM_BATCH * (16 + 4) + 32 <= 4096
    assert lib.GS_ADAM_STEP_BATCH * 8 + 8 <= 4096
    capture_safe = header[header.index("Capture-safe"):header.index("Not capture-safe")]
    for name in ("gs_grad_norm", "gs_grad_scale", "gs_adam_step_ex"):
        assert name in capture_safe, name
    assert "NOT REWRITTEN" in header  # the one deliberate difference from clip_grad_norm_ + step


def _grads(lib, ns, ptr=0x1000):
    arr = (lib.GsGradTensor * max(len(ns), 1))()
    for k, n in enumerate(ns):
        arr[k] = lib.GsGradTensor(ptr, n)
    return arr


def _adam(lib, ns, ptr=0x1000, step=None):
    arr = (lib.GsAdamTensorEx * max(len(ns), 1))()
    for k, n in enumerate(ns):
        arr[k] = lib.GsAdamTensorEx(ptr, ptr, ptr, ptr, n, 1e-3, 0.05, step, None)
    return arr


def test_argument_validation_needs_no_device(lib):
    """Everything below returns before the first HIP call (the pointers are never dereferenced)."""
    L = lib.load()
    out = ctypes.c_size_t(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    too_many = lib.GS_OPTIM_MAX_TENSORS + 1

    # gs_grad_norm_workspace_bytes
    assert L.gs_grad_norm_workspace_bytes(1, _grads(lib, [5]), None) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(1, None, ctypes.byref(out)) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(-1, _grads(lib, [5]), ctypes.byref(out)) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(1, _grads(lib, [-1]), ctypes.byref(out)) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(1, _grads(lib, [5], ptr=None), ctypes.byref(out)) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(too_many, _grads(lib, [1] * too_many), ctypes.byref(out)) == GS_E_BAD_ARG
    assert L.gs_grad_norm_workspace_bytes(0, None, ctypes.byref(out)) == GS_OK and out.value >= 4
    assert L.gs_grad_norm_workspace_bytes(3, _grads(lib, [1, 0, 4097]), ctypes.byref(out)) == GS_OK
    need = out.value
    assert need >= 4 * 2 and need % 4 == 0                # at least one partial per non-empty tensor
    assert L.gs_grad_norm_workspace_bytes(lib.GS_OPTIM_MAX_TENSORS, _grads(lib, [1] * lib.GS_OPTIM_MAX_TENSORS),
                                          ctypes.byref(out)) == GS_OK

    # gs_grad_norm
    g3 = _grads(lib, [1, 0, 4097])
    assert L.gs_grad_norm(3, g3, 0.1, None, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(3, g3, 0.1, p, None, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(3, None, 0.1, p, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(3, g3, -1.0, p, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(3, g3, float("nan"), p, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(1, _grads(lib, [-5]), 0.1, p, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(1, _grads(lib, [5], ptr=None), 0.1, p, p, need, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(too_many, _grads(lib, [1] * too_many), 0.1, p, p, 1 << 20, None) == GS_E_BAD_ARG
    assert L.gs_grad_norm(3, g3, 0.1, p, p, need - 4, None) == GS_E_WORKSPACE
    assert L.gs_grad_norm(3, g3, 0.1, p, p, 0, None) == GS_E_WORKSPACE
    assert L.gs_grad_norm(0, None, 0.1, p, p, 4, None) == GS_OK

    # gs_grad_scale
    assert L.gs_grad_scale(3, g3, None, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(3, None, p, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(-1, g3, p, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(1, _grads(lib, [-5]), p, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(1, _grads(lib, [5], ptr=None), p, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(too_many, _grads(lib, [1] * too_many), p, None) == GS_E_BAD_ARG
    assert L.gs_grad_scale(0, None, p, None) == GS_OK

    # gs_adam_step_ex
    a2 = _adam(lib, [7, 0])
    assert L.gs_adam_step_ex(2, None, 0.9, 0.999, 1e-15, 1, None, None) == GS_E_BAD_ARG
    assert L.gs_adam_step_ex(-1, a2, 0.9, 0.999, 1e-15, 1, None, None) == GS_E_BAD_ARG
    assert L.gs_adam_step_ex(1, _adam(lib, [-7]), 0.9, 0.999, 1e-15, 1, None, None) == GS_E_BAD_ARG
    assert L.gs_adam_step_ex(too_many, _adam(lib, [1] * too_many), 0.9, 0.999, 1e-15, 1, None, None) == GS_E_BAD_ARG
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        bad = _adam(lib, [7])
        setattr(bad[0], field, None)
        assert L.gs_adam_step_ex(1, bad, 0.9, 0.999, 1e-15, 1, None, None) == GS_E_BAD_ARG, field
    # a step of 0 (or below) with no device step; also when only one of the tensors lacks it
    assert L.gs_adam_step_ex(2, a2, 0.9, 0.999, 1e-15, 0, None, None) == GS_E_BAD_ARG
    assert L.gs_adam_step_ex(2, a2, 0.9, 0.999, 1e-15, -3, None, None) == GS_E_BAD_ARG
    mixed = _adam(lib, [7, 9], step=p)
    mixed[1].step = None
    assert L.gs_adam_step_ex(2, mixed, 0.9, 0.999, 1e-15, 0, None, None) == GS_E_BAD_ARG
    assert L.gs_adam_step_ex(0, None, 0.9, 0.999, 1e-15, 0, None, None) == GS_OK
    assert L.gs_adam_step_ex(0, None, 0.9, 0.999, 1e-15, 1, p, None) == GS_OK
    # the old entry point keeps its limit
    assert L.gs_adam_step(17, (lib.GsAdamTensor * 17)(), 0.9, 0.999, 1e-15, 1, None) == GS_E_BAD_ARG


def test_python_front_constructs_and_rejects():
    from gsplat_mi355.optim import FusedAdam, clip_grad_norm_, converter_optimize
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(3)]
    opt = FusedAdam([dict(params=ps[:2], lr=1e-3), dict(params=ps[2:], lr=1e-4, weight_decay=0.05)], lr=1e-3, eps=1e-15)
    assert [g["weight_decay"] for g in opt.param_groups] == [0, 0.05]
    opt = FusedAdam(ps, lr=1e-3, weight_decay=0.05, capturable=True, max_grad_norm=0.1)
    assert opt.param_groups[0]["weight_decay"] == 0.05 and opt.param_groups[0]["capturable"] is True
    assert opt.max_grad_norm == 0.1 and opt.total_norm is None
    with pytest.raises(NotImplementedError):
        FusedAdam(ps, amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdam(ps, weight_decay=-1.0)
    with pytest.raises(ValueError):
        FusedAdam(ps, max_grad_norm=-1.0)
    # state-dict layout: torch.optim.Adam loads it, and the other way round
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3)) for _ in range(3)], lr=1e-3, weight_decay=0.05)
    ref.load_state_dict(opt.state_dict())
    opt.load_state_dict(ref.state_dict())
    assert opt.param_groups[0]["weight_decay"] == 0.05
    # clip_grad_norm_: other norms, CPU gradients, nothing to clip
    for p in ps:
        p.grad = torch.ones(3)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(ps, 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(ps, 1.0, norm_type=float("inf"))
    with pytest.raises(RuntimeError, match="fp32 GPU"):
        clip_grad_norm_(ps, 1.0)
    for p in ps:
        p.grad = None
    assert float(clip_grad_norm_(ps, 1.0)) == 0.0
    assert callable(converter_optimize)


@pytest.mark.parametrize("max_norm", [None, 0.1, 1e6])
def test_restatement_agrees_with_float64_torch(max_norm):
    """clip_grad_norm_ + Adam(weight_decay) in float64 on the CPU, three steps, one tensor without a gradient, one
    empty, two groups with different lr / weight decay / betas; 1e-12 relative to each tensor's maximum."""
    rs = np.random.default_rng(5)
    sizes = [1, 3, 1023, 0, 1025, 4097, 17]
    group_of = [0, 0, 0, 0, 1, 1, 1]
    no_grad = 2
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0),
              dict(lr=5e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05)]
    init = [rs.normal(size=n) for n in sizes]
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    opt = torch.optim.Adam([dict(params=[p for p, g in zip(ps, group_of) if g == gi], **h) for gi, h in enumerate(groups)])
    P, M, V = [a.copy() for a in init], [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes]
    steps = [0] * len(sizes)
    for t in range(3):
        grads = [rs.normal(size=n) * 10.0 ** rs.uniform(-3, 1) for n in sizes]
        grads[no_grad] = None
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        norm_t = None
        if max_norm is not None:
            norm_t = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        steps = [s + (g is not None) for s, g in zip(steps, grads)]
        P, M, V, norm = optim_ref.clip_adam_step(P, grads, M, V, [groups[g] for g in group_of], steps, max_norm)
        if max_norm is not None:
            assert abs(norm - float(norm_t)) <= 1e-12 * float(norm_t)
            for p, g in zip(ps, optim_ref.clip_grads(grads, max_norm)[0]):
                if g is not None and g.size:
                    assert np.abs(p.grad.numpy() - g).max() <= 1e-12 * np.abs(g).max()
        for k, p in enumerate(ps):
            if sizes[k] == 0:
                continue
            if k == no_grad:
                assert np.array_equal(p.detach().numpy(), init[k]) and p not in opt.state
                continue
            st = opt.state[p]
            assert float(st["step"]) == steps[k]
            for got, want in ((p.detach().numpy(), P[k]), (st["exp_avg"].numpy(), M[k]), (st["exp_avg_sq"].numpy(), V[k])):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, t)


def test_restatement_keeps_non_finite_values_where_torch_does():
    for bad in (np.inf, np.nan):
        g = [np.array([1.0, bad, -2.0]), np.array([0.5])]
        ps = [torch.nn.Parameter(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)), torch.nn.Parameter(torch.tensor([4.0], dtype=torch.float64))]
        for p, a in zip(ps, g):
            p.grad = torch.from_numpy(a.copy())
        opt = torch.optim.Adam(ps, lr=1e-2, weight_decay=0.05)
        nt = torch.nn.utils.clip_grad_norm_(ps, 0.1)
        opt.step()
        P, M, V, norm = optim_ref.clip_adam_step([np.array([1.0, 2.0, 3.0]), np.array([4.0])], g, [np.zeros(3), np.zeros(1)],
                                                 [np.zeros(3), np.zeros(1)], [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)] * 2,
                                                 [1, 1], 0.1)
        assert np.isnan(norm) == bool(torch.isnan(nt)) and np.isinf(norm) == bool(torch.isinf(nt))
        for p, q in zip(ps, P):
            assert np.array_equal(np.isnan(p.detach().numpy()), np.isnan(q))
            assert np.array_equal(np.isfinite(p.detach().numpy()), np.isfinite(q))
