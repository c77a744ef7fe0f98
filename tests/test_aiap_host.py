"""The AIAP regularisers' C ABI and fixture on the CPU (no GPU needed): the new symbols are declared and exported,
workspace sizes and argument validation work without a device, and the float64 restatement tests/aiap_ref.py
reproduces the reference's own fp64 autograd results (tests/golden/aiap.npz) to 1e-12."""
import ctypes
import os

import numpy as np
import pytest

import abi_header
import aiap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_aiap_workspace_bytes", "gs_aiap_forward", "gs_aiap_backward")
CASES = {"a": ("xyz", "cov"), "b": ("x",), "c": ("x",), "d": ("x",), "e": ("x",)}


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(ROOT, "tests", "golden", "aiap.npz"))
    return {k: d[k] for k in d.files}


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    import gsplat_mi355.aiap as a
    assert callable(a.aiap_loss) and callable(a.full_aiap_loss)


def test_workspace_sizes(lib):
    L = lib.load()
    ws = lambda n, k, s=2: lib.nbytes(L.gs_aiap_workspace_bytes, n, k, s)
    by_n = [ws(n, 5) for n in (1, 1000, 200000, 1100000)]
    assert by_n == sorted(by_n) and len(set(by_n)) == len(by_n)
    by_k = [ws(200000, k) for k in range(2, 9)]
    assert by_k == sorted(by_k) and len(set(by_k)) == len(by_k)
    for n, k in ((1, 2), (1000, 5), (200000, 8)):
        assert ws(n, k) >= n * (k - 1) * 16 + (n + 1) * 4  # keys and values twice over, the list starts
        assert ws(n, k) % 256 == 0
    out = ctypes.c_size_t(0)
    for n, k, s in ((0, 5, 2), (-1, 5, 2), (10, 1, 2), (10, 9, 2), (10, 5, 0), (10, 5, 3), (400000000, 8, 1)):
        assert L.gs_aiap_workspace_bytes(n, k, s, ctypes.byref(out)) == -1, (n, k, s)
    assert L.gs_aiap_workspace_bytes(10, 5, 1, None) == -1


def test_argument_validation_without_a_device(lib):
    L = lib.load()
    fake = 0x1000  # never dereferenced: validation fails first
    nb = lib.nbytes(L.gs_aiap_workspace_bytes, 10, 5, 2)

    def sets(*specs):
        arr = (lib.GsAiapSet * max(len(specs), 1))()
        for k, (d, xc, xd, loss) in enumerate(specs):
            arr[k] = lib.GsAiapSet(xc=xc, xd=xd, D=d, loss=loss)
        return arr

    good = (3, fake, fake, fake)
    fwd = lambda n=10, k=5, idx=fake, ns=1, s=None, ws=fake, b=nb: L.gs_aiap_forward(
        n, k, idx, ns, sets(good) if s is None else s, ws, b, None)
    bwd = lambda n=10, k=5, idx=fake, ns=1, s=None, ws=fake, b=nb: L.gs_aiap_backward(
        n, k, idx, ns, sets(good) if s is None else s, ws, b, None)
    for call in (fwd, bwd):
        assert call(n=0) == -1
        assert call(k=1) == -1
        assert call(k=9) == -1
        assert call(ns=0) == -1
        assert call(ns=3) == -1
        assert call(idx=None) == -1
        assert call(ws=None) == -1
        assert call(s=sets((4, fake, fake, fake))) == -1                   # D not 3 or 6
        assert call(s=sets((3, None, fake, fake))) == -1                   # no xc
        assert call(s=sets((3, fake, None, fake))) == -1                   # no xd
        assert call(ns=2, s=sets(good, (6, fake, None, fake))) == -1      # the second set's xd
        assert call(b=nb - 1) == -5                                        # workspace too small
    assert L.gs_aiap_forward(10, 5, fake, 1, None, fake, nb, None) == -1  # no sets
    assert fwd(s=sets((3, fake, fake, None))) == -1                       # the forward needs somewhere for the loss


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_reference_fp64(fx, case):
    idx = fx["%s/idx" % case]
    for name in CASES[case]:
        p = "%s/%s/" % (case, name)
        loss, gc, gd = aiap_ref.aiap(fx[p + "xc"], fx[p + "xd"], idx)
        assert abs(loss - float(fx[p + "loss_f64"])) <= 1e-12 * max(abs(loss), 1e-300), (case, name)
        for got, key in ((gc, "gxc_f64"), (gd, "gxd_f64")):
            want = fx[p + key]
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (case, name, key)


def test_fixture_cases_hold_what_they_claim(fx):
    # (c): pairs with a = 0, with b = 0 and with both; (d): everything zero; elsewhere the sign margin
    a, b = aiap_ref.distances(fx["c/x/xc"], fx["c/x/xd"], fx["c/idx"])
    i, j = aiap_ref.pairs(fx["c/idx"])
    assert ((a == 0) & (b > 0)).any() and ((b == 0) & (a > 0)).any() and ((a == 0) & (b == 0) & (i != j)).any()
    assert float(fx["d/x/loss_f64"]) == 0.0 and not fx["d/x/gxc_f64"].any() and not fx["d/x/gxd_f64"].any()
    for case, name in (("a", "xyz"), ("a", "cov"), ("b", "x"), ("e", "x")):
        a, b = aiap_ref.distances(fx["%s/%s/xc" % (case, name)], fx["%s/%s/xd" % (case, name)], fx["%s/idx" % case])
        live = (a > 0) & (b > 0)
        assert (np.abs(a - b)[live] >= 1e-3 * np.maximum(a, b)[live]).all(), (case, name)
    counts = np.bincount(fx["e/idx"][:, 1:].reshape(-1), minlength=fx["e/idx"].shape[0])
    assert counts[0] >= fx["e/idx"].shape[0]  # the hub
