"""The LPIPS-VGG op on the GPU (csrc/lpips.hip) against float64 torch (tests/lpips_ref.py, tests/golden/lpips.npz).

Per layer: gs_lpips_conv, forward and backward-data, against float64 conv2d on maps of one pixel, smaller than a tile and
across tile edges in both directions; the bound is the rounding-error bound of a sequential fp32 sum of K = 9 Cin products,
(K + 8) 2^-24 sum |x| |w| per element (the 8: the bias, the input transform and its factor).  The pools are exact.
Whole network: loss, per-tap terms and input gradients within 16 x the error of fp32 torch on the CPU recorded in the
fixture for that case and quantity (the MFMA adds up to 4608 products in one sequential chain where the CPU GEMM adds in
blocks), on fixtures whose ReLU margin is asserted first.  Measured on an MI355X (max |delta| / max |reference|; in
brackets the recorded fp32-torch error, sixteen times which is the bound):
    n16  loss 1.1e-07 (4.6e-08)  taps 7.8e-08 (1.7e-07)  g0 5.2e-07 (1.2e-06)  g1 4.1e-07 (6.5e-07)
    r16  loss 5.7e-09 (5.7e-09)  taps 3.8e-08 (4.7e-08)  g0 1.0e-06 (1.5e-06)  g1 1.2e-06 (1.9e-06)
    n37  loss 1.5e-08 (1.5e-08)  taps 6.0e-08 (6.0e-08)  g0 8.1e-07 (1.0e-06)  g1 7.9e-07 (1.1e-06)
    r37  loss 8.9e-08 (2.7e-08)  taps 2.8e-08 (5.2e-08)  g0 1.0e-06 (1.3e-06)  g1 1.7e-06 (1.4e-06)
(with every output summed in one chain of 9 Cin products and plain pixel sums the r16 loss was 2.3e-07, above its bound
of 9.2e-08: the kernel now sums chunk by chunk and compensates the pixel sums).
Behaviour: identical bits run to run and stream to stream, a crop view gives the bits of its copy, nothing is saved under
no_grad, forward + backward replayed from a hipGraph are the eager bits, perceptual_loss is the hand-made crop."""
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LAYER_OF = {(3, 64): 0, (64, 64): 1, (128, 256): 4, (512, 512): 10}
MAPS = ((1, 1), (2, 1), (3, 5), (17, 19), (33, 40))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


@pytest.fixture(scope="module")
def model(dev):
    import lpips
    m = lpips.LPIPS(net="vgg", pretrained=False, verbose=False)
    m.load_state_dict(ref.weights())
    return m.to(dev)


def _nhwc(t):  # (C, H, W) -> (H, W, C) contiguous
    return t.permute(1, 2, 0).contiguous()


def _conv(model, dev, layer, backward, h, w, inp, mask, out, cs=0, rs=0, normalize=1):
    from gsplat_mi355 import _lib
    with _lib.on_device(dev):
        _lib.check(_lib.load().gs_lpips_conv(model.packed(dev).data_ptr(), layer, backward, normalize, h, w, inp.data_ptr(), cs, rs,
                                             _lib.ptr(mask), out.data_ptr(), _lib.stream_ptr(dev)))
    return out


@pytest.mark.parametrize("chans", sorted(LAYER_OF))
def test_one_layer_forward_and_backward_data_against_float64(model, dev, chans):
    cin, cout = chans
    layer = LAYER_OF[chans]
    sd = ref.weights()
    key = ref.trunk_keys()[layer]
    w64, b64 = sd[key + ".weight"].double(), sd[key + ".bias"].double()
    gen = torch.Generator().manual_seed(100 + layer)
    shift, scale = torch.tensor(ref.SHIFT, dtype=torch.float64).reshape(3, 1, 1), torch.tensor(ref.SCALE, dtype=torch.float64).reshape(3, 1, 1)
    for h, w in MAPS:
        # ---- forward: relu(conv(x) + b)
        if layer == 0:  # a strided crop of a larger image, read in place and transformed on the way
            big = torch.rand(3, h + 7, w + 9, generator=gen, dtype=torch.float32).to(dev)
            view = big[:, 3:3 + h, 5:5 + w]
            x64 = ((2 * view.cpu().double() - 1) - shift) / scale
            got = _conv(model, dev, 0, 0, h, w, view, None, torch.empty(h, w, cout, device=dev), cs=view.stride(0), rs=view.stride(1))
        else:
            x = torch.randn(cin, h, w, generator=gen, dtype=torch.float32)
            x64 = x.double()
            got = _conv(model, dev, layer, 0, h, w, _nhwc(x).to(dev), None, torch.empty(h, w, cout, device=dev))
        want = F.relu(F.conv2d(x64[None], w64, b64, padding=1))[0]
        bound = (9 * cin + 8) * U * (F.conv2d(x64.abs()[None], w64.abs(), b64.abs(), padding=1)[0])
        err = (got.cpu().double().permute(2, 0, 1) - want).abs()
        assert (want > 0).any() and bool((err <= bound).all()), (chans, h, w, float((err / bound).max()))
        # ---- backward-data: conv_transpose(dz * (a > 0)), the mask a saved activation with exact zeros
        act = F.relu(torch.randn(cout, h, w, generator=gen, dtype=torch.float32))
        dz = torch.randn(cout, h, w, generator=gen, dtype=torch.float32)
        assert (act == 0).any() or h * w * cout < 4
        masked = (dz * (act > 0)).double()
        want = F.conv_transpose2d(masked[None], w64, padding=1)[0]
        bound = (9 * cout + 8) * U * F.conv_transpose2d(masked.abs()[None], w64.abs(), padding=1)[0]
        if layer == 0:  # the image gradient (3, H, W), times the transform's factor 2 / scale
            got = _conv(model, dev, 0, 1, h, w, _nhwc(dz).to(dev), _nhwc(act).to(dev), torch.empty(3, h, w, device=dev)).cpu().double()
            want, bound = want * 2 / scale, bound * 2 / scale
        else:
            got = _conv(model, dev, layer, 1, h, w, _nhwc(dz).to(dev), _nhwc(act).to(dev), torch.empty(h, w, cin, device=dev))
            got = got.cpu().double().permute(2, 0, 1)
        err = (got - want).abs()
        assert want.abs().max() > 0 and bool((err <= bound).all()), (chans, h, w, "bwd", float((err / bound.clamp_min(1e-300)).max()))


def test_pools_forward_and_backward_are_exact(dev):
    from gsplat_mi355 import _lib
    L = _lib.load()

    def run(x, g, dp):
        c, h, w = x.shape
        out = torch.empty(h // 2, w // 2, c, device=dev)
        back = torch.empty(h, w, c, device=dev)
        xd, gd, dpd = _nhwc(x).to(dev), _nhwc(g).to(dev), _nhwc(dp).to(dev)
        with _lib.on_device(dev):
            _lib.check(L.gs_lpips_pool(0, h, w, c, xd.data_ptr(), None, None, out.data_ptr(), _lib.stream_ptr(dev)))
            _lib.check(L.gs_lpips_pool(1, h, w, c, xd.data_ptr(), gd.data_ptr(), dpd.data_ptr(), back.data_ptr(), _lib.stream_ptr(dev)))
        return out.cpu().permute(2, 0, 1), back.cpu().permute(2, 0, 1)

    gen = torch.Generator().manual_seed(7)
    # 3 x 5: floor drops a row and a column; 6 x 4; a window of four equal values: the first one takes the gradient
    for x in (torch.randn(64, 3, 5, generator=gen), torch.randn(128, 6, 4, generator=gen), torch.full((4, 2, 2), 0.5),
              F.relu(torch.randn(64, 8, 6, generator=gen))):
        c, h, w = x.shape
        g, dp = torch.randn(c, h, w, generator=gen), torch.randn(c, h // 2, w // 2, generator=gen)
        xr = x.clone().requires_grad_(True)
        pooled = F.max_pool2d(xr[None], 2, 2)[0]
        pooled.backward(dp)
        out, back = run(x, g, dp)
        assert torch.equal(out, pooled.detach()) and torch.equal(back, g + xr.grad)
    x = torch.full((4, 2, 2), 0.5)
    g, dp = torch.zeros(4, 2, 2), torch.ones(4, 1, 1)
    _, back = run(x, g, dp)
    assert torch.equal(back[:, 0, 0], torch.ones(4)) and float(back.sum()) == 4.0


def _check(case, fx, got):
    """Prints every measured error next to its bound, then asserts them all."""
    assert float(fx[case + "/margin"][0]) >= ref.MARGIN  # no ReLU within fp32 rounding of zero: float64 is the truth here
    bad = []
    for q, value in got.items():
        err = ref.rel_err(value, fx["%s/%s_f64" % (case, q)])
        e32 = float(fx["%s/%s_err_f32" % (case, q)][0])
        print("lpips-measure %s %s gpu %.3g torch-fp32 %.3g bound %.3g" % (case, q, err, e32, 16 * e32))
        if not err <= 16 * e32:
            bad.append((q, err, 16 * e32))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_whole_network_3d_call_both_gradients(model, dev, fx, case):
    h, w, normalize = ref.CASES[case]
    a = torch.from_numpy(fx[case + "/in0"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(fx[case + "/in1"]).to(dev).requires_grad_(True)
    val, per = model(a, b, retPerLayer=True, normalize=normalize)
    assert tuple(val.shape) == (1, 1, 1, 1) and len(per) == 5 and all(tuple(p.shape) == (1, 1, 1, 1) for p in per)
    val.sum().backward()
    _check(case, fx, dict(loss=val.detach().cpu().numpy(), taps=torch.cat(per).flatten().cpu().numpy(), g0=a.grad.cpu().numpy(),
                          g1=b.grad.cpu().numpy()))


@pytest.mark.parametrize("case", list(ref.CASES))
def test_whole_network_4d_call_in0_alone(model, dev, fx, case):
    h, w, normalize = ref.CASES[case]
    a = torch.from_numpy(fx[case + "/in0"]).to(dev)[None].requires_grad_(True)
    b = torch.from_numpy(fx[case + "/in1"]).to(dev)[None]
    val = model(a, b, normalize=normalize)
    assert tuple(val.shape) == (1, 1, 1, 1)
    (3.0 * val.mean()).backward()
    _check(case, fx, dict(loss=val.detach().cpu().numpy(), g0=a.grad[0].cpu().numpy() / 3.0))


def test_batches_loop_and_other_dtypes(model, dev, fx):
    a = torch.from_numpy(fx["n16/in0"]).to(dev)
    b = torch.from_numpy(fx["n16/in1"]).to(dev)
    with torch.no_grad():
        one = model(a, b, normalize=True)
        two = model(torch.stack([a, b]), torch.stack([b, b]), normalize=True)
        dbl = model(a.double(), b.double(), normalize=True)
    assert tuple(two.shape) == (2, 1, 1, 1) and torch.equal(two[0], one[0]) and float(two[1]) == 0.0
    assert torch.equal(dbl, one)  # (the fixture's images are fp32 values)
    ad = a.double().requires_grad_(True)
    model(ad, b, normalize=True).sum().backward()
    assert ad.grad.dtype == torch.float64 and ref.rel_err(ad.grad.cpu().numpy(), fx["n16/g0_f64"]) <= 16 * float(fx["n16/g0_err_f32"][0])


def _run(model, a, b, normalize=True):
    a = a.detach().requires_grad_(True)
    val = model(a, b, normalize=normalize)
    val.sum().backward()
    return val.detach().clone(), a.grad.clone()


def test_same_bits_run_to_run_stream_to_stream_and_from_a_crop_view(model, dev, fx):
    a = torch.from_numpy(fx["n37/in0"]).to(dev)
    b = torch.from_numpy(fx["n37/in1"]).to(dev)
    v0, g0 = _run(model, a, b)
    v1, g1 = _run(model, a, b)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        v2, g2 = _run(model, a, b)
    side.synchronize()
    assert torch.equal(v0, v2) and torch.equal(g0, g2)
    # a crop of a larger image, read in place; the gradient returns through autograd's slice backward
    h, w = a.shape[1:]
    big = torch.rand(3, h + 11, w + 6, device=dev)
    big[:, 4:4 + h, 2:2 + w] = a
    big.requires_grad_(True)
    gt = torch.rand(3, h + 11, w + 6, device=dev)
    gt[:, 4:4 + h, 2:2 + w] = b
    val = model(big[:, 4:4 + h, 2:2 + w], gt[:, 4:4 + h, 2:2 + w], normalize=True)
    val.sum().backward()
    assert torch.equal(val, v0) and torch.equal(big.grad[:, 4:4 + h, 2:2 + w], g0)
    outside = big.grad.clone()
    outside[:, 4:4 + h, 2:2 + w] = 0
    assert float(outside.abs().max()) == 0.0


def test_nothing_is_saved_without_a_gradient(model, dev, fx, monkeypatch):
    from gsplat_mi355 import _lib, lpips as gl
    h, w = 37, 29
    fwd = lambda g0, g1: gl.workspace_bytes(h, w, g0, g1, _lib.GS_LPIPS_WS_FORWARD) + gl.workspace_bytes(h, w, g0, g1, _lib.GS_LPIPS_WS_SAVED)
    assert gl.workspace_bytes(h, w, 0, 0, _lib.GS_LPIPS_WS_SAVED) == 0
    assert fwd(0, 0) < fwd(1, 0) < fwd(1, 1)
    asked = []
    real = gl.workspace_bytes
    monkeypatch.setattr(gl, "workspace_bytes", lambda *args: asked.append(args) or real(*args))
    a = torch.from_numpy(fx["n37/in0"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(fx["n37/in1"]).to(dev)
    with torch.no_grad():
        quiet = model(a, b, normalize=True)
    assert all(args[2:4] == (False, False) for args in asked) and not quiet.requires_grad
    del asked[:]
    loud = model(a, b, normalize=True)  # the ground truth never needs a gradient: only in0's branch saves
    assert all(args[2:4] == (True, False) for args in asked) and loud.requires_grad and torch.equal(loud, quiet)


def test_forward_and_backward_replayed_from_a_graph_are_the_eager_bits(model, dev, fx):
    a = torch.from_numpy(fx["n16/in0"]).to(dev)
    b = torch.from_numpy(fx["n16/in1"]).to(dev).clone()
    eager, eager_grad = _run(model, a, b)
    torch.cuda.synchronize()

    def step(leaf):
        val = model(leaf, b, normalize=True)
        val.sum().backward()
        return val

    # torch's whole-network recipe (tests/test_gpu_capture.py): a fresh leaf, warmed up on the side stream, then captured
    leaf = a.clone().requires_grad_(True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            leaf.grad = None
            step(leaf)
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    leaf.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        val = step(leaf)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(val.detach(), eager) and torch.equal(leaf.grad, eager_grad)
    # other pixels through the same graph: the replay reads the images where they live
    with torch.no_grad():
        leaf.copy_(torch.from_numpy(fx["r16/in0"]).to(dev))
        b.copy_(torch.from_numpy(fx["r16/in1"]).to(dev))
    g.replay()
    torch.cuda.synchronize()
    got_val, got_grad = val.detach().clone(), leaf.grad.clone()
    v2, g2 = _run(model, leaf.detach().clone(), b)
    assert torch.equal(got_val, v2) and torch.equal(got_grad, g2) and not torch.equal(v2, eager)


def test_perceptual_loss_is_the_hand_made_crop_and_caches_its_box(model, dev):
    from gsplat_mi355 import lpips as gl

    class Camera(object):
        pass

    gen = torch.Generator().manual_seed(11)
    image = torch.rand(3, 64, 64, generator=gen).to(dev).requires_grad_(True)
    gt = torch.rand(3, 64, 64, generator=gen).to(dev)
    cam = Camera()
    cam.original_mask = torch.zeros(1, 64, 64, device=dev)
    cam.original_mask[0, 10:30, 30:47] = 1.0  # a 20 x 17 foreground
    loss = gl.perceptual_loss(model, image, gt, cam)
    box = cam._gsplat_foreground_box
    assert box == (10, 30, 30, 47) and loss.dim() == 0
    loss.backward()
    crop = image.detach()[:, 10:30, 30:47].contiguous().requires_grad_(True)
    want = model(crop, gt[:, 10:30, 30:47].contiguous(), normalize=True).mean()
    want.backward()
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(image.grad[:, 10:30, 30:47], crop.grad)
    outside = image.grad.clone()
    outside[:, 10:30, 30:47] = 0
    assert float(outside.abs().max()) == 0.0 and float(crop.grad.abs().max()) > 0  # nothing outside the box
    # the second step on the same camera: the box object is reused and the mask is not looked at (no device-to-host copy)
    cam.original_mask = None
    again = gl.perceptual_loss(model, image, gt, cam)
    assert cam._gsplat_foreground_box is box and torch.equal(again.detach(), want.detach())
