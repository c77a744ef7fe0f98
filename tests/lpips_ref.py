"""A torch restatement of LPIPS-VGG (csrc/lpips.hip carries the spec) for the tests: F.conv2d, F.max_pool2d, the head and
autograd, in float64 (the reference) or float32 (the yardstick of the tolerances).  It also generates the weights -- 14.7 M
of them cannot be committed: He-scaled trunk, biases of 0.05 sigma, non-negative lin vectors, from a CPU torch.Generator --
and reads the fixture tests/golden/lpips.npz (written by tests/golden/make_lpips_golden.py), which pins per-layer weight
checksums, the images, the float64 results, the error of the same chain in fp32 torch on the CPU, and every case's ReLU
margin.  Structure and key names are recalled from the public lpips / torchvision packages; neither was available."""
import collections
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_LAYERS = (1, 3, 6, 9, 12)
POOL_BEFORE = (2, 4, 7, 10)  # a 2x2 max-pool in front of these layers
VGG_INDEX = ((1, 0), (1, 2), (2, 5), (2, 7), (3, 10), (3, 12), (3, 14), (4, 17), (4, 19), (4, 21), (5, 24), (5, 26), (5, 28))
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
WEIGHT_SEED = 20240
MARGIN = 1e-5  # every case's ReLU margin is at least this (the fixture maker searches image seeds until it is)
# name: (H, W, normalize).  16 x 16: relu5_3 is one pixel; 37 x 29: every pool floors (37>18>9>4>2, 29>14>7>3>1)
CASES = collections.OrderedDict((("n16", (16, 16, True)), ("r16", (16, 16, False)), ("n37", (37, 29, True)), ("r37", (37, 29, False))))
QUANTITIES = ("loss", "taps", "g0", "g1")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")


def trunk_keys():
    return ["net.slice%d.%d" % si for si in VGG_INDEX]


def random_state_dict(seed=WEIGHT_SEED):
    """fp32 weights under the keys lpips.LPIPS(net='vgg').state_dict() uses (as recalled)."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = collections.OrderedDict()
    sd["scaling_layer.shift"] = torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1)
    for l, key in enumerate(trunk_keys()):
        sigma = math.sqrt(2.0 / (9 * CHANNELS[l]))
        sd[key + ".weight"] = torch.randn(CHANNELS[l + 1], CHANNELS[l], 3, 3, generator=gen, dtype=torch.float32) * sigma
        sd[key + ".bias"] = torch.randn(CHANNELS[l + 1], generator=gen, dtype=torch.float32) * (0.05 * sigma)
    for k, l in enumerate(TAP_LAYERS):
        c = CHANNELS[l + 1]
        sd["lin%d.model.1.weight" % k] = torch.rand(1, c, 1, 1, generator=gen, dtype=torch.float32) / c
    return sd


_cache = {}


def weights(seed=WEIGHT_SEED):
    """The random state dict, generated once per process and left unchanged."""
    if seed not in _cache:
        _cache[seed] = random_state_dict(seed)
    return _cache[seed]


def checksums(sd):
    """(13 + 5, 2) float64: the sum and the absolute sum of every trunk layer's weight and bias together, then of the lins."""
    rows = []
    for key in trunk_keys():
        w, b = sd[key + ".weight"].double(), sd[key + ".bias"].double()
        rows.append((float(w.sum() + b.sum()), float(w.abs().sum() + b.abs().sum())))
    for k in range(5):
        v = sd["lin%d.model.1.weight" % k].double()
        rows.append((float(v.sum()), float(v.abs().sum())))
    return np.asarray(rows, np.float64)


def transform(x, sd, normalize, dtype):
    if normalize:
        x = 2 * x - 1
    return (x - sd["scaling_layer.shift"].to(dtype)[0]) / sd["scaling_layer.scale"].to(dtype)[0]


def trunk(x, sd, dtype):
    """x (3, H, W), transformed -> (the five taps (1, C, h, w), the thirteen pre-activations)."""
    h, taps, pre = x[None], [], []
    for l, key in enumerate(trunk_keys()):
        if l in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        z = F.conv2d(h, sd[key + ".weight"].to(dtype), sd[key + ".bias"].to(dtype), padding=1)
        pre.append(z)
        h = F.relu(z)
        if l in TAP_LAYERS:
            taps.append(h)
    return taps, pre


def _unit(f):
    return f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)


def lpips(in0, in1, sd, normalize, dtype=torch.float64):
    """(loss, the five per-tap terms (5,), the pre-activations of both branches)."""
    t0, pre0 = trunk(transform(in0.to(dtype), sd, normalize, dtype), sd, dtype)
    t1, pre1 = trunk(transform(in1.to(dtype), sd, normalize, dtype), sd, dtype)
    terms = []
    for k in range(5):
        d = (_unit(t0[k]) - _unit(t1[k])) ** 2
        lin = sd["lin%d.model.1.weight" % k].to(dtype)
        terms.append(F.conv2d(d, lin).mean())
    terms = torch.stack(terms)
    loss = terms[0]
    for k in range(1, 5):
        loss = loss + terms[k]
    return loss, terms, (pre0, pre1)


def forward_backward(in0, in1, sd, normalize, dtype=torch.float64):
    """{loss, taps, g0, g1} as numpy arrays of `dtype`, and the ReLU margin: the smallest |pre-activation| over both
    branches (the in0 branch included) divided by its layer's rms."""
    a = in0.detach().clone().to(dtype).requires_grad_(True)
    b = in1.detach().clone().to(dtype).requires_grad_(True)
    loss, terms, pres = lpips(a, b, sd, normalize, dtype)
    g0, g1 = torch.autograd.grad(loss, (a, b))
    margin = min(float(z.detach().abs().min() / z.detach().pow(2).mean().sqrt()) for pre in pres for z in pre)
    out = dict(loss=loss.detach().reshape(1).numpy(), taps=terms.detach().numpy(), g0=g0.numpy(), g1=g1.numpy())
    return out, margin


def images(h, w, seed):
    """Two fp32 images in [0, 1]: a smooth random one and a perturbed copy."""
    gen = torch.Generator().manual_seed(int(seed))
    a = torch.rand(3, h, w, generator=gen, dtype=torch.float32)
    b = (a + 0.15 * torch.randn(3, h, w, generator=gen, dtype=torch.float32)).clamp(0.0, 1.0)
    return a, b


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64).reshape(want.shape)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)


def load_fixture(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
