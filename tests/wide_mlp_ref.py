"""Float64 numpy restatement of the wide fused MLP (csrc/mlp_wide.hip; models/network_utils.py VanillaCondMLP and
HannwCondMLP with a frequency encoding, skip connections and the condition on the first layer or nowhere), with a
hand-written backward, the inputs the GPU tests draw and the loader of tests/golden/wide_mlp.npz.

  e = enc(x): x at multires 0, else [x (include_input) | w_0 sin(x) | w_0 cos(x) | w_1 sin(2 x) | w_1 cos(2 x) | ..]
  v_0 = [e | cond];  v_l = [h_l | e] / sqrt(2) for l in skip_in;  v_l = h_l otherwise;  z_l = v_l W_l^T + b_l
  h_{l+1} = z_l if z_l > 0 else slope z_l;  y = z_last
  dz_last = g;  dv_l = dz_l W_l (/ sqrt(2) at a skip, whose last E columns add to de);  dz_{l-1} = dv_l * (z_{l-1} > 0 ? 1 : slope)
  dW_l = dz_l^T v_l;  db_l = column sums of dz_l;  de += dz_0 W_0[:, :E];  dcond = W_0[:, E:]^T db_0
  dx = de_x + sum_k 2^k w_k (cos(2^k x) de_sin,k - sin(2^k x) de_cos,k)
"""
import numpy as np

KINK = 2e-5  # rows with a hidden |z| (fp64) below this are left out of gradient comparisons: see random_inputs
SQRT2 = np.sqrt(2.0)

# a network: dict(d, multires, include_input, C, width, n_hidden, skip_in, dout, slope)
def net(d, multires, C, width, n_hidden, skip_in, dout, include_input=True, slope=0.01):
    return dict(d=d, multires=multires, include_input=include_input, C=C, width=width, n_hidden=n_hidden,
                skip_in=tuple(skip_in), dout=dout, slope=slope)


# the reference's three configurations at full shape
NONRIGID = net(3, 6, 144, 256, 8, (4,), 26)
HANNW = net(3, 6, 144, 256, 8, (4,), 10, include_input=False, slope=0.0)
TEXTURE = net(271, 0, 0, 256, 4, (), 3)

# the fixture's cases (width 64, 40 rows); the hannw ones at three iterations of kick_in_iter 3000, full_band_iter 10000
ROWS = 40
CASES = {
    "enc_skip": net(3, 6, 5, 64, 3, (2,), 4),
    "enc_only": net(3, 2, 0, 64, 2, (), 5),
    "skip_plain": net(7, 0, 0, 64, 2, (1,), 4),
    "hannw_before": net(3, 6, 5, 64, 3, (2,), 10, include_input=False, slope=0.0),
    "hannw_mid": net(3, 6, 5, 64, 3, (2,), 10, include_input=False, slope=0.0),
    "hannw_full": net(3, 6, 5, 64, 3, (2,), 10, include_input=False, slope=0.0),
}
HANNW_ITERATIONS = {"hannw_before": 1000, "hannw_mid": 5800, "hannw_full": 20000}
HANNW_EMBEDDER = dict(kick_in_iter=3000, full_band_iter=10000)


def enc_dim(cfg):
    return cfg["d"] * ((1 if cfg["include_input"] else 0) + 2 * cfg["multires"]) if cfg["multires"] > 0 else cfg["d"]


def layer_shapes(cfg):
    """[(out, in)] of the nn.Linear layers, as the reference constructs them."""
    E, W, nh = enc_dim(cfg), cfg["width"], cfg["n_hidden"]
    shapes = []
    for l in range(nh + 1):
        out = cfg["dout"] if l == nh else (W - E if l + 1 in cfg["skip_in"] else W)
        shapes.append((out, E + cfg["C"] if l == 0 else W))
    return shapes


def hann_weights(multires, iteration, kick_in_iter, full_band_iter):
    """The Hann window per band, in float64."""
    if full_band_iter <= 0 or kick_in_iter >= full_band_iter:
        alpha = float(multires)
    else:
        alpha = multires * max(iteration - kick_in_iter, 0.0) / (full_band_iter - kick_in_iter)
    return [(1.0 - np.cos(np.pi * min(max(alpha - k, 0.0), 1.0))) / 2.0 for k in range(multires)]


def encode(x, cfg, band=None):
    x = np.asarray(x, np.float64)
    m = cfg["multires"]
    if m == 0:
        return x
    band = [1.0] * m if band is None else [float(w) for w in band]
    blocks = [x] if cfg["include_input"] else []
    for k in range(m):
        blocks += [band[k] * np.sin(x * 2.0 ** k), band[k] * np.cos(x * 2.0 ** k)]
    return np.concatenate(blocks, axis=1)


def forward(x, weights, biases, cfg, cond=None, band=None):
    """(y, zs, vs): the output, the hidden pre-activations and every layer's input (without the condition), float64."""
    W = [np.asarray(w, np.float64) for w in weights]
    b = [np.asarray(v, np.float64) for v in biases]
    e = encode(x, cfg, band)
    E, slope = e.shape[1], cfg["slope"]
    b0 = b[0] if cond is None else b[0] + W[0][:, E:] @ np.asarray(cond, np.float64).reshape(-1)
    zs, vs, h = [], [], e
    for l in range(len(W)):
        v = np.concatenate([h, e], axis=1) / SQRT2 if l in cfg["skip_in"] else h
        vs.append(v)
        z = v @ (W[0][:, :E] if l == 0 else W[l]).T + (b0 if l == 0 else b[l])
        if l == len(W) - 1:
            return z, zs, vs
        zs.append(z)
        h = np.where(z > 0, z, slope * z)


def forward_backward(x, weights, biases, cfg, cond=None, g=None, band=None):
    """dict(y, dx, dcond, dW=[..], db=[..]) in float64; `g` = dL/dy."""
    x = np.asarray(x, np.float64)
    W = [np.asarray(w, np.float64) for w in weights]
    nl, m, d, slope = len(W), cfg["multires"], x.shape[1], cfg["slope"]
    y, zs, vs = forward(x, W, biases, cfg, cond, band)
    E = vs[0].shape[1]
    out = dict(y=y, dW=[None] * nl, db=[None] * nl, dcond=None)
    de = np.zeros((x.shape[0], E))
    dz = np.asarray(g, np.float64)
    for l in range(nl - 1, -1, -1):
        out["dW"][l] = dz.T @ vs[l]
        out["db"][l] = dz.sum(0)
        if l == 0:
            de = de + dz @ W[0][:, :E]
            break
        dv = dz @ W[l]
        if l in cfg["skip_in"]:
            dv = dv / SQRT2
            de = de + dv[:, dv.shape[1] - E:]
            dv = dv[:, :dv.shape[1] - E]
        dz = dv * np.where(zs[l - 1] > 0, 1.0, slope)
    if m == 0:
        out["dx"] = de
    else:
        band = [1.0] * m if band is None else [float(w) for w in band]
        inc = 1 if cfg["include_input"] else 0
        dx = de[:, :d].copy() if inc else np.zeros_like(x)
        for k in range(m):
            f = 2.0 ** k
            ds, dc = de[:, (inc + 2 * k) * d:(inc + 2 * k + 1) * d], de[:, (inc + 2 * k + 1) * d:(inc + 2 * k + 2) * d]
            dx += f * band[k] * (np.cos(f * x) * ds - np.sin(f * x) * dc)
        out["dx"] = dx
    if cond is not None:
        c = np.asarray(cond, np.float64).reshape(-1)
        out["dW"][0] = np.concatenate([out["dW"][0], np.outer(out["db"][0], c)], axis=1)
        out["dcond"] = W[0][:, E:].T @ out["db"][0]
    return out


def random_params(cfg, seed):
    """(weights, biases), float32: weights uniform in +-sqrt(6 / ((1 + slope^2) fan_in)), biases in +-1 / sqrt(fan_in).
    (nn.Linear's own draw shrinks the pre-activations by about 0.4 a layer, and the kink filter then drops a third of the
    rows of an 8-layer network; with this gain every layer's pre-activation keeps a standard deviation of 0.6-1.2.)"""
    rng = np.random.default_rng(seed)
    weights, biases = [], []
    for out, fan_in in layer_shapes(cfg):
        k = np.sqrt(6.0 / ((1.0 + cfg["slope"] ** 2) * fan_in))
        weights.append(rng.uniform(-k, k, size=(out, fan_in)).astype(np.float32))
        biases.append(rng.uniform(-1.0, 1.0, size=(out,)).astype(np.float32) / np.float32(np.sqrt(fan_in)))
    return weights, biases


def random_inputs(n, weights, biases, cfg, seed, filtered=True, band=None):
    """(x (n, d), cond (C,) or None, g (n, dout)), float32.  A hidden pre-activation whose fp32 and fp64 signs differ
    flips a whole gradient path -- a threshold decision, not an error -- so with `filtered` the rows whose smallest hidden
    |z| (in fp64) is below KINK are dropped from what is drawn; at most 15 % of it may go."""
    rng = np.random.default_rng(seed)
    C = cfg["C"]
    cond = rng.normal(size=(C,)).astype(np.float32) if C else None
    drawn = n + n // 4 + 16 if filtered else n
    x = rng.uniform(-1.0, 1.0, size=(drawn, cfg["d"])).astype(np.float32)
    if filtered:
        _, zs, _ = forward(x, weights, biases, cfg, cond, band)
        keep = np.min([np.abs(z).min(axis=1) for z in zs], axis=0) >= KINK
        assert (~keep).sum() <= 0.15 * drawn, ((~keep).sum(), drawn)
        x = x[keep]
        assert x.shape[0] >= n, (x.shape[0], n)
        x = np.ascontiguousarray(x[:n])
    g = rng.normal(size=(n, cfg["dout"])).astype(np.float32)
    return x, cond, g


def load_fixture(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def case_call(fx, case):
    """(x, weights, biases, cond, g, band) of a fixture case; band is None for the un-windowed cases."""
    p, cfg = case + "/", CASES[case]
    nl = cfg["n_hidden"] + 1
    cond = fx[p + "cond"] if cfg["C"] else None
    band = fx[p + "band"] if case in HANNW_ITERATIONS else None
    return (fx[p + "x"], [fx["%sW%d" % (p, l)] for l in range(nl)], [fx["%sb%d" % (p, l)] for l in range(nl)], cond,
            fx[p + "g"], band)


def result_names(cfg):
    nl = cfg["n_hidden"] + 1
    names = ["y", "dx"] + (["dcond"] if cfg["C"] else [])
    return names + ["dW%d" % l for l in range(nl)] + ["db%d" % l for l in range(nl)]


def flat(res):
    """forward_backward's result under the fixture's names."""
    out = dict(y=res["y"], dx=res["dx"])
    if res["dcond"] is not None:
        out["dcond"] = res["dcond"]
    for l, (dW, db) in enumerate(zip(res["dW"], res["db"])):
        out["dW%d" % l], out["db%d" % l] = dW, db
    return out
