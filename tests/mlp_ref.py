"""Float64 numpy restatement of the fused MLP (csrc/mlp.hip; models/network_utils.py VanillaCondMLP with `multires` 0, no
skip connections and the condition on the first layer or nowhere), with a hand-written backward, the inputs the GPU
tests draw and the loader of tests/golden/mlp.npz.

  y = L_last(leaky(.. leaky(L_0([x | cond])) ..)),  L_l(v) = v W_l^T + b_l,  leaky(z) = z if z > 0 else slope z
  dz_last = g;  dz_{l-1} = (dz_l W_l) * (1 if z_{l-1} > 0 else slope);  dW_l = dz_l^T a_{l-1};  db_l = column sums of dz_l
  dx = dz_0 W_0[:, :din];  dW_0[:, din:] = db_0 (x) cond;  dcond = W_0[:, din:]^T db_0
"""
import numpy as np

SLOPE = 0.01
KINK = 2e-5  # rows with a hidden |z| (fp64) below this are left out of gradient comparisons: see random_inputs
# the fixture's cases: (din, C, width, hidden layers, dout, rows)
CASES = {"in3": (3, 0, 32, 2, 4, 40), "in7": (7, 0, 32, 2, 5, 40), "cond": (3, 5, 32, 2, 6, 40)}


def forward(x, weights, biases, cond=None, slope=SLOPE):
    """(y, zs, acts): the output, the hidden pre-activations and post-activations, all float64."""
    x = np.asarray(x, np.float64)
    W = [np.asarray(w, np.float64) for w in weights]
    b = [np.asarray(v, np.float64) for v in biases]
    din = x.shape[1]
    b0 = b[0] if cond is None else b[0] + W[0][:, din:] @ np.asarray(cond, np.float64).reshape(-1)
    zs, acts, a = [], [], x
    for l in range(len(W)):
        z = a @ (W[0][:, :din] if l == 0 else W[l]).T + (b0 if l == 0 else b[l])
        if l == len(W) - 1:
            return z, zs, acts
        a = np.where(z > 0, z, slope * z)
        zs.append(z)
        acts.append(a)


def forward_backward(x, weights, biases, cond=None, g=None, slope=SLOPE):
    """dict(y, dx, dcond, dW=[..], db=[..]) in float64; `g` = dL/dy."""
    x = np.asarray(x, np.float64)
    W = [np.asarray(w, np.float64) for w in weights]
    din, nl = x.shape[1], len(W)
    y, zs, acts = forward(x, W, biases, cond, slope)
    out = dict(y=y, dW=[None] * nl, db=[None] * nl, dcond=None)
    dz = np.asarray(g, np.float64)
    for l in range(nl - 1, -1, -1):
        prev = x if l == 0 else acts[l - 1]
        out["dW"][l] = dz.T @ prev
        out["db"][l] = dz.sum(0)
        if l > 0:
            dz = (dz @ W[l]) * np.where(zs[l - 1] > 0, 1.0, slope)
    out["dx"] = dz @ W[0][:, :din]
    if cond is not None:
        c = np.asarray(cond, np.float64).reshape(-1)
        out["dW"][0] = np.concatenate([out["dW"][0], np.outer(out["db"][0], c)], axis=1)
        out["dcond"] = W[0][:, din:].T @ out["db"][0]
    return out


def random_params(din, C, width, n_hidden, dout, seed):
    """(weights, biases), float32, drawn as nn.Linear draws them: uniform in +-1 / sqrt(fan_in)."""
    rng = np.random.default_rng(seed)
    dims = [din + C] + [width] * n_hidden + [dout]
    weights, biases = [], []
    for l in range(len(dims) - 1):
        k = 1.0 / np.sqrt(dims[l])
        weights.append(rng.uniform(-k, k, size=(dims[l + 1], dims[l])).astype(np.float32))
        biases.append(rng.uniform(-k, k, size=(dims[l + 1],)).astype(np.float32))
    return weights, biases


def random_inputs(n, weights, biases, C, seed, filtered=True):
    """(x (n, din), cond (C,) or None, g (n, dout)), float32.  A hidden pre-activation whose fp32 and fp64 signs differ
    flips a whole gradient path -- a threshold decision, not an error -- so with `filtered` the rows whose smallest hidden
    |z| (in fp64) is below KINK are dropped from what is drawn; at most 15 % of it may go."""
    rng = np.random.default_rng(seed)
    din, dout = weights[0].shape[1] - C, weights[-1].shape[0]
    cond = rng.normal(size=(C,)).astype(np.float32) if C else None
    drawn = n + n // 4 + 16 if filtered else n
    x = rng.uniform(-1.0, 1.0, size=(drawn, din)).astype(np.float32)
    if filtered:
        _, zs, _ = forward(x, weights, biases, cond)
        keep = np.min([np.abs(z).min(axis=1) for z in zs], axis=0) >= KINK
        assert (~keep).sum() <= 0.15 * drawn, ((~keep).sum(), drawn)
        x = x[keep]
        assert x.shape[0] >= n, (x.shape[0], n)
        x = np.ascontiguousarray(x[:n])
    g = rng.normal(size=(n, dout)).astype(np.float32)
    return x, cond, g


def load_fixture(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def case_call(fx, case):
    """(x, weights, biases, cond, g) of a fixture case."""
    p = case + "/"
    nl = CASES[case][3] + 1
    cond = fx[p + "cond"] if CASES[case][1] else None
    return fx[p + "x"], [fx["%sW%d" % (p, l)] for l in range(nl)], [fx["%sb%d" % (p, l)] for l in range(nl)], cond, fx[p + "g"]


def result_names(case):
    nl = CASES[case][3] + 1
    names = ["y", "dx"] + (["dcond"] if CASES[case][1] else [])
    return names + ["dW%d" % l for l in range(nl)] + ["db%d" % l for l in range(nl)]


def flat(res):
    """forward_backward's result under the fixture's names."""
    out = dict(y=res["y"], dx=res["dx"])
    if res["dcond"] is not None:
        out["dcond"] = res["dcond"]
    for l, (dW, db) in enumerate(zip(res["dW"], res["db"])):
        out["dW%d" % l], out["db%d" % l] = dW, db
    return out
