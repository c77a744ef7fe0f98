"""Generates tests/golden/wide_mlp.npz by EXECUTING the reference's own VanillaCondMLP.forward and HannwCondMLP.forward with
its own encoders (models/network_utils.py) on the CPU (only possible where the reference tree exists; the tests only read
the .npz).

Taken from the syntax tree and executed, nothing else: the classes Embedder and HannwEmbedder, the functions get_embedder
and get_hannw_embedder, and the methods VanillaCondMLP.forward and HannwCondMLP.forward as plain functions (the module
itself cannot be imported: it needs packages that are absent here).  Stand-in: an object that carries what the methods
read -- lin0, lin1, .. (torch's own nn.Linear), config (cond_in, skip_in, multires, embedder), embed_fn (what
get_embedder returns, as VanillaCondMLP.__init__ sets it), num_layers and the activation (nn.LeakyReLU() / nn.ReLU()).
Each case runs in fp32 (the reference's precision) and in fp64 (the same parameter and input values).  Stored: inputs,
parameters, the Hann window's band weights as the reference's embedder computed them, outputs and the autograd gradients
of x, cond and every parameter for a seeded upstream gradient; nothing of the reference's text.  Keys
"<case>/{x,cond,g,band,W<l>,b<l>}" and "<case>/{y,dx,dcond,dW<l>,db<l>}_{f32,f64}".

Cases: tests/wide_mlp_ref.py CASES (width 64, 40 rows).

The generator asserts what lets the reference alone decide every activation branch the same way in both precisions: every
hidden pre-activation of the fp64 run is further than 1e-4 from 0 (the first seed for which the restatement says so is
taken; the reference's own values are then checked through forward hooks).

Run:  python tests/golden/make_wide_mlp_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import wide_mlp_ref as ref  # noqa: E402
from make_golden import REF, _CpuTorch, _exec_nodes, _method  # noqa: E402
from make_skinning_golden import _Obj, _precision  # noqa: E402

NETWORK_UTILS = "models/network_utils.py"
F32_BOUND = 1e-6  # the reference's fp32 against its fp64, of the largest magnitude (a tenth of the GPU tests' bar)


def _reference():
    path = os.path.join(REF, NETWORK_UTILS)
    tree = ast.parse(open(path).read(), filename=path)
    names = ("Embedder", "get_embedder", "HannwEmbedder", "get_hannw_embedder")
    picked = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert sorted(n.name for n in picked) == sorted(names)
    scope = _exec_nodes(picked, path, dict(torch=_CpuTorch(), np=np))
    fns = {}
    for cls in ("VanillaCondMLP", "HannwCondMLP"):
        node, _ = _method(NETWORK_UTILS, cls, "forward")
        fns[cls] = _exec_nodes([node], path, scope)["forward"]
    return scope, fns


def _band_of(scope, embedder, multires, iteration):
    """The weights the reference's HannwEmbedder closes over, one per band (its sin and cos lambdas share them)."""
    embed, _ = scope["get_hannw_embedder"](embedder, multires, iteration)
    fns = embed.__defaults__[0].embed_fns
    ws = [fn.__defaults__[2] for fn in fns]
    assert len(ws) == 2 * multires and all(float(ws[2 * k]) == float(ws[2 * k + 1]) for k in range(multires))
    assert all(w.dtype == torch.float32 for w in ws)
    return np.array([float(ws[2 * k]) for k in range(multires)], np.float32)


def _run(scope, fns, case, x, weights, biases, cond, g):
    cfg = ref.CASES[case]
    hannw = case in ref.HANNW_ITERATIONS
    n_hidden, C = cfg["n_hidden"], cfg["C"]
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            config = _Obj(cond_in=[0] if C else [], skip_in=list(cfg["skip_in"]), multires=cfg["multires"],
                          embedder=_Obj(**ref.HANNW_EMBEDDER))
            this = _Obj(config=config, embed_fn=None, num_layers=n_hidden + 2,
                        activation=torch.nn.ReLU() if hannw else torch.nn.LeakyReLU())
            if not hannw and cfg["multires"] > 0:
                this.embed_fn, width = scope["get_embedder"](cfg["multires"], input_dims=cfg["d"])
                assert width == ref.enc_dim(cfg)
            params, pre = [], []
            for l, (w, b) in enumerate(zip(weights, biases)):
                lin = torch.nn.Linear(w.shape[1], w.shape[0])
                with torch.no_grad():
                    assert lin.weight.dtype == dt
                    lin.weight.copy_(torch.from_numpy(w).to(dt))
                    lin.bias.copy_(torch.from_numpy(b).to(dt))
                if l < n_hidden:
                    lin.register_forward_hook(lambda m, i, o: pre.append(o.detach().numpy()))
                setattr(this, "lin%d" % l, lin)
                params += [lin.weight, lin.bias]
            leaves = [torch.from_numpy(x).to(dt).requires_grad_(True)]
            if C:
                leaves.append(torch.from_numpy(cond).to(dt).reshape(1, C).requires_grad_(True))
            kw = dict(cond=leaves[1] if C else None)
            if hannw:
                y = fns["HannwCondMLP"](this, leaves[0], ref.HANNW_ITERATIONS[case], **kw)
            else:
                y = fns["VanillaCondMLP"](this, leaves[0], **kw)
            assert y.dtype == dt and tuple(y.shape) == (ref.ROWS, cfg["dout"])
            grads = torch.autograd.grad((y * torch.from_numpy(g).to(dt)).sum(), leaves + params)
        out["y_" + tag], out["dx_" + tag] = y.detach().numpy(), grads[0].numpy()
        if C:
            out["dcond_" + tag] = grads[1].numpy().reshape(C)
        for l in range(n_hidden + 1):
            out["dW%d_%s" % (l, tag)] = grads[len(leaves) + 2 * l].numpy()
            out["db%d_%s" % (l, tag)] = grads[len(leaves) + 2 * l + 1].numpy()
        if tag == "f64":
            assert len(pre) == n_hidden and min(np.abs(z).min() for z in pre) > 1e-4
    return out


def main():
    scope, fns = _reference()
    out, worst = {}, 0.0
    for k, (case, cfg) in enumerate(ref.CASES.items()):
        band = None
        if case in ref.HANNW_ITERATIONS:
            band = _band_of(scope, _Obj(**ref.HANNW_EMBEDDER), cfg["multires"], ref.HANNW_ITERATIONS[case])
            assert np.allclose(band, ref.hann_weights(cfg["multires"], ref.HANNW_ITERATIONS[case], **ref.HANNW_EMBEDDER), atol=1e-6)
        seed = 70 + k
        while True:
            weights, biases = ref.random_params(cfg, seed)
            x, cond, g = ref.random_inputs(ref.ROWS, weights, biases, cfg, seed + 100, filtered=False)
            zs = ref.forward(x, weights, biases, cfg, cond, band)[1]
            if min(np.abs(z).min() for z in zs) > 2e-4:
                break
            seed += 1000
        p = case + "/"
        out[p + "x"], out[p + "g"] = x, g
        if cfg["C"]:
            out[p + "cond"] = cond
        if band is not None:
            out[p + "band"] = band
        for l, (w, b) in enumerate(zip(weights, biases)):
            out["%sW%d" % (p, l)], out["%sb%d" % (p, l)] = w, b
        res = _run(scope, fns, case, x, weights, biases, cond, g)
        for name in ref.result_names(cfg):
            f32, f64 = res[name + "_f32"], res[name + "_f64"]
            assert f32.dtype == np.float32 and f64.dtype == np.float64
            scale = np.abs(f64).max()
            err = np.abs(f32 - f64).max() / scale if scale > 0 else float(np.abs(f32).max())
            worst = max(worst, err)
            assert err <= F32_BOUND, (case, name, err)
        out.update({p + name: v for name, v in res.items()})
        print("%s: seed %d, smallest hidden |z| %.3g, band %s" % (case, seed, min(np.abs(z).min() for z in zs),
                                                                   None if band is None else band.tolist()))
    path = os.path.join(HERE, "wide_mlp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays); the reference's fp32 within %.3g of its fp64" % (path, os.path.getsize(path), len(out), worst))


if __name__ == "__main__":
    main()
