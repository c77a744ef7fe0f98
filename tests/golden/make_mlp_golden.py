"""Generates tests/golden/mlp.npz by EXECUTING the reference's own VanillaCondMLP.forward (models/network_utils.py) on the
CPU (only possible where the reference tree exists; the tests only read the .npz).

Taken from the syntax tree and executed as a plain function, nothing else: the method VanillaCondMLP.forward (the module
itself cannot be imported: it needs packages that are absent here).  Stand-in: an object that carries what the method
reads -- lin0, lin1, .. (torch's own nn.Linear), config (cond_in, skip_in), embed_fn = None, num_layers and
nn.LeakyReLU().  Each case runs in fp32 (the reference's precision) and in fp64 (the same parameter and input values).
Stored: inputs, parameters, outputs and the autograd gradients of x, cond and every parameter for a seeded upstream
gradient; nothing of the reference's text.  Keys "<case>/{x,cond,g,W<l>,b<l>}" and "<case>/{y,dx,dcond,dW<l>,db<l>}_{f32,f64}".

Cases (tests/mlp_ref.py CASES; width 32, two hidden layers, 40 rows):
  in3   dim_in 3, dim_out 4          in7   dim_in 7, dim_out 5          cond  dim_in 3, cond_in [0] with 5 values, dim_out 6

The generator asserts what lets the reference alone decide every LeakyReLU branch the same way in both precisions: every
hidden pre-activation of the fp64 run is further than 1e-4 from 0 (the first seed for which the restatement says so is
taken; the reference's own values are then checked through forward hooks).

Run:  python tests/golden/make_mlp_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import mlp_ref as ref  # noqa: E402
from make_golden import _CpuTorch, _exec_nodes, _method  # noqa: E402
from make_skinning_golden import _Obj, _precision  # noqa: E402


def _reference_forward():
    node, path = _method("models/network_utils.py", "VanillaCondMLP", "forward")
    return _exec_nodes([node], path, dict(torch=_CpuTorch(), np=np))["forward"]


def _run(fn, case, x, weights, biases, cond, g):
    din, C, width, n_hidden, dout, n = ref.CASES[case]
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with _precision(dt):
            this = _Obj(config=_Obj(cond_in=[0] if C else [], skip_in=[]), embed_fn=None, num_layers=n_hidden + 2,
                        activation=torch.nn.LeakyReLU())
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
            y = fn(this, leaves[0], cond=leaves[1] if C else None)
            assert y.dtype == dt and tuple(y.shape) == (n, dout)
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
    fn = _reference_forward()
    out = {}
    for k, (case, (din, C, width, n_hidden, dout, n)) in enumerate(ref.CASES.items()):
        seed = 40 + k
        while True:
            weights, biases = ref.random_params(din, C, width, n_hidden, dout, seed)
            x, cond, g = ref.random_inputs(n, weights, biases, C, seed + 100, filtered=False)
            zs = ref.forward(x, weights, biases, cond)[1]
            if min(np.abs(z).min() for z in zs) > 2e-4:
                break
            seed += 1000
        p = case + "/"
        out[p + "x"], out[p + "g"] = x, g
        if C:
            out[p + "cond"] = cond
        for l, (w, b) in enumerate(zip(weights, biases)):
            out["%sW%d" % (p, l)], out["%sb%d" % (p, l)] = w, b
        res = _run(fn, case, x, weights, biases, cond, g)
        for name in ref.result_names(case):
            f32, f64 = res[name + "_f32"], res[name + "_f64"]
            assert f32.dtype == np.float32 and f64.dtype == np.float64
            # the reference's fp32 within a tenth of the GPU tests' bar of its fp64
            assert np.abs(f32 - f64).max() <= 1e-6 * np.abs(f64).max(), (case, name)
        out.update({p + name: v for name, v in res.items()})
        print("%s: seed %d, smallest hidden |z| %.3g" % (case, seed, min(np.abs(z).min() for z in zs)))
    path = os.path.join(HERE, "mlp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
