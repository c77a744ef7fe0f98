"""Writes tests/golden/lpips.npz (run from the repository root: python tests/golden/make_lpips_golden.py).

For every case of tests/lpips_ref.py CASES the image seeds 0, 1, 2, .. are tried until the ReLU margin -- the smallest
|pre-activation| of either branch divided by its layer's rms -- is at least lpips_ref.MARGIN: a ReLU whose pre-activation
is within fp32 rounding of zero may take the other branch in fp32, which changes the gradient by a finite amount, and a
comparison against float64 only means something where that cannot happen.  Recorded: per-layer weight checksums (a change
of the generator is then reported as such, not as a kernel failure), the images, the float64 loss, per-tap terms and both
input gradients, the error of the same chain in fp32 torch on the CPU against float64 (the yardstick of the GPU tests'
tolerances), the margin and the seed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lpips_ref as ref  # noqa: E402
import torch  # noqa: E402

MAX_SEEDS = 400


def main():
    sd = ref.weights()
    out = {"weight_checksums": ref.checksums(sd), "weight_seed": np.asarray([ref.WEIGHT_SEED], np.int64)}
    for case, (h, w, normalize) in ref.CASES.items():
        for seed in range(MAX_SEEDS):
            a, b = ref.images(h, w, seed)
            f64, margin = ref.forward_backward(a, b, sd, normalize, torch.float64)
            if margin >= ref.MARGIN:
                break
        else:
            raise SystemExit("%s: no seed below %d reaches the margin" % (case, MAX_SEEDS))
        f32, margin32 = ref.forward_backward(a, b, sd, normalize, torch.float32)
        out[case + "/in0"], out[case + "/in1"] = a.numpy(), b.numpy()
        out[case + "/seed"] = np.asarray([seed], np.int64)
        out[case + "/margin"] = np.asarray([margin], np.float64)
        for q in ref.QUANTITIES:
            out["%s/%s_f64" % (case, q)] = f64[q]
            out["%s/%s_err_f32" % (case, q)] = np.asarray([ref.rel_err(f32[q], f64[q])], np.float64)
        print(case, "seed", seed, "margin %.3g (fp32 %.3g)" % (margin, margin32),
              {q: "%.3g" % out["%s/%s_err_f32" % (case, q)][0] for q in ref.QUANTITIES}, "loss %.6g" % f64["loss"][0])
    np.savez_compressed(ref.FIXTURE, **out)
    print(ref.FIXTURE, os.path.getsize(ref.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
