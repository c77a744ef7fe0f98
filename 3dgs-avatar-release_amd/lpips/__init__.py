"""Drop-in for the one class of the `lpips` package the reference uses: `lpips.LPIPS(net='vgg')` (train.py:28,62-64,
127-138: the perceptual loss on the foreground crop of every iteration; utils/general_utils.py:279-291: the test metric).
The work runs in libgsplat_mi355's HIP kernels (csrc/lpips.hip) through gsplat_mi355.lpips; there is no CPU path.

Differences from upstream by design: the weights come from a local state-dict file (`model_path`, or the
environment variable GSPLAT_LPIPS_WEIGHTS) -- nothing is downloaded and no weights ship with this tree; net='vgg' only
(upstream's default net='alex' raises NotImplementedError); fp32 on the matrix unit with fixed-order sums (bitwise
reproducible, capture-safe).  The signature and the state-dict key names are recalled from the public package.
"""
from gsplat_mi355.lpips import LPIPS, foreground_box, perceptual_loss

__all__ = ["LPIPS", "foreground_box", "perceptual_loss"]
