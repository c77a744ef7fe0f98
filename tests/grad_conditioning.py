"""The per-Gaussian gradient bar: every element of a rasterizer gradient against a bound made of ITS OWN Gaussian's sums, not
of the tensor's maximum.  Shared by tests/test_grad_conditioning_host.py (the bound validated on the references alone) and
tests/test_gpu_grad_conditioning.py (the device against it).

The oracle's or_render_backward_cond returns, per Gaussian i and per sum k of the render backward (oracle.SUMS), n_i pairs,
A_ik = the sum over the pairs of the term's absolute form, B_ik = the same weighted with (Q + m) (gs_oracle.c).  With
u = 2^-24 an fp32 evaluation of sum k of Gaussian i may be off by

    u (n_i A_ik + C0 A_ik + C1 B_ik + C3 R_ik)

n_i A_ik: the worst case of an fp32 sum of n_i terms in ANY order (|fl(sum) - sum| <= (n - 1) u sum|t| + O(u^2), Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2) -- derived, not measured.

C0, C1: the rounding inside one term, counted on the oracle's expressions (or_render_backward_cond), one u per fp32
operation, 2 u (one ulp) for expf, for a hardware exp2 / reciprocal and for a divide; exact operations (a multiplication by
0.5, by 0.5 W, fminf, a negation) cost nothing.  The longest path of the nine terms is e[0] / e[1]:

    dx = xy - pix                                                      1
    G = expf(power)                                                    2      (the error of `power` itself: C1)
    alpha = co3 G                                                      1
    accum_rec = last_alpha last_color + (1 - last_alpha) accum_rec     4
    (col - accum_rec) dLp, three of them added                         1 + 1 + 3
    ... T                                                              1
    1 - alpha;  T_final / (1 - alpha);  bg_dot (mul, add);  ... bg_dot 1 + 2 + 2 + 1
    dL_dalpha = ... + ...                                              1
    dL_dG = co3 dL_dalpha                                              1
    gdx = G dx                                                         1
    dG_ddelx = -gdx co0 - gdy co1                                      2      (mul, sub)
    dL_dG dG_ddelx ddelx_dx                                            1      (ddelx_dx = W / 2 is exact)
                                                                      --
                                                                      26
  per unit of Q: power = -0.5 (co0 dx dx + co2 dy dy) - co1 dx dy: each product carries dx twice (2) and two
    multiplications (2), the two additions 1 each: 6 u Q absolute in `power`, that is 6 u Q relative in G;
  per unit of m: one factor of T: alpha (mul 1, expf 2), 1 - alpha (1), the division or multiplication (2):           6.

The count is doubled for the device (another operation order, FMA contraction, v_exp_f32 in the log2 domain):
C0 = 52, C1 = 12.  tests/test_grad_conditioning_host.py validates the count at HALF these constants: the oracle's fp32 terms
summed in double (no n_i part) against the float64 twin, every element.

C3 cond_R, in the device's bound only: csrc/render_bwd.hip walks FRONT to back and forms (its header, "FRONT-to-back
recurrence")  dL/dalpha_i = T_i (c_i . g) - Rem_i / (1 - alpha_i),  Rem_i = Gtot - sum_{j <= i} (c_j . g) alpha_j T_j,
Gtot = out_color . g: "the rest of the pixel" is a running difference that starts from the pixel's TOTAL.  Its roundings
are relative to that total, Gabs = sum_c (Cabs_c + |T_final bg_c|) |g_c|, not to T_i times it, so behind a near-opaque stack
(T_i of 1e-2 .. 1e-4) the device's dL/dalpha is a difference of numbers 1 / T_i larger than itself -- an error the back-to-front
form A, which carries T_i, does not admit.  Counted on the kernel's expression: per pair in front, the forward's colour sum
(alpha T: 1, the FMA: 1) and the backward's Rem (alpha T: 1, the FMA: 1) = 4 per unit of m; once: Gtot (3), out_color's
background FMA (1), v_rcp_f32 (1 ulp = 2), T (c . g) - Rem rcp (2) = 8: (4 m + 8) u Gabs / (1 - alpha) = C3 (m + 2) with
C3 = 4, no doubling (this IS the device's order).  cond_R is the sum over the pairs of (m + 2) x the geometric sums' absolute
form with dL_dalpha -> Gabs / (1 - alpha).  Found on the device (ladder / wall / edge: without this term the six geometric
sums exceeded the bound 3 to 33 times, only in the decades of A_i below 1, the colour sums 0.03 at most; the Long frame, no
T below 6e-3, 0.009 at most) and reproduced without one: test_grad_conditioning_host.py evaluates the recurrence above in fp32.

Derived tensors (means3D, cov3D_precomp, scales, rotations, sh; the opacities under antialiasing) are per-Gaussian linear
images of the nine sums, J_i s_i (oracle.preprocess_jacobian).  Their bound is

    2 (|J_i| bound_i + C2 u |J_i| |s_i|)

C2 counts or_preprocess_backward's longest chain, conic -> cov2D -> cov3D -> rotations, in relative errors: one u per
operation, a product carries the sum of its factors' errors, a sum of like-sized addends the largest addend's plus one per
addition (what the cancellation inside the chain loses beyond that is not in |J_i|, the END-TO-END Jacobian: the host test of
the eight probes measures it):

    M = J Rv: t = p V (6), t.x / t.z and the clamp times t.z (3), J02 = -(fx t.x) / (t.z t.z) (4), the entry (3)        16
    cov2D entry: M twice (32), two dot products of three (10), + 0.3 (1)                                                43
    denom = a c - b b: 2 x 43 + 3 = 89;   denom2inv = 1 / (denom denom + 1e-7): 2 x 89 + 1 + 1 + 2                     182
    dL_da = denom2inv (-c c gA + 2 b c gB + (denom - a c) gC): (89 + 1 + 1) + 2, times denom2inv (182 + 1)            276
    dL_dcov3D entry = m m dL_da + ...: 2 x 16 + 276 + 2 + 2                                                            312
    dL/dL = 2 dS L, L = R diag(s): R (5), L (1), a dot product of three (5)                                            323
    dR = dL s (1);  gq = 2 z (dR - dR) + ... (four addends: 1 + 2 + 3)                                                 330

doubled as above: C2 = 660; the outer factor 2 is because the reference for these rows is the oracle's own fp32
or_preprocess_backward."""
import functools
import math

import numpy as np
import torch

import helpers

U = 2.0 ** -24
C0, C1, C2, C3 = 52.0, 12.0, 660.0, 4.0
COND = ("cond_n", "cond_A", "cond_B", "cond_R", "sums")
W, H = 40, 24  # one full tile row, a partial row, a partial column
BG = (0.3, 0.6, 0.1)
DIRECT = {"means2D": (0, 1), "opacities": (5,), "colors_precomp": (6, 7, 8)}  # tensor -> its columns of oracle.SUMS


def sum_bound(cond, scale=1.0, with_n=True, front_to_back=True):
    """[P, 9]: the bound of the nine sums; `scale` on C0 and C1 (0.5 in the validation on the references, which also
    leaves out the n_i part and the front-to-back walk's term: the oracle walks back to front and adds in double)."""
    n = cond["cond_n"][:, None].astype(np.float64) if with_n else 0.0
    r = C3 * cond["cond_R"] if front_to_back else 0.0
    return U * (n * cond["cond_A"] + scale * (C0 * cond["cond_A"] + C1 * cond["cond_B"]) + r)


def add_conditions(a, b):
    """The conditions of two images' backward passes into the same gradient add (and so do their sums)."""
    return {k: a[k] + b[k] for k in COND}


def direct_bound(cond, name):
    b = sum_bound(cond)[:, DIRECT[name]]
    if name == "means2D":
        b = np.concatenate([b, np.zeros((b.shape[0], 1))], 1)  # (the third column is never written)
    return b


def derived_bound(oracle, cond, J, J_chain=None):
    """[P, K] for one derived tensor with Jacobian J [P, K, 9] (see the module docstring).  `J_chain`: what the chain's own
    rounding is relative to where that is more than |J| (sh_jacobian_abs)."""
    return 2.0 * (oracle.through_jacobian(J, sum_bound(cond)) +
                  C2 * U * oracle.through_jacobian(J if J_chain is None else J_chain, np.abs(cond["sums"])))


def sh_jacobian_abs(sc, fw, J_sh):
    """The SH rows' Jacobian with every basis polynomial replaced by its absolute form (each addition by the sum of the
    absolute values of its addends; or_preprocess_backward, (v)).  x (xx - 3 yy) and its like vanish on cones of directions:
    there the fp32 value of the basis -- the oracle's as much as the device's -- is off by u times the monomials, not by u
    times their difference (found on the Wall scene: one Gaussian's 16th basis value is -1.07e-6, the oracle's own fp32
    evaluation of it 25 000 u from float64).  Zero where J_sh is (clamped channels, culled Gaussians)."""
    from oracle import dense_ref as dr
    d = sc.means3D.astype(np.float64) - sc.campos.astype(np.float64)[None]
    x, y, z = (np.abs(d / np.linalg.norm(d, axis=1, keepdims=True))).T
    xx, yy, zz = x * x, y * y, z * z
    c2, c3 = np.abs(dr.C2), np.abs(dr.C3)
    b = [np.full_like(x, dr.C0), dr.C1 * y, dr.C1 * z, dr.C1 * x,
         c2[0] * x * y, c2[1] * y * z, c2[2] * (2 * zz + xx + yy), c2[3] * x * z, c2[4] * (xx + yy),
         c3[0] * y * (3 * xx + yy), c3[1] * x * y * z, c3[2] * y * (4 * zz + xx + yy), c3[3] * z * (2 * zz + 3 * xx + 3 * yy),
         c3[4] * x * (4 * zz + xx + yy), c3[5] * z * (xx + yy), c3[6] * x * (xx + 3 * yy)]
    out = np.zeros(J_sh.shape)
    for k in range(min(sc.M, (sc.sh_degree + 1) ** 2)):
        for c in range(3):
            out[:, 3 * k + c, 6 + c] = b[k] * (J_sh[:, c, 6 + c] != 0)  # (row c: coefficient 0, SH_C0: non-zero unless clamped or culled)
    return out


def ratios(got, want, bound):
    """error / bound per element (0 / 0 = 0: an exact zero where nothing may contribute; x / 0 = inf)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


def decade_table(ratio, A_row):
    """{decade of A_i: largest ratio among the Gaussians of that decade} for printing."""
    out = {}
    ok = A_row > 0
    dec = np.floor(np.log10(A_row[ok])).astype(int)
    r = ratio.reshape(ratio.shape[0], -1).max(1)[ok]
    for d in np.unique(dec):
        out[int(d)] = float(r[dec == d].max())
    return out


def premise(cond, want, names, decades, tag=""):
    """What every scene asserts before it compares anything: the visible Gaussians' A_i (of the means2D sums) span
    `decades` decades, and at least a quarter of the visible Gaussians have rows below 1e-5 of their tensor's maximum in
    every tensor of `names`: rows the 1e-5-of-the-maximum bar cannot see."""
    vis = cond["cond_n"] > 0
    A = cond["cond_A"][:, :2].max(1)[vis]
    span = math.log10(A.max() / A.min())
    shares = {}
    for name in names:
        w = np.abs(np.asarray(want[name], np.float64)).reshape(vis.size, -1)
        shares[name] = float((w.max(1)[vis] < 1e-5 * w.max()).mean())
    print("%s: %d Gaussians with pairs, A_i over %.1f decades; share of rows below 1e-5 of the tensor maximum: %s"
          % (tag, vis.sum(), span, {k: round(v, 3) for k, v in shares.items()}))
    assert span >= decades, (tag, span)
    assert min(shares.values()) >= 0.25, (tag, shares)
    return vis


# ---------------------------------------------------------------------------------------------------------------------
# scenes: Gaussians placed in pixel units in front of the benchmark camera (as test_gpu_bwd_round_boundary._stack does)
# ---------------------------------------------------------------------------------------------------------------------
def _place(n, seed, u, v, zc, sigma_px, opacity, sh_degree=3):
    cloud, cam = helpers.cloud_and_camera(n, W, H, sh_degree=sh_degree, seed=seed)
    f = 500.0 * W / 512.0
    cloud.xyz = torch.stack([(u - (W - 1) / 2) * zc / f, (v - (H - 1) / 2) * zc / f, zc - 3.0], 1).float().contiguous()
    cloud.scales = (sigma_px * zc[:, None] / f).float().contiguous()
    cloud.opacity = opacity.reshape(n, 1).float().contiguous()
    return cloud, cam


def _uniform(g, n, lo, hi):
    return torch.empty(n, dtype=torch.float64).uniform_(lo, hi, generator=g)


@functools.lru_cache(maxsize=None)
def ladder(seed=3, n=300):
    """Opacities from 0.9 down to 1.5 / 255 and footprints from screen-filling (sigma 40 px) down to a tenth of a pixel,
    both geometric ladders, paired at random, all over the frame; the first six are large, near-opaque and bright (SH dc
    raised) and sit in the middle of the depth range: they set the tensor maxima and bury what lies behind them."""
    g = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, 1.0, n, dtype=torch.float64)
    opacity = (0.9 * (1.5 / 255 / 0.9) ** t)[torch.randperm(n, generator=g)]
    sig = (40.0 * (0.1 / 40.0) ** t)[torch.randperm(n, generator=g)]
    sig3 = sig[:, None] * _uniform(g, 3 * n, 0.7, 1.4).view(n, 3)
    u, v, zc = _uniform(g, n, -2.0, W + 1.0), _uniform(g, n, -2.0, H + 1.0), _uniform(g, n, 2.5, 3.5)
    k = 6
    opacity[:k] = _uniform(g, k, 0.8, 0.9)
    sig3[:k] = _uniform(g, 3 * k, 9.0, 16.0).view(k, 3)
    zc[:k] = _uniform(g, k, 2.55, 2.75)
    u[:k], v[:k] = _uniform(g, k, 8.0, 32.0), _uniform(g, k, 5.0, 19.0)
    cloud, cam = _place(n, seed, u, v, zc, sig3, opacity)
    cloud.shs[:k, 0] += 3.0
    return cloud, cam


@functools.lru_cache(maxsize=None)
def wall(seed=8, n_wall=24, n_back=100):
    """A stack of near-opaque Gaussians (opacity 0.85-0.95, sigma 5-9 px, centres spread over the frame) in front of 100
    ordinary ones: where k of the wall overlap, what lies behind is composited at T ~ 0.1^k -- 1e-2 to 1e-4 -- and where
    T (1 - alpha) falls below 1e-4 the pixel stops and the Gaussians behind get nothing from it."""
    g = torch.Generator().manual_seed(seed)
    n = n_wall + n_back
    opacity = torch.cat([_uniform(g, n_wall, 0.85, 0.95), _uniform(g, n_back, 0.05, 0.8)])
    sig3 = torch.cat([_uniform(g, 3 * n_wall, 9.0, 16.0).view(-1, 3), _uniform(g, 3 * n_back, 0.5, 5.0).view(-1, 3)])
    zc = torch.cat([_uniform(g, n_wall, 2.5, 2.7), _uniform(g, n_back, 2.9, 3.5)])
    u = torch.cat([_uniform(g, n_wall, 6.0, 34.0), _uniform(g, n_back, 0.0, W - 1.0)])
    v = torch.cat([_uniform(g, n_wall, 4.0, 20.0), _uniform(g, n_back, 0.0, H - 1.0)])
    return _place(n, seed, u, v, zc, sig3, opacity)


@functools.lru_cache(maxsize=None)
def edge(seed=5, n_out=90, n_last=40, n_front=12, n_rest=18):
    """Gaussians centred OUTSIDE the frame (2 to 12 sigma beyond a border) that reach in with their tails, Gaussians on the
    last partial tile (x 32-39, y 16-23), a dozen large near-opaque ones in front of them all, and a few ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    n = n_out + n_last + n_front + n_rest
    sig = torch.exp(_uniform(g, n, math.log(0.4), math.log(8.0)))
    sig3 = sig[:, None] * _uniform(g, 3 * n, 0.8, 1.25).view(n, 3)
    opacity = torch.exp(_uniform(g, n, math.log(0.01), math.log(0.9)))
    zc = _uniform(g, n, 2.5, 3.5)
    u, v = _uniform(g, n, 0.0, W - 1.0), _uniform(g, n, 0.0, H - 1.0)
    out = slice(0, n_out)  # outside: which border, how far
    side = torch.randint(0, 4, (n_out,), generator=g)
    far = sig[out] * _uniform(g, n_out, 2.0, 12.0)
    u[out] = torch.where(side == 0, -far, torch.where(side == 1, W - 1.0 + far, u[out]))
    v[out] = torch.where(side == 2, -far, torch.where(side == 3, H - 1.0 + far, v[out]))
    last = slice(n_out, n_out + n_last)
    u[last], v[last] = _uniform(g, n_last, 32.0, 39.5), _uniform(g, n_last, 16.0, 23.5)
    front = slice(n_out + n_last, n_out + n_last + n_front)  # the tails and the last tile are seen through T of 1e-1 to 1e-4
    opacity[front], zc[front] = _uniform(g, n_front, 0.8, 0.95), _uniform(g, n_front, 2.2, 2.4)
    sig3[front] = _uniform(g, 3 * n_front, 9.0, 16.0).view(n_front, 3)
    return _place(n, seed, u, v, zc, sig3, opacity)


@functools.lru_cache(maxsize=None)
def long_lists():
    """The frame of test_chunked_backward_full_chunks_and_last_chunks_ending_inside_a_round: lists of hundreds of entries, the
    backward in chunks from the forward's checkpoints."""
    from test_gpu_bwd_round_boundary import _stack
    return _stack(420, seed=9, opacity=(0.012, 0.02), small=140)


SCENES = {"ladder": ladder, "wall": wall, "edge": edge, "long": long_lists}
DECADES = {"ladder": 6.0, "wall": 6.0, "edge": 6.0, "long": 4.0}


def pixel_gradients(tag, second=False):
    """dL/dpix of the colour image of scene `tag` (and of a second image), seeded by the scene's name."""
    gen = torch.Generator().manual_seed(sum(map(ord, tag)) + (1000 if second else 0))
    return torch.randn(3, H, W, generator=gen) + torch.tensor([1.0, -1.0, 1.0])[:, None, None]
