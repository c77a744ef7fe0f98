"""Restatement of the rasterizer's antialiasing option (GsFwdArgs.antialiasing, include/gsplat_mi355.h) in torch on the
CPU, float64 by default: the effective opacity o' = o s and the gradient the option adds to the per-Gaussian backward.

It starts where the per-Gaussian preprocess starts: means, a 3-D covariance (six-vector, or
scale + RAW quaternion: the rasterizer does not normalise) and the camera.  Every line is an elementwise operation
written in the order of csrc/gs_math.h (cov3d_from_scale_rot, cov2d), so that `dtype=torch.float32` is the same
arithmetic rounded once per operation: the yardstick for what fp32 loses on a given cloud.

    Sigma' = (a0, b, c0) = (J Rv) Sigma (J Rv)^T,   a = a0 + 0.3,  c = c0 + 0.3
    det0 = a0 c0 - b^2,  det1 = a c - b^2,  r = det0 / det1
    s = sqrt(r) if r > 0.000025 else 0.005,   o' = o s

The gradient convention is the rasterizer's own (csrc/gaussian_bwd.hip): b is ONE parameter of the symmetric 2x2
matrix; the view-space point whose x/z (y/z) ratio is clamped at 1.3 tan(fov/2) is a constant in x (y) and passes no
gradient through that coordinate; scales receive the gradient of (scale_modifier * scale)."""
import numpy as np
import torch

DILATION = 0.3
R_MIN = 0.000025
S_MIN = 0.005


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x, np.float32)).to(dtype)


def cov6_from_scale_rot(sv, q):
    """strip_symmetric(L L^T), L = R(q) diag(sv): gs_math.h cov3d_from_scale_rot, operation for operation."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)],
         [2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)],
         [2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]]
    L = [[R[i][j] * sv[:, j] for j in range(3)] for i in range(3)]
    dot = lambda i, j: L[i][0] * L[j][0] + L[i][1] * L[j][1] + L[i][2] * L[j][2]
    return torch.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], 1)


def project(means, c6, view, W, H, tanfovx, tanfovy, scalar=np.float32):
    """(a0, b, c0): the EWA-projected 2-D covariance BEFORE the dilation (gs_math.h cov2d, operation for operation).
    `scalar`: the type the focal lengths and clamp limits are formed in (the kernel's: fp32; np.float64 for a comparison
    with oracle/dense_ref.py, which forms them in float64)."""
    dt = means.dtype
    V = view.to(dt)
    f32 = lambda v: float(scalar(v))  # the kernel's scalars are fp32 values
    fx = f32(scalar(W) / (scalar(2.0) * scalar(tanfovx)))
    fy = f32(scalar(H) / (scalar(2.0) * scalar(tanfovy)))
    limx, limy = f32(scalar(1.3) * scalar(tanfovx)), f32(scalar(1.3) * scalar(tanfovy))
    px, py, pz = means[:, 0], means[:, 1], means[:, 2]
    tx = V[0, 0] * px + V[1, 0] * py + V[2, 0] * pz + V[3, 0]
    ty = V[0, 1] * px + V[1, 1] * py + V[2, 1] * pz + V[3, 1]
    tz = V[0, 2] * px + V[1, 2] * py + V[2, 2] * pz + V[3, 2]
    txtz, tytz = (tx / tz).detach(), (ty / tz).detach()
    # value: clamp(t.x / t.z) * t.z as the kernel forms it; gradient: to t.x alone, and only inside the clamp
    inx = ((txtz >= -limx) & (txtz <= limx)).to(dt)
    iny = ((tytz >= -limy) & (tytz <= limy)).to(dt)
    txc = (txtz.clamp(-limx, limx) * tz.detach()) + (tx - tx.detach()) * inx
    tyc = (tytz.clamp(-limy, limy) * tz.detach()) + (ty - ty.detach()) * iny
    J00, J02 = fx / tz, -(fx * txc) / (tz * tz)
    J11, J12 = fy / tz, -(fy * tyc) / (tz * tz)
    M0 = [J00 * V[k, 0] + J02 * V[k, 2] for k in range(3)]
    M1 = [J11 * V[k, 1] + J12 * V[k, 2] for k in range(3)]
    S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
    MS0 = [M0[0] * S[0][j] + M0[1] * S[1][j] + M0[2] * S[2][j] for j in range(3)]
    MS1 = [M1[0] * S[0][j] + M1[1] * S[1][j] + M1[2] * S[2][j] for j in range(3)]
    a0 = MS0[0] * M0[0] + MS0[1] * M0[1] + MS0[2] * M0[2]
    b = MS0[0] * M1[0] + MS0[1] * M1[1] + MS0[2] * M1[2]
    c0 = MS1[0] * M1[0] + MS1[1] * M1[1] + MS1[2] * M1[2]
    return a0, b, c0


def scaling(a0, b, c0):
    """(s, r > R_MIN): the factor on the opacity and where it is not clamped."""
    a, c = a0 + DILATION, c0 + DILATION
    det0 = a0 * c0 - b * b
    det1 = a * c - b * b
    r = det0 / det1
    free = r > R_MIN
    s = torch.where(free, torch.sqrt(torch.where(free, r, torch.ones_like(r))), torch.full_like(r, S_MIN))
    return s, free


def added_terms(gO, o_eff, a0, b, c0):
    """The three terms the option adds to dL/da, dL/db, dL/dc of the per-Gaussian backward, as the header states them
    (gO = dL/do', o_eff = o'); zero where the clamp is active."""
    a, c = a0 + DILATION, c0 + DILATION
    det0 = a0 * c0 - b * b
    det1 = a * c - b * b
    free = (det0 / det1) > R_MIN
    d0 = torch.where(free, det0, torch.ones_like(det0))
    z = torch.zeros_like(a0)
    ga = torch.where(free, gO * o_eff * 0.5 * (c0 / d0 - c / det1), z)
    gc = torch.where(free, gO * o_eff * 0.5 * (a0 / d0 - a / det1), z)
    gb = torch.where(free, gO * o_eff * b * (1.0 / det1 - 1.0 / d0), z)
    return ga, gb, gc


class Scene(object):
    """The rows `rows` (those the device reports visible) of a cloud, as leaves of the given dtype."""

    def __init__(self, means, opacity, view, W, H, tanfovx, tanfovy, cov6=None, scales=None, rotations=None,
                 scale_modifier=1.0, rows=None, dtype=torch.float64, scalar=np.float32):
        n = np.asarray(means).shape[0]
        self.n, self.dtype = n, dtype
        self.rows = np.arange(n) if rows is None else np.flatnonzero(np.asarray(rows))
        pick = lambda x: _t(np.asarray(x, np.float32).reshape(n, -1)[self.rows], dtype)
        self.means = pick(means).requires_grad_(True)
        self.opacity = pick(opacity)[:, 0]
        self.cam = (_t(view, dtype).reshape(4, 4), int(W), int(H), float(tanfovx), float(tanfovy), scalar)
        if cov6 is not None:
            self.cov6, self.sv, self.rot = pick(cov6).requires_grad_(True), None, None
        else:
            self.cov6 = None
            self.sv = (pick(scales) * float(np.float32(scale_modifier))).requires_grad_(True)
            self.rot = pick(rotations).requires_grad_(True)

    def forward(self):
        c6 = self.cov6 if self.cov6 is not None else cov6_from_scale_rot(self.sv, self.rot)
        a0, b, c0 = project(self.means, c6, *self.cam)
        s, free = scaling(a0, b, c0)
        return dict(a0=a0, b=b, c0=c0, s=s, free=free, o_eff=self.opacity * s)

    def _full(self, x):
        out = np.zeros((self.n,) + tuple(x.shape[1:]), np.float64)
        out[self.rows] = x.detach().double().numpy()
        return out

    def effective_opacity(self):
        """(o', s, clamp inactive) for all n rows (zeros / False outside `rows`)."""
        with torch.no_grad():
            f = self.forward()
        return self._full(f["o_eff"]), self._full(f["s"]), self._full(f["free"].to(self.dtype)) > 0

    def chain(self, gO):
        """What the option adds to the gradients of means3D and of cov3D (or scales, rotations) given gO = dL/do' [n]:
        autograd of sum(gO o') through this file's own forward.  Full-size float64 arrays."""
        g = _t(np.asarray(gO, np.float32).reshape(self.n)[self.rows], self.dtype)
        leaves = [self.means] + ([self.cov6] if self.cov6 is not None else [self.sv, self.rot])
        grads = torch.autograd.grad((g * self.forward()["o_eff"]).sum(), leaves, allow_unused=True)
        grads = [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, grads)]
        names = ["means3D"] + (["cov3D"] if self.cov6 is not None else ["scales", "rotations"])
        return {k: self._full(v) for k, v in zip(names, grads)}
