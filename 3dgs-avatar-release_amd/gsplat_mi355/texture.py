"""The input of the ColorMLP texture (models/texture/texture.py ColorMLP.compose_input) on the GPU through
libgsplat_mi355 (csrc/texture.hip, whose header comment carries the spec): the (N, D) matrix the colour MLP reads --
pass-through blocks, the spherical-harmonics bases of the canonical view direction, more pass-through blocks and the
broadcast latent code -- composed by one forward launch and differentiated by one backward launch (the latent code adds
one small fixed-order sum): no atomics (bitwise reproducible), no host synchronisation, no host-to-device copy per call,
capture-safe.  The MLP behind it and its sigmoid stay torch modules.

* `color_mlp_input(before, xyz, camera_center, sh_degree, fwd_transform=None, view_noise=None, after=(), latent=None)`
  -> inp (N, D), one autograd node.
* `texture_forward(self, gaussians, camera, view_noise=None)` -- ColorMLP.forward ("The texture").
Device fp32 tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

MAX_D = _lib.GS_TEXTURE_MAX_D
MAX_BEFORE = _lib.GS_TEXTURE_MAX_BEFORE
MAX_AFTER = _lib.GS_TEXTURE_MAX_AFTER
LDS_FLOATS = 8192      # csrc/texture.hip: TX_LDS_FLOATS
FINAL_THREADS = 256    # csrc/texture.hip: TX_THREADS, the width of the latent gradient's final sum


def rows_per_block(D):
    """Rows a workgroup owns at width D (csrc/texture.hip: tx_rows)."""
    return min((LDS_FLOATS // D) & ~3, FINAL_THREADS)


def _f32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("%s: fp32 tensor expected" % name)
    return t


def _on_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (the fused HIP kernels have no CPU fallback)" % name)


def _args(n, D, deg, widths_before, widths_after, lt, noise):
    a = _lib.GsTextureArgs()
    a.N, a.D, a.sh_degree, a.latent_dim = n, D, deg, lt
    a.n_before, a.n_after = len(widths_before), len(widths_after)
    a.before_w[:len(widths_before)] = widths_before
    a.after_w[:len(widths_after)] = widths_after
    a.use_noise = 1 if noise is not None else 0
    if noise is not None:
        a.noise[:] = noise
    return a


def _direction(a, xyz, campos, rot):
    a.xyz, a.campos = _lib.ptr(xyz), _lib.ptr(campos)
    if rot is not None:
        a.fwd_transform, a.rot_stride, a.rot_row = _lib.ptr(rot), rot.stride(0), rot.stride(1)


def _rotation_in_place(fwd_transform):
    """The (N, 4, 4) or (N, 3, 3) forward transforms as the kernel reads their 3x3 corner: where they lie, unless the
    layout is not rows of adjacent floats."""
    rot = fwd_transform.detach()
    s0, s1, s2 = rot.stride()
    if s2 != 1 or s1 < 3 or s0 < 2 * s1 + 3 or s0 >= 2 ** 31:
        rot = rot.contiguous()
    return rot


class _Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, campos, latent, meta, *blocks):
        ctx.set_materialize_grads(False)
        deg, noise, n_before, fwd_transform = meta
        dev, n = xyz.device, int(xyz.shape[0])
        blocks = [_lib.contiguous_aligned(b.detach()) for b in blocks]  # (a non-contiguous block is copied once)
        widths = [int(b.shape[1]) for b in blocks]
        lt = int(latent.numel()) if latent is not None else 0
        D = sum(widths) + (deg + 1) ** 2 - 1 + lt
        inp = torch.empty(n, D, dtype=torch.float32, device=dev)
        xyz, campos = xyz.detach().contiguous(), campos.detach().contiguous()
        rot = _rotation_in_place(fwd_transform) if (fwd_transform is not None and deg > 0) else None
        if n > 0:
            a = _args(n, D, deg, widths[:n_before], widths[n_before:], lt, noise)
            for k, b in enumerate(blocks):
                if k < n_before:
                    a.before[k] = b.data_ptr()
                else:
                    a.after[k - n_before] = b.data_ptr()
            if lt:
                latent = latent.detach().contiguous()
                a.latent = _lib.ptr(latent)
            if deg > 0:
                _direction(a, xyz, campos, rot)
            with _lib.on_device(dev):
                _lib.check(_lib.load().gs_texture_input_forward(ctypes.byref(a), _lib.ptr(inp), _lib.stream_ptr(dev)))
        ctx.save_for_backward(*((xyz, campos, rot) if deg > 0 else (None, None, None)))
        ctx.meta = (n, D, deg, noise, n_before, widths, lt, tuple(latent.shape) if latent is not None else None)
        return inp

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        n, D, deg, noise, n_before, widths, lt, latent_shape = ctx.meta
        if g is None or not any(need):
            return (None,) * len(need)
        xyz, campos, rot = ctx.saved_tensors
        dev = g.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dblocks = [new(n, w) if nd else None for w, nd in zip(widths, need[4:])]
        dxyz = new(n, 3) if (need[0] and deg > 0) else None
        dlatent = new(*latent_shape) if (need[2] and lt > 0) else None
        if n == 0:
            if dlatent is not None:
                dlatent.zero_()
        elif dxyz is not None or dlatent is not None or any(d is not None for d in dblocks):
            g = _lib.contiguous_aligned(g.to(torch.float32))
            L = _lib.load()
            a = _args(n, D, deg, widths[:n_before], widths[n_before:], lt, noise)
            if dxyz is not None:
                _direction(a, xyz, campos, rot)
            ptrs = [d.data_ptr() if d is not None else None for d in dblocks]
            db = (ctypes.c_void_p * MAX_BEFORE)(*ptrs[:n_before])
            da = (ctypes.c_void_p * MAX_AFTER)(*ptrs[n_before:])
            ws = new(_lib.nbytes(L.gs_texture_workspace_bytes, n, D, lt) // 4) if dlatent is not None else None
            with _lib.on_device(dev):
                _lib.check(L.gs_texture_input_backward(ctypes.byref(a), _lib.ptr(g), db, da, _lib.ptr(dxyz), _lib.ptr(dlatent),
                                                       _lib.ptr(ws), 4 * ws.numel() if ws is not None else 0,
                                                       _lib.stream_ptr(dev)))
        return (dxyz, None, dlatent, None) + tuple(dblocks)


def _blocks(seq, n, what, limit):
    if torch.is_tensor(seq):
        seq = (seq,)
    seq = list(seq)
    if len(seq) > limit:
        raise ValueError("color_mlp_input: at most %d `%s` blocks, got %d" % (limit, what, len(seq)))
    out = []
    for k, b in enumerate(seq):
        name = "%s[%d]" % (what, k)
        _f32(b, name)
        w = 1
        for s in b.shape[1:]:
            w *= int(s)
        if b.dim() < 1 or int(b.shape[0]) != n or w < 1:
            raise ValueError("color_mlp_input: %s must have N = %d rows of at least one value, got %s" % (name, n, tuple(b.shape)))
        out.append(b.reshape(n, w))
    return out


def color_mlp_input(before, xyz, camera_center, sh_degree, fwd_transform=None, view_noise=None, after=(), latent=None):
    """The (N, D) input of the colour MLP as one autograd node, columns [before.. | sh_embed | after.. | latent]:
    `before` (at most 6) and `after` (at most 2) are sequences of tensors of N rows, each viewed as (N, w) and copied into
    place (`_features_dc` (N, 1, 1) and `_features_rest` (N, 31, 1) are passed as they are); sh_embed is
    eval_sh_bases(sh_degree, unit)[..., 1:] (sh_degree 0..4; no columns at 0) of unit = d / (|d| + 1e-12), d = xyz -
    camera_center, rotated by the transpose of the 3x3 of `fwd_transform` ((N, 4, 4), read in place, or (N, 3, 3); no
    gradient) when that is given and multiplied from the right by `view_noise` (a 3x3 on the host, already transposed as
    texture.py:30-33 does; it travels to the kernel by value) when that is given; `latent` ((Lt,) or (1, Lt)) is broadcast
    to every row.  D is at most GS_TEXTURE_MAX_D."""
    _f32(xyz, "xyz")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("color_mlp_input: xyz must be (N, 3), got %s" % (tuple(xyz.shape),))
    n, deg = int(xyz.shape[0]), int(sh_degree)
    if not 0 <= deg <= 4:
        raise ValueError("color_mlp_input: sh_degree in 0..4 expected, got %d" % deg)
    before, after = _blocks(before, n, "before", MAX_BEFORE), _blocks(after, n, "after", MAX_AFTER)
    _f32(camera_center, "camera_center")
    campos = camera_center.reshape(-1)
    if campos.numel() != 3:
        raise ValueError("color_mlp_input: camera_center must hold 3 values, got %s" % (tuple(camera_center.shape),))
    if latent is not None:
        _f32(latent, "latent")
        if latent.dim() not in (1, 2) or (latent.dim() == 2 and latent.shape[0] != 1):
            raise ValueError("color_mlp_input: latent must be (Lt,) or (1, Lt), got %s" % (tuple(latent.shape),))
        if latent.numel() == 0:
            latent = None
    if fwd_transform is not None:
        _f32(fwd_transform, "fwd_transform")
        if tuple(fwd_transform.shape) not in ((n, 4, 4), (n, 3, 3)):
            raise ValueError("color_mlp_input: fwd_transform must be (N, 4, 4) or (N, 3, 3) with N = %d, got %s"
                             % (n, tuple(fwd_transform.shape)))
    noise = None
    if view_noise is not None:
        noise = tuple(float(v) for v in torch.as_tensor(view_noise, dtype=torch.float32).reshape(-1).tolist())
        if len(noise) != 9:
            raise ValueError("color_mlp_input: view_noise must be 3x3")
    D = sum(int(b.shape[1]) for b in before + after) + (deg + 1) ** 2 - 1 + (int(latent.numel()) if latent is not None else 0)
    if not 1 <= D <= MAX_D:
        raise ValueError("color_mlp_input: the input is %d columns wide; 1..%d (GS_TEXTURE_MAX_D) are supported" % (D, MAX_D))
    for t, name in [(xyz, "xyz"), (camera_center, "camera_center"), (latent, "latent"), (fwd_transform, "fwd_transform")] + \
            [(b, "before[%d]" % k) for k, b in enumerate(before)] + [(b, "after[%d]" % k) for k, b in enumerate(after)]:
        if t is not None:
            _on_gpu(t, name)
    return _Compose.apply(xyz, campos, latent, (deg, noise, len(before), fwd_transform), *(before + after))


def _latent_row(self, camera, dev):
    """The module's latent code of the camera's frame, (1, Lt): the row index is a slice of a device tensor cached on the
    module (no host-to-device copy per step); an unknown frame takes the last row."""
    row = self.frame_dict.get(camera.frame_id, len(self.frame_dict) - 1)
    rows = self.__dict__.get("_gsplat_latent_rows")
    if rows is None or rows.device != dev or rows.numel() != self.latent.num_embeddings:
        rows = self.__dict__["_gsplat_latent_rows"] = torch.arange(self.latent.num_embeddings, dtype=torch.long, device=dev)
    return self.latent(rows[row:row + 1])


def texture_forward(self, gaussians, camera, view_noise=None):
    """ColorMLP.forward (models/texture/texture.py:121-125) with the fused input composition; `self.mlp` and
    `self.color_activation` stay in torch.  Reads self.cfg, metadata["aabb"], use_xyz, use_cov, use_normal, sh_degree,
    cano_view_dir, non_rigid_dim, latent_dim (with frame_dict and latent); gaussians._features_dc / _features_rest / get_xyz
    / fwd_transform / non_rigid_feature (and get_covariance(), _scaling, _rotation with the use_* flags);
    camera.camera_center / frame_id.  In training with cfg.view_noise > 0 and cano_view_dir the noise matrix is drawn by
    the reference's own utils.sh_utils.augm_rots unless `view_noise` (3x3, already transposed) is given; in eval mode, and
    without cano_view_dir, there is no noise."""
    xyz = gaussians.get_xyz
    before = [gaussians._features_dc, gaussians._features_rest]
    for name, b in zip(("_features_dc", "_features_rest"), before):
        if b.dim() != 3 or b.shape[2] != 1:
            raise ValueError("texture_forward: %s must be (N, w, 1), got %s" % (name, tuple(b.shape)))
    if self.use_xyz:
        before.append(self.metadata["aabb"].normalize(xyz, sym=True))
    if self.use_cov:
        before.append(gaussians.get_covariance())
    if self.use_normal:  # the rotation's column of the smallest scale
        from utils.general_utils import build_rotation  # the reference's own
        rot = build_rotation(gaussians._rotation)
        index = gaussians._scaling.argmin(1).reshape(-1, 1, 1).expand(-1, 3, 1)
        before.append(torch.gather(rot, dim=2, index=index).squeeze(-1))
    deg = int(self.sh_degree)
    fwd_transform = None
    if not (deg > 0 and self.cano_view_dir and self.training):
        view_noise = None  # (the reference applies noise in training and inside the cano_view_dir branch only)
    if deg > 0 and self.cano_view_dir:
        fwd_transform = gaussians.fwd_transform
        if view_noise is None and self.training and self.cfg.get('view_noise', 0.) > 0.:
            from utils.sh_utils import augm_rots  # the reference's own, and its numpy stream
            scale = self.cfg.get('view_noise', 0.)
            view_noise = torch.as_tensor(augm_rots(scale, scale, scale), dtype=torch.float32).transpose(0, 1)
    after = []
    if self.non_rigid_dim > 0:
        assert hasattr(gaussians, "non_rigid_feature")
        after.append(gaussians.non_rigid_feature)
    latent = _latent_row(self, camera, xyz.device) if self.latent_dim > 0 else None
    inp = color_mlp_input(before, xyz, camera.camera_center, deg, fwd_transform=fwd_transform, view_noise=view_noise,
                          after=after, latent=latent)
    return self.color_activation(self.mlp(inp))
