"""The argument handling of every entry point outside the frame path, pinned on the CPU: for each pointer argument and
pointer-valued struct field the answer to null, to address + 4, to address + 8 and to address + 2; the answer to a
workspace that is too small; and which error wins where two apply.  The codes were recorded from the library as it was
while all of these entry points still lived in capi.hip, on a machine without a device, and are compared as literals --
never recomputed from the library under test.

Only calls that the library answers BEFORE any launch are in the table (a validation code, or GS_OK from an early
return): on a machine without a device a call that reaches a launch answers GS_E_HIP, and a `.` marks the pointer cases
that do.  Device pointers are fake addresses that nothing may dereference, hence the module-level skip on a machine that
has a device.  (Pointers the HOST reads or writes -- the `out` of a size query, the host arrays of gs_hashgrid_levels,
the arrays of block gradients of gs_texture_input_backward -- are real buffers; gs_sh2rgb's host noise matrix is null.)"""
import ctypes
import os
import re

import pytest
import torch

import abi_header

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: host logic only, pinned without a device")

FAKE = 0x100000   # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 32     # "large enough" for every workspace of the small shapes below
GS_E_HIP = -4
DEV, HOST = "dev", "host"  # placeholders: a fake device address / a real 16-byte aligned host buffer
POINTER_CASES = (":0", "+4", "+8", "+2")  # null, and what tells a 16-byte, an 8-byte and a 4-byte rule from no rule
_PARENTS = [0] + list(range(23))


class St(object):
    """A struct argument: the _lib class by name and its fields (lists fill array fields from element 0)."""

    def __init__(self, cls, **fields):
        self.cls, self.fields = cls, fields


def _mlp():
    return St("GsMlpArgs", N=100, dim_in=8, dim_cond=4, width=32, n_hidden=2, dim_out=3, slope=0.01, x=DEV, cond=DEV, W=[DEV] * 3,
              b=[DEV] * 3, dW=[DEV] * 3, db=[DEV] * 3, dx=DEV, dcond=DEV)


def _lpips():
    return St("GsLpipsArgs", H=32, W=32, normalize=1, need_grad0=1, need_grad1=1, cs0=1024, rs0=32, cs1=1024, rs1=32, in0=DEV,
              in1=DEV, packed=DEV, weight=[DEV] * 13, bias=[DEV] * 13, lin=[DEV] * 5, shift=DEV, scale=DEV)


def _texture():  # D = 8 (degree 2) + 4 (latent) + 3 + 1
    return St("GsTextureArgs", N=100, D=16, sh_degree=2, n_before=1, n_after=1, before_w=[3], after_w=[1], latent_dim=4,
              rot_stride=16, rot_row=4, use_noise=0, before=[DEV], after=[DEV], xyz=DEV, campos=DEV, fwd_transform=DEV, latent=DEV)


def _pose():
    return St("GsPoseArgs", V=100, NB=10, parents=_PARENTS, v_template=DEV, shapedirs=DEV, J_template=DEV, J_shapedirs=DEV,
              betas=DEV, root_orient=DEV, pose_body=DEV, pose_hand=DEV, trans=DEV, rots_gt=DEV)


def _pose_enc():
    return St("GsPoseEncArgs", d=8, parents=_PARENTS, rots=DEV, Jtrs=DEV, W0=DEV, b0=DEV, W1=[DEV] * 24, b1=[DEV] * 24,
              W2=[DEV] * 24, b2=[DEV] * 24)


def _grid():
    return St("GsHashGrid", n_levels=4, n_features_per_level=2, log2_hashmap_size=10, base_resolution=4, per_level_scale=1.5)


def _aiap_sets():
    return [St("GsAiapSet", xc=DEV, xd=DEV, D=3, loss=DEV, dL_dloss=DEV, dL_dxc=DEV, dL_dxd=DEV)]


def _grad_tensors():
    return [St("GsGradTensor", grad=DEV, n=10)]


def _ptrs(*names):
    return [(n, DEV) for n in names]


_WS = [("workspace", DEV), ("workspace_bytes", BIG)]
_END = [("stream", None)]
_OUT = [("out", HOST)]

# entry point -> its baseline call: (argument name, value) in the order of the C signature; every check passes
BASELINES = {
    # knn.hip
    "knn_workspace_bytes": [("P", 100)] + _OUT,
    "knn_dist2": [("P", 100)] + _ptrs("points", "mean_d2") + _WS + _END,
    "knn_points": [("Nq", 10), ("queries", DEV), ("Nr", 10), ("ref", DEV), ("K", 3), ("dists", DEV), ("idx", DEV)] + _WS + _END,
    # prepass.hip
    "gs_build_covariance": [("N", 10), ("scaling", DEV), ("scaling_modifier", 1.0), ("rotation", DEV), ("rotation_is_matrix", 0),
                            ("cov6", DEV)] + _END,
    "gs_build_covariance_backward": [("N", 10), ("scaling", DEV), ("scaling_modifier", 1.0), ("rotation", DEV),
                                     ("rotation_is_matrix", 0)] + _ptrs("dL_dcov6", "dL_dscaling", "dL_drotation") + _END,
    "gs_sh2rgb": [("N", 10), ("sh_degree", 3), ("M", 16)] + _ptrs("shs", "xyz", "campos", "fwd_rotation") +
                 [("view_noise_host", None)] + _ptrs("colors", "clamped") + _END,
    "gs_sh2rgb_backward": [("N", 10), ("sh_degree", 3), ("M", 16)] + _ptrs("shs", "xyz", "campos", "fwd_rotation") +
                          [("view_noise_host", None)] + _ptrs("clamped", "dL_dcolors", "dL_dshs", "dL_dxyz") + _END,
    # loss.hip
    "gs_l1_loss_workspace_bytes": [("n", 1024)] + _OUT,
    "gs_l1_loss": [("n", 1024)] + _ptrs("x", "y", "loss", "dL_dx") + _WS + _END,
    "gs_bce_loss": [("n", 1024)] + _ptrs("x", "y", "loss", "dL_dx") + _WS + _END,
    "gs_ssim_workspace_bytes": [("C", 3), ("H", 64), ("W", 64)] + _OUT,
    "gs_ssim_forward": [("C", 3), ("H", 64), ("W", 64)] +
                       _ptrs("img1", "img2", "ssim_out", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12") + _WS + _END,
    "gs_ssim_backward": [("C", 3), ("H", 64), ("W", 64)] +
                        _ptrs("img1", "img2", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12", "dL_dssim", "dL_dimg1") + _END,
    # optim.hip
    "gs_densify_stats": [("N", 10)] + _ptrs("radii", "viewspace_grad", "max_radii2D", "xyz_gradient_accum", "denom") + _END,
    "gs_adam_step": [("n_tensors", 1), ("tensors", [St("GsAdamTensor", param=DEV, grad=DEV, exp_avg=DEV, exp_avg_sq=DEV, n=10,
                                                       lr=1e-3)]),
                     ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-15), ("step", 1)] + _END,
    "gs_grad_norm_workspace_bytes": [("n_tensors", 1), ("tensors", _grad_tensors())] + _OUT,
    "gs_grad_norm": [("n_tensors", 1), ("tensors", _grad_tensors()), ("max_norm", 1.0), ("out", DEV)] + _WS + _END,
    "gs_grad_scale": [("n_tensors", 1), ("tensors", _grad_tensors()), ("clip_coef", DEV)] + _END,
    "gs_adam_step_ex": [("n_tensors", 1),
                        ("tensors", [St("GsAdamTensorEx", param=DEV, grad=DEV, exp_avg=DEV, exp_avg_sq=DEV, n=10, lr=1e-3,
                                        weight_decay=0.0, step=DEV, lr_dev=DEV)]),
                        ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-15), ("step", 1), ("clip_coef", DEV)] + _END,
    # densify.hip
    "gs_densify_workspace_bytes": [("N", 100)] + _OUT,
    "gs_densify_plan": [("p", St("GsDensifyPlan", N=100, scaling=DEV, opacity=DEV, grad_accum=DEV, denom=DEV, prune_mask=DEV,
                                 grad_threshold=1e-4, split_scale=0.01, min_opacity=0.05, max_world_scale=1.0,
                                 max_screen_size=20.0, prune_size=1))] + _WS + [("count_host_pinned", DEV)] + _END,
    "gs_densify_apply": [("N", 100), ("N_new", 120)] + _WS +
                        [("n_tensors", 1), ("tensors", [St("GsDensifyTensor", src=DEV, dst=DEV, width=3, kind=3)])] +
                        _ptrs("scaling", "rotation", "noise") + _END,
    "gs_reset_opacity": [("N", 100)] + _ptrs("opacity_in", "opacity_out", "exp_avg", "exp_avg_sq") + _END,
    # aiap.hip
    "gs_aiap_workspace_bytes": [("N", 100), ("K", 4), ("n_sets", 1)] + _OUT,
    "gs_aiap_forward": [("N", 100), ("K", 4), ("idx", DEV), ("n_sets", 1), ("sets", _aiap_sets())] + _WS + _END,
    "gs_aiap_backward": [("N", 100), ("K", 4), ("idx", DEV), ("n_sets", 1), ("sets", _aiap_sets())] + _WS + _END,
    # hashgrid.hip
    "gs_hashgrid_levels": [("grid", _grid()), ("offsets", HOST), ("scales", HOST), ("resolutions", HOST), ("n_params", HOST)],
    "gs_hashgrid_workspace_bytes": [("grid", _grid()), ("N", 100)] + _OUT,
    "gs_hashgrid_forward": [("grid", _grid()), ("N", 100)] + _ptrs("x", "params", "out") + _END,
    "gs_hashgrid_backward": [("grid", _grid()), ("N", 100)] + _ptrs("x", "params", "dL_dout", "dL_dx", "dL_dparams") + _WS + _END,
    # skinning.hip
    "gs_skin_weights_forward": [("N", 100), ("kind", 0)] + _ptrs("logits", "weights") + _END,
    "gs_skin_weights_backward": [("N", 100), ("kind", 0)] + _ptrs("logits", "dL_dweights", "dL_dlogits") + _END,
    "gs_skinning_workspace_bytes": [("N", 100)] + _OUT,
    "gs_skinning_forward": [("N", 100), ("kind", 2)] +
                           _ptrs("w", "tfs", "xyz", "rotation", "xyz_out", "rotation_out", "T_fwd") + _END,
    "gs_skinning_backward": [("N", 100), ("kind", 2)] +
                            _ptrs("w", "tfs", "xyz", "rotation", "dL_dxyz_out", "dL_drotation_out", "dL_dw", "dL_dtfs", "dL_dxyz",
                                  "dL_drotation") + _WS + _END,
    # skinloss.hip
    "gs_mesh_sample": [("n", 10), ("V", 10), ("F", 10)] +
                      _ptrs("verts", "faces", "cdf", "vweights", "aabb_min", "aabb_inv_extent", "draws", "points_norm", "target",
                            "face", "bary", "points") + _END,
    "gs_skin_loss_workspace_bytes": [("n", 10)] + _OUT,
    "gs_skin_loss_forward": [("n", 10), ("kind", 0)] + _ptrs("logits", "target", "loss") + _WS + _END,
    "gs_skin_loss_backward": [("n", 10), ("kind", 0)] + _ptrs("logits", "target", "dL_dloss", "dL_dlogits") + _END,
    # pose.hip
    "gs_pose_workspace_bytes": [("V", 100)] + _OUT,
    "gs_pose_forward": [("a", _pose())] + _ptrs("rots", "Jtrs", "bone_transforms", "loss_pose", "state") + _WS + _END,
    "gs_pose_backward": [("a", _pose())] +
                        _ptrs("state", "dL_drots", "dL_dJtrs", "dL_dbone_transforms", "dL_dloss_pose", "dL_dbetas",
                              "dL_droot_orient", "dL_dpose_body", "dL_dpose_hand", "dL_dtrans") + _END,
    # nonrigid.hip
    "gs_pose_encoder_grad_floats": [("d", 8)] + _OUT,
    "gs_pose_encoder_forward": [("a", _pose_enc())] + _ptrs("out", "state") + _END,
    "gs_pose_encoder_backward": [("a", _pose_enc())] + _ptrs("state", "dL_dout", "dL_dparams", "dL_drots", "dL_dJtrs") + _END,
    "gs_nonrigid_workspace_bytes": [("N", 100), ("D", 12)] + _OUT,
    "gs_nonrigid_apply_forward": [("N", 100), ("D", 12), ("scale_offset", 0), ("rot_offset", 0)] +
                                 _ptrs("deltas", "xyz", "scaling", "rotation", "xyz_out", "scaling_out", "rotation_out", "feature",
                                       "losses") + _WS + _END,
    "gs_nonrigid_apply_backward": [("N", 100), ("D", 12), ("scale_offset", 0), ("rot_offset", 0)] +
                                  _ptrs("deltas", "scaling", "rotation", "dL_dxyz_out", "dL_dscaling_out", "dL_drotation_out",
                                        "dL_dfeature", "dL_dnr_xyz", "dL_dnr_scale", "dL_dnr_rot", "dL_ddeltas", "dL_dscaling",
                                        "dL_drotation") + _END,
    # texture.hip
    "gs_texture_workspace_bytes": [("N", 100), ("D", 16), ("latent_dim", 4)] + _OUT,
    "gs_texture_input_forward": [("a", _texture()), ("inp", DEV)] + _END,
    "gs_texture_input_backward": [("a", _texture()), ("dL_dinp", DEV), ("dL_dbefore", [DEV]), ("dL_dafter", [DEV]),
                                  ("dL_dxyz", DEV), ("dL_dlatent", DEV)] + _WS + _END,
    # mlp.hip
    "gs_mlp_workspace_bytes": [("a", _mlp()), ("backward", 1)] + _OUT,
    "gs_mlp_forward": [("a", _mlp()), ("y", DEV), ("acts", DEV)] + _WS + _END,
    "gs_mlp_backward": [("a", _mlp()), ("acts", DEV), ("dL_dy", DEV)] + _WS + _END,
    # lpips.hip
    "gs_lpips_packed_bytes": list(_OUT),
    "gs_lpips_pack_weights": [("a", _lpips()), ("packed", DEV), ("packed_bytes", BIG)] + _END,
    "gs_lpips_workspace_bytes": [("H", 32), ("W", 32), ("need_grad0", 1), ("need_grad1", 0), ("which", 0)] + _OUT,
    "gs_lpips_forward": [("a", _lpips()), ("loss", DEV), ("per_tap", DEV), ("saved", DEV), ("saved_bytes", BIG)] + _WS + _END,
    "gs_lpips_backward": [("a", _lpips()), ("dL_dloss", DEV), ("d_in0", DEV), ("d_in1", DEV), ("saved", DEV),
                          ("saved_bytes", BIG)] + _WS + _END,
    "gs_lpips_conv": [("packed", DEV), ("layer", 1), ("backward", 1), ("normalize", 0), ("H", 16), ("W", 16), ("in", DEV),
                      ("in_cs", 256), ("in_rs", 16), ("mask", DEV), ("out", DEV)] + _END,
    "gs_lpips_pool": [("backward", 1), ("H", 16), ("W", 16), ("C", 64)] + _ptrs("in", "g", "dp", "out") + _END,
}


# ---- a call: the baseline materialised (placeholders -> addresses), mutated, turned into ctypes arguments
class _Call(object):
    def __init__(self, lib, name):
        self.lib, self.name, self.keep = lib, name, []
        self.pointers = []  # the path of every pointer argument and pointer-valued struct field, in order
        self.args = [[n, self._plain(v, n)] for n, v in BASELINES[name]]

    def _host(self):
        buf = ctypes.create_string_buffer(1024 + 16)
        self.keep.append(buf)
        return (ctypes.addressof(buf) + 15) & ~15

    def _plain(self, v, path):
        if v == DEV or v == HOST:
            self.pointers.append(path)
            return FAKE if v == DEV else self._host()
        if isinstance(v, St):
            return {"cls": v.cls, "fields": {k: self._plain(x, path + "." + k) for k, x in v.fields.items()}}
        if isinstance(v, list):
            return [self._plain(x, "%s[%d]" % (path, i)) for i, x in enumerate(v)]
        return v

    def mutate(self, mut):
        """`path:value` sets, `path+offset` adds; a path is argument, argument.field, argument[i].field or ....field[i]."""
        m = re.match(r"^([\w.\[\]]+)([:+])(-?\w+)$", mut)
        assert m, mut
        keys = re.findall(r"\w+", m.group(1))
        node = next(slot for slot in self.args if slot[0] == keys[0])  # a [name, value] slot
        at = 1
        for k in keys[1:]:
            node, at = (node[at], int(k)) if k.isdigit() else (node[at]["fields"], k)
        node[at] = int(m.group(3), 0) if m.group(2) == ":" else node[at] + int(m.group(3), 0)

    def _struct(self, d):
        s = getattr(self.lib, d["cls"])()
        for k, v in d["fields"].items():
            if isinstance(v, list):
                arr = getattr(s, k)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(s, k, v)
        return s

    def __call__(self):
        fn = getattr(self.lib.load(), self.name)
        out = []
        for (_, v), argtype in zip(self.args, fn.argtypes):
            if isinstance(v, dict):
                self.keep.append(self._struct(v))
                v = ctypes.byref(self.keep[-1])
            elif isinstance(v, list) and v and isinstance(v[0], dict):
                arr = (getattr(self.lib, v[0]["cls"]) * len(v))(*[self._struct(d) for d in v])
                self.keep.append(arr)
                v = arr
            elif isinstance(v, list):
                self.keep.append((ctypes.c_void_p * len(v))(*v))
                v = self.keep[-1]
            elif isinstance(v, int) and issubclass(argtype, ctypes._Pointer):  # a typed pointer: an address, or null
                v = ctypes.cast(ctypes.c_void_p(v), argtype) if v else None
            out.append(v)
        assert len(out) == len(fn.argtypes), self.name
        return fn(*out)


def run_case(lib, name, case):
    """The status of entry point `name` with the `&`-joined mutations of `case` applied to its baseline."""
    call = _Call(lib, name)
    for mut in case.split("&"):
        call.mutate(mut)
    return call()


def pointer_paths(lib, name):
    return _Call(lib, name).pointers


def _expand(path):
    """`a.W[0..2]` -> a.W[0], a.W[1], a.W[2]"""
    m = re.match(r"^(.*)\[(\d+)\.\.(\d+)\]$", path)
    return ["%s[%d]" % (m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)] if m else [path]


def parse_line(line):
    """`path@a/b/c/d` -> the pointer cases of `path` (POINTER_CASES: null, + 4, + 8, + 2; `.`: the call reaches a launch, not
    pinned), `path[i..j]@...` those of every element; `mutation[&mutation...]=code` -> one case."""
    cases = []
    for item in line.split():
        if "@" in item:
            paths, codes = item.split("@")
            assert len(codes.split("/")) == len(POINTER_CASES), item
            for path in _expand(paths):
                cases += [(path + mut, int(code)) for mut, code in zip(POINTER_CASES, codes.split("/")) if code != "."]
        else:
            case, code = item.rsplit("=", 1)
            cases.append((case, int(code)))
    return cases


# RECORDED: see the module docstring.  One string per entry point; a pointer of the baseline without an `@` item is one
# whose four cases all reach a launch.
RECORDED = {
    "knn_workspace_bytes": "out@-1/0/0/0 P:-1=-1 P:-1&out:0=-1",
    "knn_dist2": (
        "points@-1/././. mean_d2@-1/././. workspace@-1/././. workspace_bytes:16=-5 P:0&points:0=0 "
        "P:-1&workspace_bytes:16=-1 points:0&workspace_bytes:16=-1"),
    "knn_points": (
        "queries@-1/././. ref@-1/././. dists@-1/././. idx@-1/././. workspace@-1/././. workspace_bytes:16=-5 "
        "Nq:0&queries:0=0 Nq:0&ref:0=-1 K:9&workspace_bytes:16=-1"),
    "gs_build_covariance": (
        "scaling@-1/././. rotation@-1/-1/-1/-1 cov6@-1/././. N:0&scaling:0=0 N:0&rotation+4=-1 scaling:0&rotation+4=-1"),
    "gs_build_covariance_backward": (
        "scaling@-1/././. rotation@-1/-1/-1/-1 dL_dcov6@-1/././. dL_dscaling@-1/././. dL_drotation@-1/-1/-1/-1 "
        "N:0&dL_drotation+4=-1 rotation+4&dL_dscaling:0=-1 N:-1&rotation+4=-1"),
    "gs_sh2rgb": (
        "shs@-1/././. xyz@-1/././. campos@-1/././. colors@-1/././. clamped@-1/././. N:0&shs:0=0 M:9&shs:0=-1 N:0&M:9=-1"),
    "gs_sh2rgb_backward": (
        "shs@-1/././. xyz@-1/././. campos@-1/././. clamped@-1/././. dL_dcolors@-1/././. dL_dshs@-1/././. dL_dxyz@-1/././. "
        "N:0&shs:0=0 M:17&dL_dshs:0=-1 N:0&sh_degree:4=-1"),
    "gs_l1_loss_workspace_bytes": "out@-1/0/0/0 n:-1=-1 n:-1&out:0=-1",
    "gs_l1_loss": (
        "x@-1/-1/-1/-1 y@-1/-1/-1/-1 loss@-1/././. dL_dx@-1/-1/-1/-1 workspace@-1/././. workspace_bytes:0=-5 n:0&x+4=-1 "
        "x+4&workspace_bytes:0=-1 x:0&y+4=-1"),
    "gs_bce_loss": (
        "x@-1/././. y@-1/././. loss@-1/././. dL_dx@-1/././. workspace@-1/././. workspace_bytes:0=-5 "
        "n:0&workspace_bytes:0=-1 x:0&workspace_bytes:0=-1"),
    "gs_ssim_workspace_bytes": "out@-1/0/0/0 W:0=-1 W:0&out:0=-1",
    "gs_ssim_forward": (
        "img1@-1/././. img2@-1/././. ssim_out@-1/././. dm_dmu1@-1/././. dm_dsigma1_sq@-1/././. dm_dsigma12@-1/././. "
        "workspace@-1/././. workspace_bytes:0=-5 dm_dmu1:0&workspace_bytes:0=-1 C:0&workspace_bytes:0=-1 "
        "dm_dmu1:0&dm_dsigma1_sq:0&dm_dsigma12:0&workspace_bytes:0=-5"),
    "gs_ssim_backward": (
        "img1@-1/././. img2@-1/././. dm_dmu1@-1/././. dm_dsigma1_sq@-1/././. dm_dsigma12@-1/././. dL_dssim@-1/././. "
        "dL_dimg1@-1/././. C:0&img1:0=-1 img1:0&img2:0=-1"),
    "gs_densify_stats": (
        "radii@-1/././. viewspace_grad@-1/././. max_radii2D@-1/././. xyz_gradient_accum@-1/././. denom@-1/././. "
        "N:0&radii:0=0 N:-1&radii:0=-1"),
    "gs_adam_step": (
        "tensors[0].param@-1/././. tensors[0].grad@-1/././. tensors[0].exp_avg@-1/././. tensors[0].exp_avg_sq@-1/././. "
        "step:0=-1 n_tensors:17=-1 n_tensors:0&tensors:0=0 n_tensors:0&step:0=-1 tensors[0].n:-1=-1 "
        "tensors[0].n:0&tensors[0].param:0=0"),
    "gs_grad_norm_workspace_bytes": (
        "tensors[0].grad@-1/0/0/0 out@-1/0/0/0 tensors[0].n:0x20000000000=-3 out:0&tensors[0].n:0x20000000000=-1 "
        "n_tensors:0&tensors:0=0 tensors[0].n:0x20000000000&tensors[0].grad:0=-1"),
    "gs_grad_norm": (
        "tensors[0].grad@-1/././. out@-1/././. workspace@-1/././. workspace_bytes:0=-5 "
        "tensors[0].n:0x20000000000&workspace_bytes:0=-3 out:0&tensors[0].n:0x20000000000=-1 n_tensors:0&tensors:0=0 "
        "max_norm:-1=-1 tensors[0].grad:0&workspace_bytes:0=-1"),
    "gs_grad_scale": (
        "tensors[0].grad@-1/././. clip_coef@-1/././. n_tensors:0&clip_coef:0=-1 "
        "tensors[0].n:0x20000000000&tensors[0].grad:0=-1 n_tensors:0&tensors:0=0"),
    "gs_adam_step_ex": (
        "tensors[0].param@-1/././. tensors[0].grad@-1/././. tensors[0].exp_avg@-1/././. tensors[0].exp_avg_sq@-1/././. "
        "tensors[0].step:0&step:0=-1 tensors[0].n:0x20000000000=-3 tensors[0].n:0x20000000000&tensors[0].param:0=-1 "
        "n_tensors:0&tensors:0=0 n_tensors:4097=-1"),
    "gs_densify_workspace_bytes": "out@-1/0/0/0 N:0x40000000=-1 N:-1&out:0=-1",
    "gs_densify_plan": (
        "workspace@-1/././. workspace_bytes:16=-5 p.N:-1&workspace_bytes:16=-1 p.prune_mask:0&p.scaling:0=-1 "
        "p.prune_mask:0&p.scaling:0&workspace_bytes:16=-1 p:0=-1"),
    "gs_densify_apply": (
        "workspace@-1/././. tensors[0].src@-1/././. tensors[0].dst@-1/././. scaling@-1/././. rotation@-1/././. "
        "noise@-1/././. workspace_bytes:16=-5 N_new:201&workspace_bytes:16=-1 workspace_bytes:16&tensors[0].width:0=-5 "
        "N_new:0&tensors[0].dst:0=0 tensors[0].kind:5=-1 n_tensors:0&tensors:0=0 tensors[0].width:4=-1"),
    "gs_reset_opacity": "opacity_in@-1/././. opacity_out@-1/././. N:0&opacity_in:0=0 N:-1&opacity_in:0=-1",
    "gs_aiap_workspace_bytes": "out@-1/0/0/0 K:9=-1 N:0=-1 K:9&out:0=-1",
    "gs_aiap_forward": (
        "idx@-1/././. sets[0].xc@-1/././. sets[0].xd@-1/././. sets[0].loss@-1/././. workspace@-1/././. "
        "workspace_bytes:16=-5 K:9&workspace_bytes:16=-1 idx:0&workspace_bytes:16=-1 sets[0].D:4=-1 "
        "sets[0].D:4&workspace_bytes:16=-1 n_sets:3&sets:0=-1"),
    "gs_aiap_backward": (
        "idx@-1/././. sets[0].xc@-1/././. sets[0].xd@-1/././. workspace@-1/././. workspace_bytes:16=-5 "
        "K:9&workspace_bytes:16=-1 idx:0&workspace_bytes:16=-1 sets[0].D:4=-1 sets[0].D:4&workspace_bytes:16=-1 "
        "n_sets:3&sets:0=-1"),
    "gs_hashgrid_levels": (
        "offsets@0/0/0/0 scales@0/0/0/0 resolutions@0/0/0/0 n_params@0/0/0/0 grid.n_levels:0=-1 "
        "grid.n_levels:33&offsets:0=-1 grid.log2_hashmap_size:31=-1 grid:0=-1"),
    "gs_hashgrid_workspace_bytes": "out@-1/0/0/0 N:-1=-1 N:0x7fffffff=-3 grid.n_features_per_level:3&N:0x7fffffff=-1",
    "gs_hashgrid_forward": (
        "x@-1/././-1 params@-1/-1/./-1 out@0/-1/./-1 N:0&x:0=0 out:0&x:0=0 grid.n_levels:0&x:0=-1 x:0&params+4=-1 "
        "N:0x7fffffff&x:0=-3"),
    "gs_hashgrid_backward": (
        "x@-1/././-1 params@-1/-1/./-1 dL_dout@-1/-1/./-1 dL_dx@./././-1 dL_dparams@./-1/./-1 workspace@-1/././. "
        "workspace_bytes:16=-5 dL_dparams:0&dL_dx:0&x:0=0 x:0&workspace_bytes:16=-1 params+4&workspace:0=-1 "
        "N:0x7fffffff&x:0=-3 N:0&dL_dparams:0&x+4=0"),
    "gs_skin_weights_forward": (
        "logits@-1/-1/-1/-1 weights@-1/-1/-1/-1 N:0&logits:0=0 kind:2&logits:0=-1 kind:2&N:0=-1 logits:0&weights+4=-1"),
    "gs_skin_weights_backward": (
        "logits@-1/-1/-1/-1 dL_dweights@-1/-1/-1/-1 dL_dlogits@-1/-1/-1/-1 N:0&logits:0=0 kind:2&logits:0=-1 "
        "kind:2&N:0=-1 logits:0&dL_dlogits+4=-1"),
    "gs_skinning_workspace_bytes": "out@-1/0/0/0 N:-1=-1 N:-1&out:0=-1",
    "gs_skinning_forward": (
        "w@-1/-1/-1/-1 tfs@-1/-1/-1/-1 xyz@-1/././-1 rotation@-1/-1/-1/-1 xyz_out@-1/-1/-1/-1 rotation_out@-1/-1/-1/-1 "
        "T_fwd@-1/-1/-1/-1 N:0&w:0=0 kind:3&w:0=-1 w:0&tfs+4=-1 xyz+2&w+4=-1"),
    "gs_skinning_backward": (
        "w@-1/-1/-1/-1 tfs@-1/-1/-1/-1 xyz@-1/././-1 rotation@-1/-1/-1/-1 dL_dxyz_out@./././-1 dL_drotation_out@./././-1 "
        "dL_dw@./-1/-1/-1 dL_dtfs@./././-1 dL_dxyz@./././-1 dL_drotation@./-1/-1/-1 workspace@-1/-1/-1/-1 "
        "workspace_bytes:16=-5 w+4&workspace_bytes:16=-1 dL_dw:0&dL_dtfs:0&dL_dxyz:0&dL_drotation:0=0 "
        "dL_dw:0&dL_dtfs:0&dL_dxyz:0&dL_drotation:0&dL_dxyz_out+2=-1 N:0&w:0=0 workspace:0&workspace_bytes:16=-1"),
    "gs_mesh_sample": (
        "verts@-1/././-1 faces@-1/././-1 cdf@-1/././-1 vweights@-1/-1/-1/-1 aabb_min@-1/././-1 aabb_inv_extent@-1/././-1 "
        "draws@-1/././-1 points_norm@-1/-1/-1/-1 target@-1/-1/-1/-1 face@./././-1 bary@./-1/-1/-1 points@./-1/-1/-1 "
        "n:0&draws:0=0 n:0&verts:0=-1 V:0&verts:0=-1 verts:0&faces+2=-1 draws:0&points_norm+4=-1"),
    "gs_skin_loss_workspace_bytes": "out@-1/0/0/0 n:-1=-1 n:-1&out:0=-1",
    "gs_skin_loss_forward": (
        "logits@-1/-1/-1/-1 target@-1/-1/-1/-1 loss@-1/././-1 workspace@-1/-1/-1/-1 workspace_bytes:0=-5 "
        "kind:2&workspace_bytes:0=-1 n:0&logits:0=0 logits+4&workspace_bytes:0=-1 loss+2=-1"),
    "gs_skin_loss_backward": (
        "logits@-1/-1/-1/-1 target@-1/-1/-1/-1 dL_dloss@-1/././-1 dL_dlogits@-1/-1/-1/-1 n:0&logits:0=0 kind:2&n:0=-1 "
        "logits:0&target+4=-1"),
    "gs_pose_workspace_bytes": "out@-1/0/0/0 V:0=-1 V:0&out:0=-1",
    "gs_pose_forward": (
        "a.v_template@-1/././-1 a.shapedirs@-1/././-1 a.J_template@-1/././-1 a.J_shapedirs@-1/././-1 a.betas@-1/././-1 "
        "a.root_orient@-1/././-1 a.pose_body@-1/././-1 a.pose_hand@-1/././-1 a.trans@-1/././-1 a.rots_gt@./././-1 "
        "rots@-1/././-1 Jtrs@-1/././-1 bone_transforms@-1/././-1 loss_pose@-1/././-1 state@-1/././-1 workspace@-1/-1/./-1 "
        "workspace_bytes:0=-5 a.V:0&workspace_bytes:0=-1 rots:0&workspace_bytes:0=-1 a.parents[3]:3&a.J_shapedirs:0=-1 "
        "a:0=-1 workspace+4&workspace_bytes:0=-1"),
    "gs_pose_backward": (
        "a.J_shapedirs@-1/././-1 a.root_orient@-1/././-1 a.pose_body@-1/././-1 a.pose_hand@-1/././-1 a.rots_gt@./././-1 "
        "state@-1/././-1 dL_drots@./././-1 dL_dJtrs@./././-1 dL_dbone_transforms@./././-1 dL_dloss_pose@./././-1 "
        "dL_dbetas@./././-1 dL_droot_orient@./././-1 dL_dpose_body@./././-1 dL_dpose_hand@./././-1 dL_dtrans@./././-1 "
        "a.NB:17&state:0=-1 dL_dbetas:0&dL_droot_orient:0&dL_dpose_body:0&dL_dpose_hand:0&dL_dtrans:0=0 "
        "dL_dbetas:0&dL_droot_orient:0&dL_dpose_body:0&dL_dpose_hand:0&dL_dtrans:0&state:0=-1 "
        "dL_dbetas:0&dL_droot_orient:0&dL_dpose_body:0&dL_dpose_hand:0&dL_dtrans:0&dL_drots+2=-1"),
    "gs_pose_encoder_grad_floats": "out@-1/0/0/0 d:0=-1 d:17=-1 d:17&out:0=-1",
    "gs_pose_encoder_forward": (
        "a.rots@-1/././-1 a.Jtrs@-1/././-1 a.W0@-1/././-1 a.b0@-1/././-1 a.W1[0..23]@-1/././-1 a.b1[0..23]@-1/././-1 "
        "a.W2[0..23]@-1/././-1 a.b2[0..23]@-1/././-1 out@-1/././-1 state@-1/././-1 a.d:0&out:0=-1 a.W0:0&out+4=-1 "
        "a.parents[5]:5=-1 a:0=-1"),
    "gs_pose_encoder_backward": (
        "a.W0@-1/././-1 a.W1[0..23]@-1/././-1 a.W2[0..23]@-1/././-1 state@-1/././-1 dL_dout@-1/././-1 dL_dparams@./././-1 "
        "dL_drots@./././-1 dL_dJtrs@./././-1 dL_dparams:0&dL_drots:0&dL_dJtrs:0=0 "
        "dL_dparams:0&dL_drots:0&dL_dJtrs:0&state:0=-1 a.d:17&state:0=-1"),
    "gs_nonrigid_workspace_bytes": "out@-1/0/0/0 D:9=-1 N:-1=-1 D:2049&out:0=-1",
    "gs_nonrigid_apply_forward": (
        "deltas@-1/-1/-1/-1 xyz@-1/././-1 scaling@-1/././-1 rotation@-1/-1/-1/-1 xyz_out@-1/././-1 scaling_out@-1/././-1 "
        "rotation_out@-1/-1/-1/-1 feature@-1/-1/-1/-1 losses@./././-1 workspace@-1/././-1 workspace_bytes:0=-5 "
        "D:9&workspace_bytes:0=-1 N:0&deltas:0=0 deltas+4&workspace_bytes:0=-1 scaling:0&scaling_out:0=-1 "
        "scale_offset:2&scaling:0=-1 workspace:0&workspace_bytes:0=-1"),
    "gs_nonrigid_apply_backward": (
        "deltas@-1/-1/-1/-1 scaling@./././-1 rotation@./-1/-1/-1 dL_dxyz_out@./././-1 dL_dscaling_out@./././-1 "
        "dL_drotation_out@./-1/-1/-1 dL_dfeature@./-1/-1/-1 dL_dnr_xyz@./././-1 dL_dnr_scale@./././-1 dL_dnr_rot@./././-1 "
        "dL_ddeltas@./-1/-1/-1 dL_dscaling@./././-1 dL_drotation@./-1/-1/-1 N:0&deltas:0=0 D:9&deltas:0=-1 "
        "dL_ddeltas:0&dL_dscaling:0&dL_drotation:0=0 dL_ddeltas:0&dL_dscaling:0&dL_drotation:0&deltas+4=-1 "
        "scale_offset:1&scaling:0=-1"),
    "gs_texture_workspace_bytes": "out@-1/0/0/0 latent_dim:17=-1 D:0=-1 D:513&out:0=-1",
    "gs_texture_input_forward": (
        "a.before[0]@-1/-1/-1/-1 a.after[0]@-1/-1/-1/-1 a.xyz@-1/././-1 a.campos@-1/././-1 a.fwd_transform@./././-1 "
        "a.latent@-1/././-1 inp@-1/-1/-1/-1 a.N:0&inp:0=0 a.D:17&inp:0=-1 inp:0&a.before[0]+4=-1 a.rot_row:2=-1 a:0=-1"),
    "gs_texture_input_backward": (
        "a.xyz@-1/././-1 a.campos@-1/././-1 a.fwd_transform@./././-1 dL_dinp@-1/-1/-1/-1 dL_dbefore[0]@./-1/-1/-1 "
        "dL_dafter[0]@./-1/-1/-1 dL_dxyz@./././-1 dL_dlatent@./././-1 workspace@-1/././-1 workspace_bytes:0=-5 "
        "a.D:17&workspace_bytes:0=-1 dL_dinp+4&workspace_bytes:0=-1 dL_dbefore:0&dL_dafter:0&dL_dxyz:0&dL_dlatent:0=0 "
        "a.N:0&dL_dinp:0=0 a.latent_dim:0&a.D:12=-1 workspace:0&workspace_bytes:0=-1"),
    "gs_mlp_workspace_bytes": (
        "a.x@0/0/0/0 a.cond@0/0/0/0 a.W[0..2]@0/0/0/0 a.b[0..2]@0/0/0/0 a.dW[0..2]@0/0/0/0 a.db[0..2]@0/0/0/0 "
        "a.dx@0/0/0/0 a.dcond@0/0/0/0 out@-1/0/0/0 a.width:33=-1 a:0=-1 out:0&a.width:33=-1"),
    "gs_mlp_forward": (
        "a.x@-1/-1/-1/-1 a.cond@-1/././-1 a.W[0..2]@-1/././-1 a.b[0..2]@-1/././-1 y@-1/././-1 acts@./-1/-1/-1 "
        "workspace@-1/././-1 workspace_bytes:0=-5 a.width:33&workspace_bytes:0=-1 a.N:0&a.x:0=0 y:0&workspace_bytes:0=-1 "
        "a.x+4&workspace_bytes:0=-1"),
    "gs_mlp_backward": (
        "a.x@-1/-1/-1/-1 a.cond@-1/././-1 a.W[0..2]@-1/././-1 a.b[0..2]@-1/././-1 a.dW[0..2]@./././-1 a.db[0..2]@./././-1 "
        "a.dx@./././-1 a.dcond@./././-1 acts@-1/-1/-1/-1 dL_dy@-1/-1/-1/-1 workspace@-1/-1/-1/-1 workspace_bytes:0=-5 "
        "a.N:0&acts:0=0 acts:0&workspace_bytes:0=-1 a.dim_cond:0=-1 a.dW[0]+2&workspace_bytes:0=-1 "
        "a.dx:0&a.dcond:0&a.dW[0]:0&a.dW[1]:0&a.dW[2]:0&a.db[0]:0&a.db[1]:0&a.db[2]:0&workspace:0=0 "
        "a.dx:0&a.dcond:0&a.dW[0]:0&a.dW[1]:0&a.dW[2]:0&a.db[0]:0&a.db[1]:0&a.db[2]:0&dL_dy+4=-1"),
    "gs_lpips_packed_bytes": "out@-1/0/0/0",
    "gs_lpips_pack_weights": (
        "a.weight[0..12]@-1/././-1 a.bias[0..12]@-1/././-1 a.lin[0..4]@-1/././-1 a.shift@./././-1 a.scale@./././-1 "
        "packed@-1/-1/-1/-1 packed_bytes:16=-5 packed:0&packed_bytes:16=-1 a.lin[4]:0&packed_bytes:16=-1 a:0=-1"),
    "gs_lpips_workspace_bytes": "out@-1/0/0/0 H:15=-1 which:3=-1 W:2049=-1 H:15&out:0=-1",
    "gs_lpips_forward": (
        "a.in0@-1/././-1 a.in1@-1/././-1 a.packed@-1/-1/-1/-1 loss@-1/././-1 per_tap@./././-1 saved@-1/-1/-1/-1 "
        "workspace@-1/-1/-1/-1 workspace_bytes:16=-5 saved_bytes:16=-5 saved_bytes:16&workspace_bytes:16=-5 "
        "a.H:15&workspace_bytes:16=-1 loss:0&workspace_bytes:16=-1 a.rs0:31=-1 saved+4&saved_bytes:16=-1"),
    "gs_lpips_backward": (
        "a.in0@-1/././-1 a.in1@-1/././-1 a.packed@-1/-1/-1/-1 dL_dloss@./././-1 d_in0@./././-1 d_in1@./././-1 "
        "saved@-1/-1/-1/-1 workspace@-1/-1/-1/-1 workspace_bytes:16=-5 saved_bytes:16=-5 d_in0:0&d_in1:0&saved:0=0 "
        "a.need_grad1:0=-1 d_in0:0&d_in1:0&dL_dloss+2=-1 saved:0&workspace_bytes:16=-1"),
    "gs_lpips_conv": (
        "packed@-1/-1/-1/-1 in@-1/-1/-1/-1 mask@-1/-1/-1/-1 out@-1/-1/-1/-1 layer:13&packed:0=-1 "
        "layer:0&backward:0&in_rs:15=-1 mask:0&out+4=-1 H:0&in:0=-1"),
    "gs_lpips_pool": "in@-1/-1/-1/-1 g@-1/-1/-1/-1 dp@-1/-1/-1/-1 out@-1/-1/-1/-1 C:6&in:0=-1 g:0&dp+4=-1 C:516=-1",
}


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


def test_every_entry_point_outside_the_frame_path_is_pinned(lib):
    frame_path = {"gs_geom_bytes", "gs_image_bytes", "gs_image_bytes_for", "gs_binning_bytes", "gs_backward_scratch_bytes",
                  "gs_forward_preprocess", "gs_forward_render", "gs_forward", "gs_forward_shared", "gs_opacity_image", "gs_backward",
                  "gs_backward_with_opacity", "gs_backward_with_second", "gs_mark_visible", "gs_pair_stats", "gs_geom_field",
                  "gs_binning_field", "gs_image_field", "gs_clock_probe", "gs_xcc_probe", "gs_tuning", "gs_status_string",
                  "gs_last_hip_error", "gs_last_stage", "gs_build_info", "gs_profile_enable", "gs_profile_reserve",
                  "gs_profile_filter", "gs_profile_collect"}
    assert set(BASELINES) == set(lib.EXPORTS) - frame_path
    assert set(RECORDED) == set(BASELINES)
    for name, line in RECORDED.items():
        cases = parse_line(line)
        assert cases, name
        assert GS_E_HIP not in [code for _, code in cases], name
        # the pointer items name pointers of the baseline, in its order; every entry point with a workspace has a small one
        listed = [p for item in line.split() if "@" in item for p in _expand(item.split("@")[0])]
        assert listed == [p for p in pointer_paths(lib, name) if p in listed], name
        if "workspace_bytes" in dict(BASELINES[name]):
            assert any(case.startswith("workspace_bytes:") for case, _ in cases), name


def test_entry_points_outside_the_frame_path_answer_bad_arguments_as_before(lib):
    got, want = {}, {}
    for name, line in RECORDED.items():
        want[name] = parse_line(line)
        got[name] = [(case, run_case(lib, name, case)) for case, _ in want[name]]
    for name in want:
        assert got[name] == want[name], name
