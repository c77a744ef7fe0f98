"""The C calls diff_gaussian_rasterization makes, call by call: what "the wrapper's behaviour" means.

A recording proxy stands in for the loaded library (helpers._CallCounter, subclassed) while one tiny scene -- 300 Gaussians
on a 64 x 48 image, twelve tiles -- goes through every form of the frame path: eager (first frame of a shape, second
frame), the reference's two-call step (fused second backward and not), with_opacity, with_invdepth (gradient used and
unused), l1_target, no_grad, and a training step captured into a graph.  Each case's sequence of calls is compared with
the table below, which was recorded before the wrapper's forward was split into its three forms and has to survive every
later change of the Python side untouched.

One line per call: `name(arg, arg, ...)`.
* A pointer argument is `p` (given) or `0` (NULL).
* A count or size argument is its value, written as the quantity it has to be: P; D, the frame's pair count; CAP =
  _capacity_for(D), the speculative capacity of a following frame; CCAP, the fixed capacity of a captured frame; GEOM, IMG,
  BIN(x), SCR(x) = the library's own size queries for them.  (So the table holds in both binning modes.)  The size
  queries themselves are memoised by the wrapper and not part of the sequence.
* The GsFwdArgs block is shown as it is AT THE MOMENT of the call -- it is reused and mutated between forward and backward
  and copied for the inverse-depth render: ll = long_lists, fo = forward_only, aa = antialiasing, M, then the NULL-ness of
  shs, cp = colors_precomp, fs = frame_stats, l1t / l1l / l1g = l1_target / l1_loss / l1_grad.
* A GsSecondImage is shown with its long_lists and the NULL-ness of dL_dcolors (dc)."""
import ctypes
import gc
import math

import pytest
import torch

import helpers
from helpers import _CallCounter

pytestmark = pytest.mark.gpu

N, W, H = 300, 64, 48

_FWD = "{ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=p l1t=0 l1l=0 l1g=0}"
_FWD_NO_FS = "{ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=0 l1t=0 l1l=0 l1g=0}"
_ONES = "{ll=0 fo=0 aa=0 M=0 shs=0 cp=p fs=p l1t=0 l1l=0 l1g=0}"
_INVZ = "{ll=0 fo=0 aa=0 M=0 shs=0 cp=p fs=0 l1t=0 l1l=0 l1g=0}"

TABLE = {
    # no estimate of the pair count: gs_forward is given no binning state, reports the count, and phase 2 runs again
    "eager-first": [
        "gs_forward(%s, p, GEOM, 0, 0, 0, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_forward_render(%s, p, GEOM, p, BIN(D), p, IMG, D, p, 0)" % _FWD,
        "gs_backward(%s, p, p, GEOM, p, BIN(D), p, IMG, D, p, p, p, SCR(D), p, 0)" % _FWD,
    ],
    "eager-second": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_backward(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, SCR(CAP), p, 0)" % _FWD,
    ],
    "two-call-fused": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_forward_shared(%s, p, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, 0)" % _ONES,
        "gs_backward_with_second(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p{ll=0 dc=0}, p, SCR(CAP), p, 0)" % _FWD,
    ],
    "two-call-apart": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_forward_shared(%s, p, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, 0)" % _ONES,
        "gs_backward(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, SCR(CAP), p, 0)" % _ONES,
        "gs_backward(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, SCR(CAP), p, 0)" % _FWD,
    ],
    "with-opacity": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_opacity_image(%s, p, IMG, p, 0)" % _FWD,
        "gs_backward_with_opacity(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, p, SCR(CAP), p, 0)" % _FWD,
    ],
    "invdepth-used": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_geom_field(p, P, 0, p)",
        "gs_forward_shared(%s, p, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, 0)" % _INVZ,
        "gs_geom_field(p, P, 5, p)",
        "gs_backward_with_second(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p{ll=0 dc=p}, p, SCR(CAP), p, 0)" % _FWD,
    ],
    "invdepth-unused": [
        "gs_forward(%s, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)" % _FWD,
        "gs_geom_field(p, P, 0, p)",
        "gs_forward_shared(%s, p, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, 0)" % _INVZ,
        "gs_geom_field(p, P, 5, p)",
        "gs_backward(%s, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, SCR(CAP), p, 0)" % _FWD,
    ],
    # the loss alone is differentiated: no gradient image (dL_dpix NULL), its gradient is formed inside the backward
    "l1-target": [
        "gs_forward({ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=p l1t=p l1l=p l1g=0}, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)",
        "gs_backward({ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=p l1t=p l1l=0 l1g=p}, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, 0, p, "
        "SCR(CAP), p, 0)",
    ],
    "l1-target-and-colour": [
        "gs_forward({ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=p l1t=p l1l=p l1g=0}, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)",
        "gs_backward({ll=0 fo=0 aa=0 M=16 shs=p cp=0 fs=p l1t=p l1l=0 l1g=p}, p, p, GEOM, p, BIN(CAP), p, IMG, CAP, p, p, p, "
        "SCR(CAP), p, 0)",
    ],
    "no-grad": [
        "gs_forward({ll=0 fo=1 aa=0 M=16 shs=p cp=0 fs=p l1t=0 l1l=0 l1g=0}, p, GEOM, p, BIN(CAP), CAP, p, IMG, p, p, p, p, 0)",
    ],
    # on the capturing side stream (a stream handle, not NULL); the replay makes no call
    "captured": [
        "gs_forward_preprocess(%s, p, GEOM, p, IMG, p, 0, p)" % _FWD_NO_FS,
        "gs_forward_render(%s, p, GEOM, p, BIN(CCAP), p, IMG, CCAP, p, p)" % _FWD_NO_FS,
        "gs_geom_field(p, P, 5, p)",
        "gs_backward(%s, p, p, GEOM, p, BIN(CCAP), p, IMG, CCAP, p, p, p, SCR(CCAP), p, p)" % _FWD_NO_FS,
    ],
}

_VALUE_TYPES = (ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int)


def _null(v):
    if isinstance(v, ctypes.c_void_p):
        v = v.value
    return "0" if not v else "p"


class _CallRecorder(_CallCounter):
    """_CallCounter that also writes every call down (module docstring), size queries excepted.  `names`: {value: what to
    call it}, applied when the lines are read (the first frame runs before the pair count is known)."""

    def __init__(self, lib):
        super().__init__(lib)
        self.noted, self.names = [], {}

    def _struct(self, s):
        from gsplat_mi355 import _lib
        if isinstance(s, _lib.GsFwdArgs):
            return "{ll=%d fo=%d aa=%d M=%d shs=%s cp=%s fs=%s l1t=%s l1l=%s l1g=%s}" % (
                s.long_lists, s.forward_only, s.antialiasing, s.M, _null(s.shs), _null(s.colors_precomp), _null(s.frame_stats),
                _null(s.l1_target), _null(s.l1_loss), _null(s.l1_grad))
        if isinstance(s, _lib.GsSecondImage):
            return "p{ll=%d dc=%s}" % (s.long_lists, _null(s.dL_dcolors))
        return "p"

    def _note(self, name, args):
        super()._note(name, args)
        if "_bytes" in name:
            return
        types = getattr(self._lib, name).argtypes or [None] * len(args)
        assert len(types) == len(args), name
        out = []
        for t, v in zip(types, args):
            if t in _VALUE_TYPES:
                out.append(int(v))
            elif hasattr(v, "_obj"):  # ctypes.byref(...)
                out.append(self._struct(v._obj))
            else:
                out.append(_null(v))
        self.noted.append((name, out))

    def take(self):
        noted, self.noted = self.noted, []
        return noted

    def lines(self, noted):
        return ["%s(%s)" % (name, ", ".join(v if isinstance(v, str) else self.names.get(v, str(v)) for v in args))
                for name, args in noted]


def _record_all():
    """Runs every case once; returns ({case: [line]}, {fact: value})."""
    import diff_gaussian_rasterization as dgr
    from gsplat_mi355 import _lib
    assert dgr._SHARE and dgr._FUSE_SECOND and dgr._SPECULATE and dgr._LONG_LISTS == "0"  # the defaults are under test
    dev = torch.device("cuda:0")
    cloud, cam = helpers.cloud_and_camera(N, W, H, sh_degree=3, seed=2)
    settings = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
        projmatrix=cam.full_proj_transform.to(dev), sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False,
        debug=False)
    rast = dgr.GaussianRasterizer(settings)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    ones = torch.ones(N, 3, device=dev)

    def leaves():
        kw = dict(means3D=cloud.xyz.to(dev), means2D=torch.zeros(N, 3, device=dev), opacities=cloud.opacity.to(dev),
                  scales=cloud.scales.to(dev), rotations=cloud.rotations.to(dev), shs=cloud.shs.to(dev))
        for t in kw.values():
            t.requires_grad_(True)
        return kw

    def step(**extra):
        color = rast(**leaves(), **extra)[0]
        color.sum().backward()

    def two_call():
        kw = leaves()
        c1 = rast(**kw)[0]
        kw.pop("shs")
        c2 = rast(colors_precomp=ones, **kw)[0]
        (c1.sum() + c2[:1].sum()).backward()

    L = _lib.load()
    rec = _CallRecorder(L)
    key = (0, N, W, H)
    saved_count, saved_fuse, gc_was_on = dgr._last_count.get(key), dgr._FUSE_SECOND, gc.isenabled()
    got, facts = {}, {}
    _lib._lib = rec
    try:
        def case(name, fn):
            dgr.release_shared_geometry()
            rec.take()
            fn()
            torch.cuda.synchronize()
            got[name] = rec.take()

        dgr._last_count.pop(key, None)
        case("eager-first", step)
        D = dgr._last_count[key]
        CAP = dgr._capacity_for(D)
        CCAP = dgr._capacity_for(max(int(D * (1.0 + dgr._CAPTURE_SLACK)), 1024))
        a = dgr._make_args(settings, cloud.xyz.to(dev), cloud.shs.to(dev), None, cloud.opacity.to(dev), cloud.scales.to(dev),
                           cloud.rotations.to(dev), None, [])
        named = [(N, "P"), (D, "D"), (CAP, "CAP"), (CCAP, "CCAP"), (_lib.nbytes(L.gs_geom_bytes, N), "GEOM"),
                 (_lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a)), "IMG")]
        for x, s in ((D, "D"), (CAP, "CAP"), (CCAP, "CCAP")):
            named += [(_lib.nbytes(L.gs_binning_bytes, x, W, H), "BIN(%s)" % s),
                      (_lib.nbytes(L.gs_backward_scratch_bytes, x, N, W, H), "SCR(%s)" % s)]
        rec.names = dict(named)
        facts["pairs"], facts["sizes are distinct"] = D, len(rec.names) == len(named) and min(rec.names) > 16
        case("eager-second", step)
        hits0 = dgr._geom_cache.hits
        case("two-call-fused", two_call)
        facts["hits of the two-call step"] = dgr._geom_cache.hits - hits0
        dgr._FUSE_SECOND = False
        try:
            case("two-call-apart", two_call)
        finally:
            dgr._FUSE_SECOND = saved_fuse

        def opacity():
            color, _, opa = rast(with_opacity=True, **leaves())
            (color.sum() + opa.sum()).backward()
        case("with-opacity", opacity)

        def invdepth(used):
            color, _, inv = rast(with_invdepth=True, **leaves())
            (color.sum() + inv.sum() if used else color.sum()).backward()
        case("invdepth-used", lambda: invdepth(True))
        case("invdepth-unused", lambda: invdepth(False))

        def l1(with_colour):
            color, _, loss = rast(l1_target=gt, **leaves())
            (loss + color.sum() if with_colour else loss).backward()
        case("l1-target", lambda: l1(False))
        case("l1-target-and-colour", lambda: l1(True))

        def no_grad():
            with torch.no_grad():
                rast(**leaves())
        case("no-grad", no_grad)

        # the offer is owned by the producing call's autograd node alone: it dies with the call's outputs, by reference
        # counting, without a backward and without the cycle collector
        dgr.release_shared_geometry()
        gc.disable()
        try:
            out = rast(**leaves())
            ref = dgr._geom_cache.offer[0]
            facts["offer alive while the outputs are"] = ref() is not None
            del out
            facts["offer dead once they are dropped"] = ref() is None
        finally:
            if gc_was_on:
                gc.enable()

        # a training step captured after eager ones, as tests/test_gpu_capture.py shapes it: fresh leaves, warmed up on the
        # side stream, captured there, replayed once
        kw = leaves()

        def train():
            for t in kw.values():
                t.grad = None
            dgr.release_shared_geometry()
            rast(**kw)[0].sum().backward()
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                train()
        side.synchronize()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        dgr.captured_forwards(clear=True)

        def capture():
            with torch.cuda.graph(graph, stream=side):
                train()
            graph.replay()
        case("captured", capture)
        (cnt, capacity), = dgr.captured_forwards(clear=True)
        facts["captured frame"] = (int(cnt.item()), capacity == CCAP)
    finally:
        _lib._lib = L
        dgr._FUSE_SECOND = saved_fuse
        dgr.release_shared_geometry()
        dgr.captured_forwards(clear=True)
        if saved_count is None:
            dgr._last_count.pop(key, None)
        else:
            dgr._last_count[key] = saved_count
    return {name: rec.lines(noted) for name, noted in got.items()}, facts


@pytest.fixture(scope="module")
def recorded(oracle):
    got, facts = _record_all()
    for name, lines in got.items():
        print(name)
        for ln in lines:
            print("   ", ln)
    print(facts)
    return got, facts


def test_every_case_is_in_the_table(recorded):
    assert set(recorded[0]) == set(TABLE)


@pytest.mark.parametrize("case", sorted(TABLE))
def test_the_sequence_of_c_calls(recorded, case):
    assert recorded[0][case] == TABLE[case]


def test_the_two_call_step_is_served_once_from_the_first_calls_geometry(recorded):
    assert recorded[1]["hits of the two-call step"] == 1


def test_the_offer_dies_with_the_calls_outputs_without_the_cycle_collector(recorded):
    facts = recorded[1]
    assert facts["offer alive while the outputs are"] and facts["offer dead once they are dropped"]


def test_the_scene_has_pairs_and_its_sizes_tell_apart(recorded):
    facts = recorded[1]
    assert facts["pairs"] > 0 and facts["sizes are distinct"]
    assert facts["captured frame"] == (facts["pairs"], True)
