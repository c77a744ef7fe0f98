"""C-ABI library on the CPU (no GPU needed): the binding gsplat_mi355/_lib.py states what include/gsplat_mi355.h declares --
every function's arguments, every struct's fields and layout, every constant -- the library loads and exports all of it,
and its size functions and argument validation run without touching a device."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_header
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return abi_header.lib()


@pytest.fixture(scope="module")
def header():
    return abi_header.parse()


# ---- the binding (gsplat_mi355/_lib.py: SIGNATURES, the Structure classes, the GS_* constants) against the header, whole
_INT_CODES = {"b": True, "h": True, "i": True, "l": True, "q": True, "B": False, "H": False, "I": False, "L": False, "Q": False}
C_SCALARS = {  # what the header's scalar types are on the one ABI the library is built for (LP64): (kind, bytes, signed)
    "int32_t": ("int", 4, True), "int64_t": ("int", 8, True), "uint8_t": ("int", 1, False), "uint32_t": ("int", 4, False),
    "uint64_t": ("int", 8, False), "size_t": ("int", 8, False), "int": ("int", 4, True), "float": ("float", 4, None),
    "double": ("float", 8, None), "char": ("int", 1, True)}


def _scalar(ct):
    """(kind, bytes, signed) of a ctypes scalar, None for anything else (pointers, c_void_p and c_char_p included)."""
    code = getattr(ct, "_type_", None) if isinstance(ct, type) and issubclass(ct, ctypes._SimpleCData) else None
    if code in ("f", "d"):
        return ("float", ctypes.sizeof(ct), None)
    if code in _INT_CODES:
        return ("int", ctypes.sizeof(ct), _INT_CODES[code])
    return None


def abi_mismatch(ct, t, length=None):
    """None when the ctypes type `ct` is ABI-equivalent to the header's type `t` (an array of `length` of them when that is
    not None), else what differs."""
    if length is not None or (isinstance(ct, type) and issubclass(ct, ctypes.Array)):
        if not (isinstance(ct, type) and issubclass(ct, ctypes.Array)) or length is None:
            return "array in one, not in the other"
        if ct._length_ != length:
            return "%d elements, the header has %d" % (ct._length_, length)
        return abi_mismatch(ct._type_, t)
    if t.depth == 0:
        if t.base not in C_SCALARS:
            return "a %s by value" % t.base
        if _scalar(ct) == C_SCALARS[t.base]:
            return None
        return "%s is %r, %s is %r" % (getattr(ct, "__name__", ct), _scalar(ct), t.base, C_SCALARS[t.base])
    is_pointer = isinstance(ct, type) and issubclass(ct, ctypes._Pointer)
    if t.depth == 2:
        want = ctypes.c_char_p if (t.base, t.const) == ("char", True) else ctypes.c_void_p
        return None if is_pointer and ct._type_ is want else "pointer to pointer: POINTER(%s) expected" % want.__name__
    if t.depth != 1:
        return "pointer depth %d" % t.depth
    if ct is ctypes.c_char_p:
        return None if (t.base, t.const) == ("char", True) else "c_char_p for %s*" % t.base
    if t.base not in C_SCALARS and t.base != "void":  # a struct: by POINTER of the class of that name, never a bare c_void_p
        ok = is_pointer and issubclass(ct._type_, ctypes.Structure) and ct._type_.__name__ == t.base
        return None if ok else "POINTER(%s) expected" % t.base
    if ct is ctypes.c_void_p:
        return None
    if not is_pointer:
        return "%s for a pointer" % getattr(ct, "__name__", ct)
    if t.base == "void" or _scalar(ct._type_) is None:
        return "POINTER(%s) for %s*" % (ct._type_.__name__, t.base)
    return None if _scalar(ct._type_)[:2] == C_SCALARS[t.base][:2] else "pointee %r, the header's is %r" % (
        _scalar(ct._type_), C_SCALARS[t.base])


def _structures(lib):
    return {n: c for n, c in vars(lib).items()
            if isinstance(c, type) and issubclass(c, ctypes.Structure) and c.__module__ == lib.__name__}


def test_the_scalar_table_is_this_platform_s():
    for name, ct in (("int32_t", ctypes.c_int32), ("int64_t", ctypes.c_int64), ("uint8_t", ctypes.c_uint8),
                     ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64), ("size_t", ctypes.c_size_t), ("int", ctypes.c_int),
                     ("float", ctypes.c_float), ("double", ctypes.c_double), ("char", ctypes.c_byte)):
        assert _scalar(ct) == C_SCALARS[name], name
    assert set(C_SCALARS) == set(abi_header.SCALARS)
    assert _scalar(ctypes.c_void_p) is None and _scalar(ctypes.c_char_p) is None


def test_every_function_is_bound_as_the_header_declares_it(lib, header):
    raw = abi_header.text()
    declared = re.findall(r"^(?:int|const char\*)\s+((?:gs|knn)_\w+)\s*\(", raw, flags=re.M)  # an independent line count
    assert len(declared) == len(set(declared)) == len(header.functions) >= 90
    assert set(declared) == set(header.functions)
    assert set(lib.SIGNATURES) == set(header.functions)
    assert lib.EXPORTS == list(lib.SIGNATURES) == list(header.functions)  # (the header's order)
    wrong = []
    for name, fn in header.functions.items():
        restype, argtypes = lib.SIGNATURES[name]
        want = {("int", False, 0): ctypes.c_int, ("char", True, 1): ctypes.c_char_p}[tuple(fn.restype)]
        if restype is not want:
            wrong.append("%s: restype %s" % (name, restype))
        if len(argtypes) != len(fn.params):
            wrong.append("%s: %d arguments bound, %d declared" % (name, len(argtypes), len(fn.params)))
            continue
        for ct, (pname, t) in zip(argtypes, fn.params):
            why = abi_mismatch(ct, t)
            if why:
                wrong.append("%s(%s): %s" % (name, pname, why))
    assert wrong == []
    L = lib.load()  # load() applies the table: every symbol is there, with the table's types
    for name, (restype, argtypes) in lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_every_struct_is_bound_as_the_header_declares_it(lib, header):
    classes = _structures(lib)
    assert len(header.structs) == abi_header.text().count("typedef struct") >= 15
    assert set(classes) == set(header.structs)
    wrong = []
    for name, fields in header.structs.items():
        bound = classes[name]._fields_
        if [f[0] for f in bound] != [f.name for f in fields]:
            wrong.append("%s: fields %s, the header has %s" % (name, [f[0] for f in bound], [f.name for f in fields]))
            continue
        for (fname, ct), f in zip(bound, fields):
            why = abi_mismatch(ct, f.type, f.length)
            if why:
                wrong.append("%s.%s: %s" % (name, fname, why))
    assert wrong == []


CONSTANTS_NOT_IN_THE_HEADER = {"GS_COUNT_NOT_ONES"}  # mirrors csrc/common.h: tests/test_invdepth_host.py holds it


def test_every_constant_of_the_binding_is_the_header_s(lib, header):
    bound = {n: v for n, v in vars(lib).items() if n.startswith("GS_") and isinstance(v, int)}
    assert CONSTANTS_NOT_IN_THE_HEADER <= set(bound)
    wrong = {n: (v, header.constants.get(n)) for n, v in bound.items()
             if n not in CONSTANTS_NOT_IN_THE_HEADER and header.constants.get(n) != v}
    assert wrong == {}
    for n in ("GS_OK", "GS_E_BAD_ARG", "GS_E_EXCLUSIVE", "GS_E_TOO_LARGE", "GS_E_HIP", "GS_E_WORKSPACE", "GS_E_CAPTURE"):
        assert n in bound, n
    # the field numbers of the introspection calls are ABI: all of the header's enums are bound, at these values
    fields = [n for n in header.constants if re.match(r"GS_(GEOM|BIN|IMG)_", n)]
    assert len(fields) == 6 + 2 + 6 + 3 and set(fields) <= set(bound)  # fields + the three counts
    assert (lib.GS_GEOM_FIELDS, lib.GS_BIN_FIELDS, lib.GS_IMG_FIELDS) == (6, 2, 6)
    assert (lib.GS_GEOM_COUNT, lib.GS_IMG_ORDER) == (5, 5)
    assert (lib.GS_OK, lib.GS_E_BAD_ARG, lib.GS_E_EXCLUSIVE, lib.GS_E_TOO_LARGE, lib.GS_E_HIP) == (0, -1, -2, -3, -4)


def test_struct_layouts_are_the_compiler_s(lib, header, tmp_path):
    """The reader and ctypes could share a wrong idea of padding: a host program that includes the header prints sizeof of
    every struct and offsetof of every field, and ctypes must say the same."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gsplat_mi355.h"', "int main() {"]
    for name, fields in header.structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f.name, name, f.name))
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines))
    cc = abi_header.build_module().hipcc()
    r = subprocess.run([cc, "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    want = {}
    for name, cls in _structures(lib).items():
        want[name] = ctypes.sizeof(cls)
        for fname, _ in cls._fields_:
            want["%s.%s" % (name, fname)] = getattr(cls, fname).offset
    assert got == want
    assert (got["GsFwdArgs"], got["GsFwdArgs.antialiasing"]) == (184, 180)


def test_the_integration_guide_shows_the_binding_s_frame_arguments(lib):
    """INTEGRATION.md's GsFwdArgs snippet: the same ("name", c_type) pairs in the same order as the binding's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = doc.index("class GsFwdArgs(ctypes.Structure)")
    snippet = doc[start:doc.index("\n\n", start)]
    pairs = re.findall(r'\("(\w+)",\s*(c_\w+)\)', snippet)
    assert [(n, getattr(ctypes, t)) for n, t in pairs] == list(lib.GsFwdArgs._fields_)


def test_size_functions_and_status_strings(lib):
    L = lib.load()
    g1, g2 = lib.nbytes(L.gs_geom_bytes, 1000), lib.nbytes(L.gs_geom_bytes, 200000)
    assert 0 < g1 < g2 and g2 >= 200000 * 48
    assert lib.nbytes(L.gs_image_bytes, 1024, 1024) >= 1024 * 1024 * 12
    b = lib.nbytes(L.gs_binning_bytes, 5_000_000, 1024, 1024)
    assert b >= 5_000_000 * (4 + 16 + 16)  # list entry, quadrant-list entries, the four row marks of a pair
    s = lib.nbytes(L.gs_backward_scratch_bytes, 5_000_000, 200000, 1024, 1024)
    assert s >= 5_000_000 * 4 * 32  # eight fp32 sums per (pair, quadrant) row (the ninth is the row's mark word: binning state)
    assert lib.nbytes(L.knn_workspace_bytes, 50000) > 50000 * 16
    for code in (0, -1, -2, -3, -4, -5, -6):
        assert len(L.gs_status_string(code)) > 0
    out = ctypes.c_size_t(0)
    assert L.gs_binning_bytes(1 << 30, 64, 64, ctypes.byref(out)) == -3  # GS_E_TOO_LARGE
    assert L.gs_geom_bytes(-1, ctypes.byref(out)) == -1                    # GS_E_BAD_ARG
    assert b"gfx950" in L.gs_build_info()


def test_image_state_size_follows_the_long_lists_flag(lib):
    """GsFwdArgs.long_lists: the checkpoints of the chunked backward are part of the image state on images of up to 2048
    tiles whatever the flag says, on larger ones only with the flag (gs_image_bytes_for); gs_image_bytes = flag 0."""
    L = lib.load()
    a = lib.GsFwdArgs()
    for (W, H), always in (((512, 512), True), ((1024, 1024), False)):
        a.W, a.H = W, H
        a.long_lists = 0
        plain = lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a))
        assert plain == lib.nbytes(L.gs_image_bytes, W, H)
        a.long_lists = 1
        flagged = lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a))
        tiles = (W // 16) * (H // 16)
        if always:
            assert flagged == plain >= tiles * 4 * 7 * 64 * 16
        else:
            assert flagged >= plain + tiles * 4 * 7 * 64 * 16


def test_image_state_size_does_not_depend_on_the_forward_switch(lib):
    """The image state's layout is a function of (W, H, long_lists, "small_tiles") alone: whichever forward "fwd4" selects,
    gs_image_bytes_for returns what the library returned at its default switches before the chunk-parallel forward (whose
    state was part of the image state while it was switched on) left."""
    L = lib.load()
    a = lib.GsFwdArgs()
    want = {(64, 64, 0): 1041920, (512, 512, 0): 66633984, (1024, 1024, 0): 13369600, (1024, 1024, 1): 266010880,
            (17, 33, 0): 380160}
    try:
        for fwd4 in (0, 1):
            lib.tuning("fwd4", fwd4)
            for (W, H, long_lists), nbytes in want.items():
                a.W, a.H, a.long_lists = W, H, long_lists
                assert lib.nbytes(L.gs_image_bytes_for, ctypes.byref(a)) == nbytes, (fwd4, W, H, long_lists)
    finally:
        lib.tuning("fwd4", helpers.process_fwd4())


def test_argument_validation_without_a_device(lib):
    """Exclusivity / null checks are done on the host before any HIP call."""
    L = lib.load()
    a = lib.GsFwdArgs()
    a.P, a.W, a.H, a.sh_degree, a.M = 10, 64, 64, 0, 1
    fake = 0x1000  # never dereferenced: validation fails first
    a.bg = a.viewmatrix = a.projmatrix = a.campos = a.means3D = a.opacities = fake
    a.shs = fake
    a.colors_precomp = fake  # both colour inputs -> GS_E_EXCLUSIVE
    a.scales = a.rotations = fake
    rc = L.gs_forward_preprocess(ctypes.byref(a), fake, 1 << 30, fake, 1 << 30, fake, None, None)
    assert rc == -2
    a.colors_precomp = None
    a.cov3D_precomp = fake  # both covariance inputs
    assert L.gs_forward_preprocess(ctypes.byref(a), fake, 1 << 30, fake, 1 << 30, fake, None, None) == -2
    a.cov3D_precomp = None
    a.sh_degree = 3  # M too small for the degree
    assert L.gs_forward_preprocess(ctypes.byref(a), fake, 1 << 30, fake, 1 << 30, fake, None, None) == -1
    a.sh_degree = 0
    a.M = 17  # more SH coefficients than degree 3 has: the backward's LDS tile is sized for M <= 16
    assert L.gs_forward_preprocess(ctypes.byref(a), fake, 1 << 30, fake, 1 << 30, fake, None, None) == -1
    a.M = 1
    a.rotations = fake + 4  # quaternions are read as float4
    assert L.gs_forward_preprocess(ctypes.byref(a), fake, 1 << 30, fake, 1 << 30, fake, None, None) == -1
    a.rotations = fake
    assert L.gs_forward_preprocess(ctypes.byref(a), fake, 16, fake, 1 << 30, fake, None, None) == -5  # workspace too small
    with pytest.raises(RuntimeError, match="exactly one of"):
        lib.check(-2)


def test_neighbouring_entry_points_validate_on_the_host(lib):
    """The N2-N4 entry points (losses, pre-pass, knn_points, optimiser) reject bad arguments before any HIP call."""
    L = lib.load()
    fake = 0x1000  # 16-byte aligned, never dereferenced
    out = ctypes.c_size_t(0)
    assert L.gs_l1_loss_workspace_bytes(1024 * 1024 * 3, ctypes.byref(out)) == 0 and out.value >= 4
    assert L.gs_l1_loss(0, fake, fake, fake, fake, fake, 1 << 20, None) == -1          # n must be positive
    assert L.gs_l1_loss(16, fake + 4, fake, fake, fake, fake, 1 << 20, None) == -1     # float4 alignment
    assert L.gs_l1_loss(1 << 24, fake, fake, fake, fake, fake, 4, None) == -5          # workspace too small
    assert L.gs_ssim_workspace_bytes(3, 64, 0, ctypes.byref(out)) == -1
    assert L.gs_ssim_forward(3, 64, 64, fake, fake, fake, fake, None, None, fake, 1 << 20, None) == -1  # maps: all or none
    assert L.gs_ssim_forward(3, 64, 64, fake, fake, fake, None, None, None, fake, 4, None) == -5
    assert L.gs_ssim_backward(3, 64, 64, fake, fake, fake, fake, fake, None, fake, None) == -1
    assert L.gs_build_covariance(10, fake, 1.0, fake + 4, 0, fake, None) == -1          # quaternions read as float4
    assert L.gs_build_covariance(-1, fake, 1.0, fake, 1, fake, None) == -1
    assert L.gs_sh2rgb(10, 3, 9, fake, fake, fake, None, None, fake, fake, None) == -1  # degree 3 needs 16 coefficients
    assert L.gs_sh2rgb(10, 4, 16, fake, fake, fake, None, None, fake, fake, None) == -1
    assert L.knn_points(10, fake, 10, fake, 9, fake, fake, fake, 1 << 20, None) == -1   # K <= 8
    assert L.knn_points(10, fake, 0, fake, 1, fake, fake, fake, 1 << 20, None) == -1    # empty reference set
    t = (lib.GsAdamTensor * 1)(lib.GsAdamTensor(fake, fake, None, fake, 10, 1e-3))
    assert L.gs_adam_step(1, t, 0.9, 0.999, 1e-15, 1, None) == -1                      # missing state tensor
    t[0].exp_avg = fake
    assert L.gs_adam_step(1, t, 0.9, 0.999, 1e-15, 0, None) == -1                      # step numbers start at 1
    assert L.gs_adam_step(17, t, 0.9, 0.999, 1e-15, 1, None) == -1                     # more than GS_ADAM_MAX_TENSORS
    assert L.gs_densify_stats(5, None, fake, fake, fake, fake, None) == -1
    # empty inputs are fine and touch nothing
    assert L.gs_build_covariance(0, None, 1.0, None, 0, None, None) == 0
    assert L.gs_adam_step(0, None, 0.9, 0.999, 1e-15, 1, None) == 0
    assert L.gs_densify_stats(0, None, None, None, None, None, None) == 0


def test_inference_context_offers_what_the_forward_uses_of_an_autograd_context():
    """Under no_grad the wrapper calls the forward with a plain object in place of the autograd context
    (diff_gaussian_rasterization._InferenceCtx).  Every METHOD the forward path calls on `ctx` must exist there -- attributes
    it merely assigns are fine on any object -- and the entry points of the path must keep the argument count
    needs_input_grad is sized for."""
    import inspect
    import sys
    sys.path.insert(0, os.path.join(ROOT, "3dgs-avatar-release_amd"))
    import diff_gaussian_rasterization as dgr
    src = inspect.getsource(dgr._RasterizeGaussians._forward) + inspect.getsource(dgr._RasterizeGaussians._finish) + \
        inspect.getsource(dgr._RasterizeGaussians.forward)
    called = set(re.findall(r"\bctx\.([a-z_]+)\(", src))
    read = set(re.findall(r"\bctx\.([a-z_]+)\b(?!\s*=[^=])", src)) - called
    ictx = dgr._InferenceCtx()
    for name in called:
        assert callable(getattr(ictx, name, None)), name
    assigned = set(re.findall(r"\bctx\.([a-z_]+)\s*=[^=]", src))
    for name in read - assigned:
        assert hasattr(ictx, name), name
    n_inputs = len(inspect.signature(dgr._RasterizeGaussians.forward).parameters) - 1  # (ctx)
    assert len(ictx.needs_input_grad) == n_inputs
    assert not any(ictx.needs_input_grad)


def test_the_entry_switch_of_render_bwd_keeps_its_loads_inside_one_statement():
    """render_bwd.hip's exec-masked LDS reads land in live registers; since round 4 each group is issued and waited for
    inside one asm statement.  The gate that checks the GENERATED code (3dgs-avatar-release_amd/check_inflight.py, run by
    build.py on every compile) is run here on the object the build left in-tree, so that it does not depend on build.py
    alone: it must find the read groups (both render_bwd modes, the round-start switch and the in-step one) and nothing
    that touches their destination registers before the wait."""
    import importlib.util
    pkg = os.path.join(ROOT, "3dgs-avatar-release_amd")
    obj = os.path.join(pkg, "build", "render_bwd.o")
    if not os.path.exists(obj):
        import __graft_entry__
        __graft_entry__.build()
    spec = importlib.util.spec_from_file_location("check_inflight", os.path.join(pkg, "check_inflight.py"))
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    assert ci.check(obj, "hipcc") >= 8
    src = open(os.path.join(pkg, "csrc", "render_bwd.hip")).read()
    # every ds_read of the file sits in an asm statement that also holds its s_waitcnt
    for stmt in src.split("asm volatile(")[1:]:
        body = stmt[:stmt.index(");")]
        if "ds_read_b" in body:
            assert "s_waitcnt lgkmcnt(0)" in body or "GS_ACC_Y" in body
    assert "s_waitcnt lgkmcnt(0)" in src[src.index("#define GS_ACC_Y"):src.index("#define GS_ACC_Y_OUT")]


# ---- the frame path's argument handling, pinned (return codes and state-buffer offsets recorded from the library as it
# was before the state carve moved behind typed views; calls that fail validation return before any HIP call)
FAKE = 0x100000   # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 32     # "large enough" for every state of the small frame below (and too small for 2^30 pairs)
SMALL = 16
BAD_ARG, EXCLUSIVE, TOO_LARGE, WORKSPACE = -1, -2, -3, -5


def _frame_args(lib, P=10, W=64, H=64):
    a = lib.GsFwdArgs()
    a.P, a.W, a.H, a.sh_degree, a.M = P, W, H, 0, 1
    a.bg = a.viewmatrix = a.projmatrix = a.campos = a.means3D = a.opacities = FAKE
    a.colors_precomp = a.scales = a.rotations = FAKE
    return a


def _grads(lib, **over):
    g = lib.GsGrads(*([FAKE] * 8))
    for k, v in over.items():
        setattr(g, k, v)
    return g


class _Call(object):
    """One entry point with arguments that pass every check; call(name=value, ...) replaces some of them.  `a_...` keywords
    set fields of the GsFwdArgs, `gr_...` of the GsGrads, `second_...` of the GsSecondImage (second=None: a null pointer)."""

    def __init__(self, lib, fn, names, **defaults):
        self.lib, self.fn, self.names, self.defaults = lib, fn, names, defaults

    def __call__(self, **over):
        lib = self.lib
        v = dict(self.defaults)
        a = _frame_args(lib)
        gr = _grads(lib)
        second = lib.GsSecondImage(FAKE, FAKE, FAKE, FAKE, BIG, 0)
        for k, x in over.items():
            if k.startswith("a_"):
                setattr(a, k[2:], x)
            elif k.startswith("gr_"):
                setattr(gr, k[3:], x)
            elif k.startswith("second_"):
                setattr(second, k[7:], x)
            else:
                assert k in v, k
                v[k] = x
        keep = []  # (host words the library may write before it validates)
        args = []
        for n in self.names:
            x = v[n]
            if n == "a":
                x = ctypes.byref(a) if x else None
            elif n == "gr":
                x = ctypes.byref(gr) if x else None
            elif n == "second":
                x = ctypes.byref(second) if x else None
            elif x == "word":
                keep.append(ctypes.c_int64(0))
                x = ctypes.cast(ctypes.byref(keep[-1]), ctypes.c_void_p) if n == "count" else ctypes.byref(keep[-1])
            args.append(x)
        return self.fn(*args)


def _entry_points(lib):
    L = lib.load()
    states = dict(geom=FAKE, gb=BIG, binning=FAKE, bb=BIG, img=FAKE, ib=BIG, D=100)
    bwd = dict(a=True, radii=FAKE, out=FAKE, dpix=FAKE, scratch=FAKE, sb=BIG, gr=True, stream=None, **states)
    bwd_head = ["a", "radii", "geom", "gb", "binning", "bb", "img", "ib", "D", "out", "dpix"]
    bwd_tail = ["scratch", "sb", "gr", "stream"]
    return dict(
        render=_Call(lib, L.gs_forward_render, ["a", "geom", "gb", "binning", "bb", "img", "ib", "D", "out", "stream"],
                     a=True, out=FAKE, stream=None, **states),
        forward=_Call(lib, L.gs_forward, ["a", "geom", "gb", "binning", "bb", "D", "img", "ib", "radii", "count", "out", "num",
                                          "stream"], a=True, radii=FAKE, count="word", out=FAKE, num="word", stream=None, **states),
        shared=_Call(lib, L.gs_forward_shared, ["a", "geom_src", "img_src", "geom", "gb", "binning", "bb", "img", "ib", "D", "out",
                                                "stream"], a=True, geom_src=FAKE, img_src=FAKE, out=FAKE, stream=None, **states),
        backward=_Call(lib, L.gs_backward, bwd_head + bwd_tail, **bwd),
        with_opacity=_Call(lib, L.gs_backward_with_opacity, bwd_head + ["dopa"] + bwd_tail, dopa=FAKE, **bwd),
        with_second=_Call(lib, L.gs_backward_with_second, bwd_head + ["second"] + bwd_tail, second=True, **bwd),
        opacity_image=_Call(lib, L.gs_opacity_image, ["a", "img", "ib", "opacity", "stream"], a=True, img=FAKE, ib=BIG,
                            opacity=FAKE, stream=None),
        pair_stats=_Call(lib, L.gs_pair_stats, ["a", "geom", "gb", "binning", "bb", "img", "ib", "D", "counts", "stream"],
                         a=True, counts=FAKE, stream=None, **states),
    )


# (entry point, what is wrong, expected).  Where two errors apply the comment names the one that wins.
_both_colours = dict(a_shs=FAKE)  # shs and colors_precomp at once: GS_E_EXCLUSIVE from the common validation
BOUNDARY_CASES = [
    ("render", dict(gb=SMALL), WORKSPACE),
    ("render", dict(bb=SMALL), WORKSPACE),
    ("render", dict(ib=SMALL), WORKSPACE),
    ("render", dict(out=None), BAD_ARG),
    ("render", dict(geom=None), BAD_ARG),
    ("render", dict(img=None), BAD_ARG),
    ("render", dict(binning=None), BAD_ARG),
    ("render", dict(D=-1), BAD_ARG),
    ("render", dict(D=1 << 30), TOO_LARGE),
    ("render", dict(a_l1_target=FAKE), BAD_ARG),
    ("render", dict(a=None), BAD_ARG),
    ("render", dict(out=None, gb=SMALL), BAD_ARG),                # null pointer before sizes
    ("render", dict(D=1 << 30, gb=SMALL), TOO_LARGE),             # capacity before sizes
    ("render", dict(D=1 << 30, a_l1_target=FAKE), BAD_ARG),       # the L1 pair before the capacity
    ("render", dict(out=None, **_both_colours), EXCLUSIVE),       # the common validation before everything else
    ("forward", dict(count=None), BAD_ARG),
    ("forward", dict(num=None), BAD_ARG),
    ("forward", dict(D=-1), BAD_ARG),
    ("forward", dict(gb=SMALL), WORKSPACE),
    ("forward", dict(ib=SMALL), WORKSPACE),
    ("forward", dict(geom=None), BAD_ARG),
    ("forward", dict(radii=None), BAD_ARG),
    ("forward", dict(**_both_colours), EXCLUSIVE),
    ("forward", dict(count=None, **_both_colours), BAD_ARG),      # its own null checks before the common validation
    ("forward", dict(geom=None, gb=SMALL), BAD_ARG),
    ("shared", dict(geom_src=None), BAD_ARG),
    ("shared", dict(img_src=None), BAD_ARG),
    ("shared", dict(out=None), BAD_ARG),
    ("shared", dict(binning=None), BAD_ARG),
    ("shared", dict(gb=SMALL), WORKSPACE),
    ("shared", dict(bb=SMALL), WORKSPACE),
    ("shared", dict(ib=SMALL), WORKSPACE),
    ("shared", dict(D=1 << 30), WORKSPACE),                       # (no capacity check here: the binning state is too small)
    ("shared", dict(geom_src=None, ib=SMALL), BAD_ARG),
    ("shared", dict(geom_src=None, **_both_colours), EXCLUSIVE),
    ("backward", dict(gr=None), BAD_ARG),
    ("backward", dict(dpix=None), BAD_ARG),
    ("backward", dict(radii=None), BAD_ARG),
    ("backward", dict(scratch=None), BAD_ARG),
    ("backward", dict(gr_dL_dmeans2D=None), BAD_ARG),
    ("backward", dict(gr_dL_dscales=None), BAD_ARG),
    ("backward", dict(gr_dL_drotations=FAKE + 4), BAD_ARG),
    ("backward", dict(sb=SMALL), WORKSPACE),
    ("backward", dict(gb=SMALL), WORKSPACE),
    ("backward", dict(bb=SMALL), WORKSPACE),
    ("backward", dict(ib=SMALL), WORKSPACE),
    ("backward", dict(D=1 << 30), WORKSPACE),
    ("backward", dict(gr_dL_drotations=FAKE + 4, sb=SMALL), BAD_ARG),
    ("backward", dict(gr=None, **_both_colours), EXCLUSIVE),
    ("with_opacity", dict(dopa=None), BAD_ARG),
    ("with_opacity", dict(sb=SMALL), WORKSPACE),
    ("with_opacity", dict(gr=None), BAD_ARG),
    ("with_opacity", dict(dopa=None, **_both_colours), BAD_ARG),  # the extra argument before the common validation
    ("with_opacity", dict(gr=None, sb=SMALL), BAD_ARG),
    ("with_second", dict(second=None), BAD_ARG),
    ("with_second", dict(second_colors=None), BAD_ARG),
    ("with_second", dict(second_img=None), BAD_ARG),
    ("with_second", dict(ib=SMALL), WORKSPACE),
    ("with_second", dict(second=None, **_both_colours), BAD_ARG),
    ("with_second", dict(second_img_bytes=SMALL, sb=SMALL), WORKSPACE),  # the first image's states before the second's
    ("with_second", dict(second_img_bytes=SMALL, **_both_colours), EXCLUSIVE),
    ("opacity_image", dict(ib=SMALL), WORKSPACE),
    ("opacity_image", dict(img=None), BAD_ARG),
    ("opacity_image", dict(opacity=None), BAD_ARG),
    ("opacity_image", dict(opacity=None, ib=SMALL), BAD_ARG),
    ("opacity_image", dict(opacity=None, **_both_colours), EXCLUSIVE),
    ("pair_stats", dict(ib=SMALL), WORKSPACE),
    ("pair_stats", dict(gb=SMALL), WORKSPACE),
    ("pair_stats", dict(bb=SMALL), WORKSPACE),
    ("pair_stats", dict(counts=None), BAD_ARG),
    ("pair_stats", dict(D=-1), BAD_ARG),
    ("pair_stats", dict(D=1 << 30), WORKSPACE),
    ("pair_stats", dict(counts=None, ib=SMALL), BAD_ARG),
    ("pair_stats", dict(counts=None, **_both_colours), EXCLUSIVE),
]


def test_frame_entry_points_answer_bad_arguments_as_before(lib):
    """Null required pointers, every state buffer too small in turn, scratch too small, a capacity of 2^30 pairs, l1_target
    without l1_loss, misaligned dL_drotations, null `second` / dL_dopacity_img -- and which error wins where two apply."""
    calls = _entry_points(lib)
    got = [(name, sorted(over), calls[name](**over)) for name, over, _ in BOUNDARY_CASES]
    want = [(name, sorted(over), rc) for name, over, rc in BOUNDARY_CASES]
    print(got)
    assert got == want
    assert {name for name, _, _ in BOUNDARY_CASES} == set(calls)


def test_second_image_state_is_checked_before_anything_is_enqueued(lib):
    """gs_backward_with_second: a second image state that is too small, or carved for another long_lists (another number of
    backward chunks), is GS_E_BAD_ARG with nothing enqueued -- like every other check of the boundary.  (Until the check
    moved in front of the tile-order launch this returned GS_E_HIP on a machine without a device.)"""
    calls = _entry_points(lib)
    assert calls["with_second"](second_img_bytes=SMALL) == BAD_ARG
    # 1024 x 1024 has 4096 tiles: the chunked backward's checkpoints exist only with long_lists
    assert calls["with_second"](a_W=1024, a_H=1024, second_long_lists=1) == BAD_ARG
    assert calls["with_second"](a_W=1024, a_H=1024, a_long_lists=1, second_long_lists=0) == BAD_ARG


def _field_offsets(L, fn, n_fields, *shape):
    out = ctypes.c_void_p(0)
    offs = []
    for f in range(n_fields):
        rc = fn(FAKE, *shape, f, ctypes.byref(out))
        offs.append(out.value - FAKE if rc == 0 else rc)
    return offs


def test_tuning_switch_names_and_value_rules(lib):
    L = lib.load()
    defaults = dict(xcd_map=1, depth_sort=1, nt_stores=1, bwd_chunks=1, fwd4=helpers.process_fwd4(), small_tiles=2048,
                    shared_qlist=1, ones_fast=1, bwd_order=1, fwd_marks=1)
    try:
        for name, v in defaults.items():
            assert L.gs_tuning(name.encode(), v) == 0, name
        assert L.gs_tuning(b"no_such_switch", 1) == BAD_ARG
        assert L.gs_tuning(None, 1) == BAD_ARG
        assert L.gs_tuning(b"fwd4", 2) == BAD_ARG        # (the chunk-parallel forward, retired)
        assert L.gs_tuning(b"fwd4", -1) == BAD_ARG
        assert L.gs_tuning(b"fwdc_ch", 256) == BAD_ARG   # (its switches: unknown names now)
        assert L.gs_tuning(b"fwdc_div", 320) == BAD_ARG
        assert L.gs_tuning(b"fwd4", 0) == 0
        assert L.gs_tuning(b"fwd4", 1) == 0
    finally:
        for name, v in defaults.items():
            lib.tuning(name, v)


def test_introspection_fields_sit_where_they_did(lib):
    """Byte offset of every gs_geom_field / gs_binning_field / gs_image_field field inside its state (the state-buffer byte
    layouts are ABI: debug.py and the tools read them), and GS_E_BAD_ARG for the first number past each range (the last
    entry of every list)."""
    L = lib.load()
    assert _field_offsets(L, L.gs_geom_field, 7, 10) == [512, 768, 0, 1024, 1792, 70144, BAD_ARG]
    assert _field_offsets(L, L.gs_geom_field, 7, 200000) == [9600000, 10400000, 0, 11200000, 13600000, 18707200, BAD_ARG]
    for W, H in ((64, 64), (1024, 1024)):  # (the binning state's carve does not depend on the image)
        assert _field_offsets(L, L.gs_binning_field, 3, 100, W, H) == [0, 512, BAD_ARG]
        assert _field_offsets(L, L.gs_binning_field, 3, 5_000_000, W, H) == [0, 20000000, BAD_ARG]
    small = [0, 256, 16640, 49408, 33024, 49664]
    large = [0, 32768, 4227072, 12615680, 8421376, 12681216]
    assert _field_offsets(L, L.gs_image_field, 7, 64, 64) == small + [BAD_ARG]
    assert _field_offsets(L, L.gs_image_field, 7, 1024, 1024) == large + [BAD_ARG]
    out = ctypes.c_void_p(0)
    assert L.gs_geom_field(None, 10, 0, ctypes.byref(out)) == BAD_ARG
    assert L.gs_geom_field(FAKE, -1, 0, ctypes.byref(out)) == BAD_ARG
    assert L.gs_binning_field(FAKE, -1, 64, 64, 0, ctypes.byref(out)) == BAD_ARG
    assert L.gs_image_field(FAKE, 64, 64, 0, None) == BAD_ARG

