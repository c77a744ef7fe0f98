"""ctypes binding of the wide fused MLP's entry points of libgsplat_mi355.so (include/gsplat_mi355_wmlp.h): the module's own
header, and its own table beside gsplat_mi355/_lib.py's.  load() returns the library _lib.load() returns, with this
table applied as well; tests/test_wide_mlp_host.py holds the table, the struct and the constants against the header."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_int32, c_size_t, c_uint32, c_void_p

from . import _lib

# include/gsplat_mi355_wmlp.h
GS_WMLP_MAX_WIDTH, GS_WMLP_MAX_HIDDEN, GS_WMLP_MAX_LAYERS, GS_WMLP_MAX_FREQS, GS_WMLP_MAX_ENC = 256, 8, 9, 10, 512
GS_WMLP_MAX_COND, GS_WMLP_MAX_OUT, GS_WMLP_TILE_ROWS, GS_WMLP_PARTIAL_MIN_ROWS, GS_WMLP_MAX_PARTIALS = 512, 64, 128, 256, 128


class GsWideMlpArgs(ctypes.Structure):  # include/gsplat_mi355_wmlp.h: GsWideMlpArgs
    _fields_ = [(n, c_int32) for n in ("N", "dim_x", "multires", "include_input", "dim_cond", "width", "n_hidden", "dim_out")] + [
        ("skip_mask", c_uint32), ("slope", c_float), ("band_w", c_float * GS_WMLP_MAX_FREQS), ("x", c_void_p), ("cond", c_void_p)] + [
        (n, c_void_p * GS_WMLP_MAX_LAYERS) for n in ("W", "b", "dW", "db")] + [("dx", c_void_p), ("dcond", c_void_p)]


_size_out = POINTER(c_size_t)
nbytes = _lib.nbytes  # (fn, *args) -> the size_t a size query writes
# every function of include/gsplat_mi355_wmlp.h, in the header's order: name -> (restype, argtypes)
SIGNATURES = {
    "gs_wmlp_workspace_bytes": (c_int, [POINTER(GsWideMlpArgs), c_int32, _size_out]),
    "gs_wmlp_saved_bytes": (c_int, [POINTER(GsWideMlpArgs), _size_out]),
    "gs_wmlp_forward": (c_int, [POINTER(GsWideMlpArgs), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gs_wmlp_backward": (c_int, [POINTER(GsWideMlpArgs), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}
_applied = False


def load():
    """The HIP library (as _lib.load() loads it: there is no fallback), with this module's functions typed."""
    global _applied
    L = _lib.load()
    if not _applied:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _applied = True
    return L
