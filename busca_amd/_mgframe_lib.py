"""ctypes binding of libbusca_mgframe.so (include/busca_mgframe.h): the context-free library of the GHOST frames of many sequences on one resident
store.  It is built next to the other libraries by busca_amd.build and bound here, apart from _lib, _track_lib, _store_lib, _rounds_lib, _sort_lib,
_frame_lib, _sframe_lib, _mframe_lib, _msframe_lib and _gframe_lib: those bindings and the headers they list stay what they are.  No fallback: a
missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
MGFRAME_LIB_PATH = os.path.join(_HERE, "libbusca_mgframe.so")
HEADER = "busca_mgframe.h"
ABI_MAJOR = 1                  # busca_mgframe_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_MGFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_MGFRAME_MAX_DETS
MAX_BATCH = 65535              # BUSCA_MGFRAME_MAX_BATCH
MAX_ROWS = 65535               # BUSCA_MGFRAME_MAX_ROWS
PROBLEM_WORDS = 13             # a row of the problem table: act_begin, na, inact_begin, ni, idle_begin, nidle, det_begin, m, free_begin, n_free, warp, frame, flags
DIFF32, STEP = 1, 2            # BUSCA_MGFRAME_DIFF32 / _STEP
E_MIN, E_MAX = 16, 2048        # BUSCA_MGFRAME_E_MIN / _MAX
MEDIAN_BUDGET_MAX = 256        # BUSCA_MGFRAME_MEDIAN_BUDGET_MAX

# name -> (restype, argtypes); mirrors include/busca_mgframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
# S, slot, n_total, m_total, f_total, n_warps, problems, batch, N, M, L, R, inact_row: what every call but advance takes in this order
_TABLE = [_i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32]
MGFRAME_API = {
    "busca_mgframe_version": (C.c_int, []),
    "busca_mgframe_last_error": (C.c_char_p, []),
    "busca_mgframe_advance": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                        _i32, _vp, _i32, _vp]),
    "busca_mgframe_distance": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32] + _TABLE + [_vp, _i32, _vp]),
    "busca_mgframe_thresholds": (C.c_int, [_vp, _f64, _f64, _i32] + _TABLE + [_vp, _i32, _vp]),
    "busca_mgframe_cost": (C.c_int, [_vp, _vp, _vp, _f64, _vp, _vp, _vp] + _TABLE + [_i32, _vp]),
    "busca_mgframe_keep": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32] + _TABLE + [_i32, _vp]),
    "busca_mgframe_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp] + _TABLE
                            + [_vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(MGFRAME_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % MGFRAME_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(MGFRAME_LIB_PATH)
        for name, (res, args) in MGFRAME_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_mgframe_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_mgframe.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_mgframe error %d: %s" % (rc, load().busca_mgframe_last_error().decode()))
