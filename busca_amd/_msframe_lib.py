"""ctypes binding of libbusca_msframe.so (include/busca_msframe.h): the context-free library of the StrongSORT frames of many sequences on one resident
store.  It is built next to the other libraries by busca_amd.build and bound here, apart from _lib, _track_lib, _store_lib, _rounds_lib, _sort_lib,
_frame_lib, _sframe_lib and _msframe_lib: those bindings and the headers they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
MSFRAME_LIB_PATH = os.path.join(_HERE, "libbusca_msframe.so")
HEADER = "busca_msframe.h"
ABI_MAJOR = 1                  # busca_msframe_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_MSFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_MSFRAME_MAX_DETS
MAX_BATCH = 65535              # BUSCA_MSFRAME_MAX_BATCH
PROBLEM_WORDS = 7              # a row of the problem table: row_begin, n_k, det_begin, m_k, free_begin, n_free_k, matrix_k
MC, CLAMP = 1, 2               # BUSCA_MSFRAME_MC / _CLAMP
E_MIN, E_MAX = 16, 2048        # BUSCA_MSFRAME_E_MIN / _MAX

# name -> (restype, argtypes); mirrors include/busca_msframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
MSFRAME_API = {
    "busca_msframe_version": (C.c_int, []),
    "busca_msframe_last_error": (C.c_char_p, []),
    "busca_msframe_advance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "busca_msframe_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _f64, _i32, _f64, _f64, _f64, _vp, _vp,
                                     _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "busca_msframe_apply": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _f64, _vp, _i32, _i32, _vp, _i32, _i32, _i32,
                                      _vp, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(MSFRAME_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % MSFRAME_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(MSFRAME_LIB_PATH)
        for name, (res, args) in MSFRAME_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_msframe_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_msframe.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_msframe error %d: %s" % (rc, load().busca_msframe_last_error().decode()))
