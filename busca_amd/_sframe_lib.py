"""ctypes binding of libbusca_sframe.so (include/busca_sframe.h): the context-free library of a StrongSORT frame on resident track state.  It is built
next to the other libraries by busca_amd.build and bound here, apart from _lib, _track_lib, _store_lib, _rounds_lib, _sort_lib and _frame_lib: those
bindings and the headers they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
SFRAME_LIB_PATH = os.path.join(_HERE, "libbusca_sframe.so")
HEADER = "busca_sframe.h"
ABI_MAJOR = 1                  # busca_sframe_version() // 1000 this binding was written for
MC, CLAMP = 1, 2               # BUSCA_SFRAME_* flags of busca_sframe_cost (the values of busca_sort.h)
EINVAL = -1                    # BUSCA_SFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_SFRAME_MAX_DETS

# name -> (restype, argtypes); mirrors include/busca_sframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
SFRAME_API = {
    "busca_sframe_version": (C.c_int, []),
    "busca_sframe_last_error": (C.c_char_p, []),
    "busca_sframe_advance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp]),
    "busca_sframe_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _f64, _i32, _f64, _f64, _f64, _vp, _vp, _i32, _vp, _vp,
                                    _i32, _vp]),
    "busca_sframe_apply": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _f64, _vp, _i32, _vp, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SFRAME_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % SFRAME_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(SFRAME_LIB_PATH)
        for name, (res, args) in SFRAME_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_sframe_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_sframe.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_sframe error %d: %s" % (rc, load().busca_sframe_last_error().decode()))
