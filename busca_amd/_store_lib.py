"""ctypes binding of libbusca_store.so (include/busca_store.h): the context-free library of appearance state that lives on the device - GHOST's feature
rings and moving-average table, StrongSORT's EMA feature.  It is built next to libbusca_hip.so and libbusca_track.so by busca_amd.build and bound here,
apart from _lib and _track_lib: those bindings and the headers they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
STORE_LIB_PATH = os.path.join(_HERE, "libbusca_store.so")
HEADER = "busca_store.h"
ABI_MAJOR = 1                  # busca_store_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_STORE_EINVAL

# name -> (restype, argtypes); mirrors include/busca_store.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
STORE_API = {
    "busca_store_version": (C.c_int, []),
    "busca_store_last_error": (C.c_char_p, []),
    "busca_store_ring_add": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp]),
    "busca_store_release": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "busca_store_mv_avg": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _f64, _f64, _vp, _i32, _vp]),
    "busca_store_ema_fit": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _f64, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(STORE_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % STORE_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(STORE_LIB_PATH)
        for name, (res, args) in STORE_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_store_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_store.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_store error %d: %s" % (rc, load().busca_store_last_error().decode()))
