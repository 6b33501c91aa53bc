"""ctypes binding of libbusca_sort.so (include/busca_sort.h): the context-free library of StrongSORT's track state that lives on the device.  It is
built next to the other four libraries by busca_amd.build and bound here, apart from _lib, _track_lib, _store_lib and _rounds_lib: those bindings and
the headers they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
SORT_LIB_PATH = os.path.join(_HERE, "libbusca_sort.so")
HEADER = "busca_sort.h"
ABI_MAJOR = 1                  # busca_sort_version() // 1000 this binding was written for
MC, CLAMP = 1, 2               # BUSCA_SORT_* flags of busca_sort_gate_cost / busca_sort_iou_cost
EINVAL = -1                    # BUSCA_SORT_EINVAL

# name -> (restype, argtypes); mirrors include/busca_sort.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
SORT_API = {
    "busca_sort_version": (C.c_int, []),
    "busca_sort_last_error": (C.c_char_p, []),
    "busca_sort_predict": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "busca_sort_update": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "busca_sort_gate_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _f64, _i32, _f64, _f64, _vp, _vp, _i32, _vp]),
    "busca_sort_iou_cost": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _f64, _vp, _i32, _vp]),
    "busca_sort_camera_update": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SORT_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % SORT_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(SORT_LIB_PATH)
        for name, (res, args) in SORT_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_sort_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_sort.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_sort error %d: %s" % (rc, load().busca_sort_last_error().decode()))
