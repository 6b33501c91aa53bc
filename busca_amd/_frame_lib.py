"""ctypes binding of libbusca_frame.so (include/busca_frame.h): the context-free library of a ByteTrack frame on resident Kalman state.  It is built
next to the other libraries by busca_amd.build and bound here, apart from _lib, _track_lib, _store_lib, _rounds_lib and _sort_lib: those bindings and
the headers they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
FRAME_LIB_PATH = os.path.join(_HERE, "libbusca_frame.so")
HEADER = "busca_frame.h"
ABI_MAJOR = 1                  # busca_frame_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_FRAME_EINVAL
MAX_DETS = 2048                # BUSCA_FRAME_MAX_DETS
CLASS_FIRST, CLASS_SECOND, CLASS_NONE = 0, 1, 2      # det_class: a first-round detection, a second-round one, one of neither round

# name -> (restype, argtypes); mirrors include/busca_frame.h one to one
_vp, _i32 = C.c_void_p, C.c_int32
FRAME_API = {
    "busca_frame_version": (C.c_int, []),
    "busca_frame_last_error": (C.c_char_p, []),
    "busca_frame_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "busca_frame_apply": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.c_double, _vp, _i32, _vp, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(FRAME_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % FRAME_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(FRAME_LIB_PATH)
        for name, (res, args) in FRAME_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_frame_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_frame.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_frame error %d: %s" % (rc, load().busca_frame_last_error().decode()))
