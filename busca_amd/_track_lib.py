"""ctypes binding of libbusca_track.so (include/busca_track.h): the context-free library of tracker state that lives on the device.  It is built next
to libbusca_hip.so by busca_amd.build and bound here, apart from _lib: that binding and the headers it lists stay what they are.  No fallback: a
missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
TRACK_LIB_PATH = os.path.join(_HERE, "libbusca_track.so")
HEADER = "busca_track.h"
ABI_MAJOR = 1                  # busca_track_version() // 1000 this binding was written for
FUSE_MOTION, ONLY_POSITION, GATE_ONLY = 1, 2, 4      # BUSCA_TRACK_* flags of busca_track_round_cost
EINVAL = -1                    # BUSCA_TRACK_EINVAL

# name -> (restype, argtypes); mirrors include/busca_track.h one to one
_vp, _i32 = C.c_void_p, C.c_int32
TRACK_API = {
    "busca_track_version": (C.c_int, []),
    "busca_track_last_error": (C.c_char_p, []),
    "busca_track_kalman_initiate": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp]),
    "busca_track_kalman_predict": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp]),
    "busca_track_kalman_update": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp]),
    "busca_track_kalman_boxes": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp]),
    "busca_track_round_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, C.c_double, _vp, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(TRACK_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % TRACK_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(TRACK_LIB_PATH)
        for name, (res, args) in TRACK_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_track_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_track.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_track error %d: %s" % (rc, load().busca_track_last_error().decode()))
