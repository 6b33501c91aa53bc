"""ctypes binding of libbusca_rounds.so (include/busca_rounds.h): the context-free library of association rounds batched across sequences.  It is
built next to the other three libraries by busca_amd.build and bound here, apart from _lib, _track_lib and _store_lib: those bindings and the headers
they list stay what they are.  No fallback: a missing library raises."""
import ctypes as C
import os

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDS_LIB_PATH = os.path.join(_HERE, "libbusca_rounds.so")
HEADER = "busca_rounds.h"
ABI_MAJOR = 1                  # busca_rounds_version() // 1000 this binding was written for
FUSE_MOTION, ONLY_POSITION, GATE_ONLY = 1, 2, 4      # BUSCA_ROUNDS_* flags of busca_rounds_cost
EINVAL = -1                    # BUSCA_ROUNDS_EINVAL
MAX_BATCH = 65535              # problems of one busca_rounds_cost call

# name -> (restype, argtypes); mirrors include/busca_rounds.h one to one
_vp, _i32 = C.c_void_p, C.c_int32
ROUNDS_API = {
    "busca_rounds_version": (C.c_int, []),
    "busca_rounds_last_error": (C.c_char_p, []),
    "busca_rounds_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _i32, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(ROUNDS_LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % ROUNDS_LIB_PATH)
        import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
        lib = C.CDLL(ROUNDS_LIB_PATH)
        for name, (res, args) in ROUNDS_API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.busca_rounds_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_rounds.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


def check(rc):
    """Raise BuscaError with the library's message for a non-zero return code."""
    if rc != 0:
        raise BuscaError("libbusca_rounds error %d: %s" % (rc, load().busca_rounds_last_error().decode()))
