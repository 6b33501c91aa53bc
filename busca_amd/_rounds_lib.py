"""ctypes binding of libbusca_rounds.so (include/busca_rounds.h): the context-free library of association rounds batched across sequences.  load() and
check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

ROUNDS_LIB_PATH = _capi.lib_path("rounds")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "rounds", ROUNDS_API, ABI_MAJOR)
