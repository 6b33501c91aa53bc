"""ctypes binding of libbusca_mframe.so (include/busca_mframe.h): the context-free library of the ByteTrack frames of many sequences on one resident
Kalman store.  load() and check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

MFRAME_LIB_PATH = _capi.lib_path("mframe")
HEADER = "busca_mframe.h"
ABI_MAJOR = 1                  # busca_mframe_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_MFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_MFRAME_MAX_DETS
MAX_BATCH = 65535              # BUSCA_MFRAME_MAX_BATCH
PROBLEM_WORDS = 6              # a row of the problem table: row_begin, n_k, det_begin, m_k, free_begin, n_free_k

# name -> (restype, argtypes); mirrors include/busca_mframe.h one to one
_vp, _i32 = C.c_void_p, C.c_int32
MFRAME_API = {
    "busca_mframe_version": (C.c_int, []),
    "busca_mframe_last_error": (C.c_char_p, []),
    "busca_mframe_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "busca_mframe_apply": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.c_double, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp,
                                     _i32, _vp]),
}

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "mframe", MFRAME_API, ABI_MAJOR)
