"""ctypes binding of libbusca_msframe.so (include/busca_msframe.h): the context-free library of the StrongSORT frames of many sequences on one
resident store.  load() and check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

MSFRAME_LIB_PATH = _capi.lib_path("msframe")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "msframe", MSFRAME_API, ABI_MAJOR)
