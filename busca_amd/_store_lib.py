"""ctypes binding of libbusca_store.so (include/busca_store.h): the context-free library of appearance state that lives on the device - GHOST's
feature rings and moving-average table, StrongSORT's EMA feature.  load() and check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

STORE_LIB_PATH = _capi.lib_path("store")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "store", STORE_API, ABI_MAJOR)
