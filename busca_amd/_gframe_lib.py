"""ctypes binding of libbusca_gframe.so (include/busca_gframe.h): the context-free library of a GHOST frame on resident track state.  load() and
check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

GFRAME_LIB_PATH = _capi.lib_path("gframe")
HEADER = "busca_gframe.h"
ABI_MAJOR = 1                  # busca_gframe_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_GFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_GFRAME_MAX_DETS

# name -> (restype, argtypes); mirrors include/busca_gframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
GFRAME_API = {
    "busca_gframe_version": (C.c_int, []),
    "busca_gframe_last_error": (C.c_char_p, []),
    "busca_gframe_advance": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "busca_gframe_cost": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _f64, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "busca_gframe_keep": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "busca_gframe_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32,
                                     _vp, _vp, _i32, _vp, _i32, _vp]),
}

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "gframe", GFRAME_API, ABI_MAJOR)
