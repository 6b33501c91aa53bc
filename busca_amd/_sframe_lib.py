"""ctypes binding of libbusca_sframe.so (include/busca_sframe.h): the context-free library of a StrongSORT frame on resident track state.  load() and
check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

SFRAME_LIB_PATH = _capi.lib_path("sframe")
HEADER = "busca_sframe.h"
ABI_MAJOR = 1                  # busca_sframe_version() // 1000 this binding was written for
MC, CLAMP = 1, 2               # BUSCA_SFRAME_* flags of busca_sframe_cost (the values of busca_sort.h)
EINVAL = -1                    # BUSCA_SFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_SFRAME_MAX_DETS

# name -> (restype, argtypes); mirrors include/busca_sframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
SFRAME_API = {
    "busca_sframe_version": (C.c_int, []),
    "busca_sframe_last_error": (C.c_char_p, []),
    "busca_sframe_advance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp]),
    "busca_sframe_cost": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _f64, _i32, _f64, _f64, _f64, _vp, _vp, _i32, _vp, _vp,
                                    _i32, _vp]),
    "busca_sframe_apply": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _f64, _vp, _i32, _vp, _vp, _i32, _vp]),
}

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "sframe", SFRAME_API, ABI_MAJOR)
