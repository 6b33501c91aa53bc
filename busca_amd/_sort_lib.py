"""ctypes binding of libbusca_sort.so (include/busca_sort.h): the context-free library of StrongSORT's track state that lives on the device.  load()
and check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

SORT_LIB_PATH = _capi.lib_path("sort")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "sort", SORT_API, ABI_MAJOR)
