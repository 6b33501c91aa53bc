"""ctypes binding of libbusca_frame.so (include/busca_frame.h): the context-free library of a ByteTrack frame on resident Kalman state.  load() and
check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

FRAME_LIB_PATH = _capi.lib_path("frame")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "frame", FRAME_API, ABI_MAJOR)
