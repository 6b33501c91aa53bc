"""ctypes binding of libbusca_track.so (include/busca_track.h): the context-free library of tracker state that lives on the device.  load() and
check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

TRACK_LIB_PATH = _capi.lib_path("track")
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

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "track", TRACK_API, ABI_MAJOR)
