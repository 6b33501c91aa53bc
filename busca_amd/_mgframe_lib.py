"""ctypes binding of libbusca_mgframe.so (include/busca_mgframe.h): the context-free library of the GHOST frames of many sequences on one resident
store.  load() and check() come from _capi.bind.  No fallback: a missing library raises."""
import ctypes as C

from . import _capi

MGFRAME_LIB_PATH = _capi.lib_path("mgframe")
HEADER = "busca_mgframe.h"
ABI_MAJOR = 1                  # busca_mgframe_version() // 1000 this binding was written for
EINVAL = -1                    # BUSCA_MGFRAME_EINVAL
MAX_DETS = 2048                # BUSCA_MGFRAME_MAX_DETS
MAX_BATCH = 65535              # BUSCA_MGFRAME_MAX_BATCH
MAX_ROWS = 65535               # BUSCA_MGFRAME_MAX_ROWS
PROBLEM_WORDS = 13             # a row of the problem table: act_begin, na, inact_begin, ni, idle_begin, nidle, det_begin, m, free_begin, n_free, warp, frame, flags
DIFF32, STEP = 1, 2            # BUSCA_MGFRAME_DIFF32 / _STEP
E_MIN, E_MAX = 16, 2048        # BUSCA_MGFRAME_E_MIN / _MAX
MEDIAN_BUDGET_MAX = 256        # BUSCA_MGFRAME_MEDIAN_BUDGET_MAX

# name -> (restype, argtypes); mirrors include/busca_mgframe.h one to one
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
# S, slot, n_total, m_total, f_total, n_warps, problems, batch, N, M, L, R, inact_row: what every call but advance takes in this order
_TABLE = [_i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32]
MGFRAME_API = {
    "busca_mgframe_version": (C.c_int, []),
    "busca_mgframe_last_error": (C.c_char_p, []),
    "busca_mgframe_advance": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                        _i32, _vp, _i32, _vp]),
    "busca_mgframe_distance": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32] + _TABLE + [_vp, _i32, _vp]),
    "busca_mgframe_thresholds": (C.c_int, [_vp, _f64, _f64, _i32] + _TABLE + [_vp, _i32, _vp]),
    "busca_mgframe_cost": (C.c_int, [_vp, _vp, _vp, _f64, _vp, _vp, _vp] + _TABLE + [_i32, _vp]),
    "busca_mgframe_keep": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32] + _TABLE + [_i32, _vp]),
    "busca_mgframe_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp] + _TABLE
                            + [_vp, _i32, _vp]),
}

_lib = None                    # the loaded library, kept here by load()
load, check = _capi.bind(__name__, "mgframe", MGFRAME_API, ABI_MAJOR)
