"""ctypes binding of libbusca_hip.so: one signature table per header under include/, listed in HEADERS.  No fallback: if the library is missing the
import of any compute path raises - the product never computes on the CPU."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbusca_hip.so")

ACT_RELU, ACT_GELU = 0, 1
LAYOUT_CAN_FIRST, LAYOUT_NO_BAD, LAYOUT_SEP_AS_CAN = 1, 2, 4      # busca_dt_cfg.layout bits
PREC_F32, PREC_F16, PREC_F16X3 = 0, 1, 2
ABI_MAJOR = 2                  # busca_version() // 1000 this binding was written for (include/busca_hip.h)
PAIR_CENTER, PAIR_CENTER_WEIGHTED, PAIR_IOU, PAIR_IOU_COST = 0, 1, 2, 3


class DTCfg(C.Structure):
    _fields_ = [("d", C.c_int32), ("ff", C.c_int32), ("nhead", C.c_int32), ("nlayers", C.c_int32),
                ("E", C.c_int32), ("activation", C.c_int32), ("fake_bbox_f64", C.c_int32),
                ("precision", C.c_int32), ("layout", C.c_int32)]


# name -> (restype, argtypes); mirrors include/busca_hip.h one to one
_vp, _i32, _sz = C.c_void_p, C.c_int32, C.c_size_t
SIGNATURES = {
    "busca_version": (C.c_int, []),
    "busca_build_info": (C.c_char_p, []),
    "busca_set_option": (C.c_int, [_vp, C.c_char_p, _i32]),
    "busca_get_option": (C.c_int, [_vp, C.c_char_p, C.POINTER(_i32)]),
    "busca_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "busca_ctx_destroy": (None, [_vp]),
    "busca_last_error": (C.c_char_p, [_vp]),
    "busca_dt_blob_floats": (_sz, [C.POINTER(DTCfg)]),
    "busca_dt_load_weights": (C.c_int, [_vp, C.POINTER(DTCfg), _vp, _sz, _vp, _vp, _vp, _i32]),
    "busca_dt_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "busca_dt_reserve": (C.c_int, [_vp, _i32, _i32, _i32, _vp]),
    "busca_dt_bucket_ids": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "busca_timing_enable": (C.c_int, [_vp, _i32]),
    "busca_timing_read": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), _i32]),
    "busca_pairwise": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "busca_topk_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "busca_coverage": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "busca_ecc_align": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.c_double, _vp, C.POINTER(C.c_double), C.POINTER(_i32), _vp]),
    "busca_kalman_multi_predict": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "busca_kalman_update": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "busca_kalman_initiate": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "busca_kalman_boxes": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "busca_kalman_gating": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "busca_duplicate_masks": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "busca_crop_gather": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "busca_crop_gather_ex": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "busca_crop_gather_sized": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "busca_gather_crops": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "busca_reid_forward_ex": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "busca_reid_forward_w": (C.c_int, [_vp, _vp, _i32, _vp, _vp, C.c_double, _vp, _vp]),
    "busca_reid_blob_floats": (_sz, []),
    "busca_reid_load_weights": (C.c_int, [_vp, _vp, _sz]),
    "busca_reid_load_weights_ex": (C.c_int, [_vp, _vp, _sz, _i32]),
    "busca_reid_forward": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "busca_reid_workspace_bytes": (_sz, [_i32]),
    "busca_reid_reserve": (C.c_int, [_vp, _i32, _vp]),
    "busca_bn_stats_1x1": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
}

# include/busca_assign.h, typed after SIGNATURES (which stays the one-to-one mirror of busca_hip.h)
ASSIGN_SIGNATURES = {
    "busca_linear_assignment": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
}
ASSIGN_MAX = 2048              # BUSCA_ASSIGN_MAX

# include/busca_assign_stages.h: the staged solver beside busca_linear_assignment.  Typed by load() after the tables of HEADERS, which stay the
# headers of the one-call-one-problem interface as they were
ASSIGN_STAGES_HEADER = "busca_assign_stages.h"
ASSIGN_STAGES_API = {
    "busca_assign_stages": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "busca_assign_stages_lds_bytes": (C.c_int64, [_i32, _i32, _i32]),
}
ASSIGN_STAGES_MAX = 128        # BUSCA_ASSIGN_STAGES_MAX

# include/busca_appearance.h
APPEARANCE_SIGNATURES = {
    "busca_appearance_cost": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
}
APPEAR_MIN, APPEAR_MEAN, APPEAR_MAX = 0, 1, 2       # BUSCA_APPEAR_* reductions
APPEAR_CLAMP0 = 1                                   # BUSCA_APPEAR_CLAMP0

# include/busca_ghost.h
GHOST_SIGNATURES = {
    "busca_ghost_distance": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "busca_ghost_proxies": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "busca_ghost_thresholds": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _vp, _vp]),
    "busca_ghost_combine": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.c_double, _vp, _vp, _i32, _vp, _vp, _vp]),
}
GHOST_MIN, GHOST_MEAN, GHOST_MAX, GHOST_MIDRANGE, GHOST_MEDIAN = 0, 1, 2, 3, 4       # BUSCA_GHOST_* reductions
GHOST_MEDIAN_BUDGET_MAX = 256                                                        # BUSCA_GHOST_MEDIAN_BUDGET_MAX
GHOST_PROXY_LAST, GHOST_PROXY_FIRST, GHOST_PROXY_MEAN, GHOST_PROXY_MEANNORM, GHOST_PROXY_MEDIAN = 0, 1, 2, 3, 4     # BUSCA_GHOST_PROXY_* modes

# include/busca_ghost_motion.h
GHOST_MOTION_SIGNATURES = {
    "busca_ghost_motion_append": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "busca_ghost_motion_warp": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp]),
    "busca_ghost_motion_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
}

# include/busca_reid_bn.h
REID_BN_SIGNATURES = {
    "busca_reid_running_floats": (_sz, []),
    "busca_reid_load_running_stats": (C.c_int, [_vp, _vp, _sz]),
    "busca_reid_reset_running_stats": (C.c_int, [_vp]),
    "busca_reid_get_running_stats": (C.c_int, [_vp, _vp, _sz, _vp]),
    "busca_reid_forward_running": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp]),
    "busca_reid_adapt": (C.c_int, [_vp, _vp, _i32, _vp, C.c_double, _i32, _vp, _vp]),
}
REID_OUT_PLAIN, REID_OUT_NORM = 0, 1                # BUSCA_REID_OUT_*

# include/busca_ecc.h
_i64 = C.c_int64
ECC_SIGNATURES = {
    "busca_ecc_gauss_taps": (C.c_int, [_i32, _vp]),
    "busca_ecc_prepare": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _vp, _vp]),
    "busca_ecc_align_planes": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, C.POINTER(C.c_double), C.POINTER(_i32), _vp]),
}
ECC_KSIZE_MAX = 31                                                  # BUSCA_ECC_KSIZE_MAX
ECC_EUCLIDEAN, ECC_AFFINE, ECC_TRANSLATION = 0, 1, 2                # BUSCA_ECC_* motion codes

# header under include/ -> its signature table, in the order load() types them; a name lives in exactly one of them
HEADERS = {"busca_hip.h": SIGNATURES, "busca_assign.h": ASSIGN_SIGNATURES, "busca_appearance.h": APPEARANCE_SIGNATURES, "busca_ghost.h": GHOST_SIGNATURES,
           "busca_ghost_motion.h": GHOST_MOTION_SIGNATURES, "busca_reid_bn.h": REID_BN_SIGNATURES, "busca_ecc.h": ECC_SIGNATURES}
__doc__ += "\nHeaders: " + ", ".join("include/" + h for h in HEADERS) + "."

_lib = None


def load():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). "
                              "busca_amd has no CPU fallback." % LIB_PATH)
        # torch must be imported first: it bundles its own libamdhip64 (SONAME libamdhip64.so.7); when that
        # copy is already loaded, this library's NEEDED libamdhip64.so.7 binds to it and both share ONE HIP
        # runtime (same device pointers, same streams).  Loading in the other order gives two runtimes.
        import torch  # noqa: F401
        lib = C.CDLL(os.environ.get("BUSCA_HIP_LIB", LIB_PATH))      # override: experiment builds of the same ABI
        for table in list(HEADERS.values()) + [ASSIGN_STAGES_API]:
            for name, (res, args) in table.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        v = lib.busca_version()
        if v // 1000 != ABI_MAJOR:
            raise ImportError("libbusca_hip.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (v, ABI_MAJOR))
        _lib = lib
    return _lib


class BuscaError(RuntimeError):
    pass


def build_info(lib=None):
    """The flag set the loaded library was compiled with (busca_build_info)."""
    return (lib or load()).busca_build_info().decode()


class Context:
    """One busca_ctx per process/GPU."""

    def __init__(self, device=0):
        self.lib = load()
        h = _vp()
        rc = self.lib.busca_ctx_create(int(device), C.byref(h))
        if rc != 0 or not h.value:
            raise BuscaError("busca_ctx_create(device=%d) failed with %d: %s" % (
                device, rc, self.lib.busca_last_error(None).decode()))
        self.h = h
        self.device = int(device)

    def check(self, rc):
        if rc != 0:
            raise BuscaError("libbusca_hip error %d: %s" % (rc, self.lib.busca_last_error(self.h).decode()))

    def set_option(self, name, value):
        """Developer option of this context (include/busca_hip.h: busca_set_option)."""
        self.check(self.lib.busca_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = _i32(0)
        self.check(self.lib.busca_get_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        # host-side attachments of busca_amd.geometry (frame scope, pinned tables still referenced behind their launches, crop pool)
        self._frame_scope = None
        q = getattr(self, "_pinned_in_flight", None)
        if q:
            for _, ev in q:
                ev.synchronize()
            q.clear()
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.busca_ctx_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data
