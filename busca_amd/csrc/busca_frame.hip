// libbusca_frame.so: a ByteTrack frame on resident Kalman state and its C-ABI (include/busca_frame.h).  A library of its own, without a busca_ctx, as
// libbusca_track.so and libbusca_rounds.so are: the interfaces of the other libraries stay what they are.  The device code is the per-track bodies of
// track_kernel.hip.inc, the pair functions of pairwise_kernel.hip.inc and the addressing of kalman_store_kernel.hip.inc - the very text
// libbusca_track.so compiles - behind the two kernels of frame_kernel.hip.inc.  The other kernels the three included files define come along unused
// (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here

#pragma GCC visibility push(default)
#include "../../include/busca_frame.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "frame_kernel.hip.inc"

#define CAPI_EHIP BUSCA_FRAME_EHIP
#include "capi_prelude.hpp"

extern "C" int busca_frame_version(void) { return 1000; }

extern "C" const char* busca_frame_last_error(void) { return g_err; }

extern "C" int busca_frame_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_tlbr,
                                const double* det_score, const uint8_t* det_class, int32_t m, double* out, int32_t* status, int32_t device,
                                void* stream) {
    static const char* who = "busca_frame_cost";
    if (S < 0 || n < 0 || m < 0) return refuse(BUSCA_FRAME_EINVAL, "%s: negative size (S %d, n %d, m %d)", who, S, n, m);
    if (device < 0) return refuse(BUSCA_FRAME_EINVAL, "%s: negative device %d", who, device);
    if (n == 0 || m == 0) return 0;
    if (!mean || !slot) return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (mean and slot are required)", who);
    if (!det_tlbr || !det_class || !out) return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (det_tlbr, det_class and out are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_tlbr, 8) || misaligned(det_score, 8) || misaligned(out, 8) || misaligned(slot, 4) ||
        misaligned(status, 4))
        return refuse(BUSCA_FRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const long long row_tiles = ((long long)n + PW_TA - 1) / PW_TA, col_tiles = ((long long)m + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_FRAME_EINVAL, "%s: %d tracks need more workgroups than a grid holds (%d at most)", who, n, 65535 * PW_TA);
    const KStore k{(double*)mean, (double*)cov, (const int*)slot, S, n};       // the covariances are not read: a box is a function of the mean
    CAPI_LAUNCH(who, device, frame_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles), dim3(256), stream, k, det_tlbr, det_score, det_class, m,
                out, (int*)status);
    return 0;
}

extern "C" int busca_frame_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const int32_t* row_to_col,
                                 const int32_t* col_to_row, const double* det_xyah, const double* det_score, const uint8_t* det_class, int32_t m,
                                 double det_thresh, const int32_t* free_slot, int32_t n_free, int32_t* new_slot, int32_t* status, int32_t device,
                                 void* stream) {
    static const char* who = "busca_frame_apply";
    if (S < 0 || n < 0 || m < 0) return refuse(BUSCA_FRAME_EINVAL, "%s: negative size (S %d, n %d, m %d)", who, S, n, m);
    if (n_free < 0) return refuse(BUSCA_FRAME_EINVAL, "%s: negative size (n_free %d)", who, n_free);
    if (device < 0) return refuse(BUSCA_FRAME_EINVAL, "%s: negative device %d", who, device);
    if (det_thresh != det_thresh) return refuse(BUSCA_FRAME_EINVAL, "%s: det_thresh is NaN", who);
    if (m > BUSCA_FRAME_MAX_DETS) return refuse(BUSCA_FRAME_EINVAL, "%s: %d detections, one call takes %d", who, m, BUSCA_FRAME_MAX_DETS);
    if ((long long)n + m > 2147483647LL) return refuse(BUSCA_FRAME_EINVAL, "%s: %d rows and %d columns need more workgroups than a grid holds", who, n, m);
    if (n == 0 && m == 0) return 0;
    if (!mean || !cov) return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (mean and cov are required)", who);
    if (n > 0 && (!slot || !row_to_col)) return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (slot and row_to_col are required with n > 0)", who);
    if (m > 0 && (!col_to_row || !det_xyah || !det_class || !new_slot))
        return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (col_to_row, det_xyah, det_class and new_slot are required with m > 0)", who);
    if (m > 0 && n_free > 0 && !free_slot) return refuse(BUSCA_FRAME_EINVAL, "%s: null pointer (free_slot with n_free %d)", who, n_free);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_score, 8) || misaligned(slot, 4) ||
        misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(free_slot, 4) || misaligned(new_slot, 4) || misaligned(status, 4))
        return refuse(BUSCA_FRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const KStore k{mean, cov, (const int*)slot, S, n};
    FrameApply f;
    f.row_to_col = (const int*)row_to_col, f.col_to_row = (const int*)col_to_row;
    f.det_xyah = det_xyah, f.det_score = det_score, f.det_class = det_class;
    f.free_slot = (const int*)free_slot, f.new_slot = (int*)new_slot, f.status = (int*)status;
    f.det_thresh = det_thresh, f.m = m, f.n_free = n_free;
    CAPI_LAUNCH(who, device, frame_apply_kernel, dim3((unsigned)((long long)n + m)), dim3(64), stream, k, f);
    return 0;
}
