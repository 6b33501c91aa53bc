// libbusca_track.so: tracker state resident on the device and its C-ABI (include/busca_track.h).  A library of its own, without a busca_ctx: the calls
// need no weights and no workspace, and libbusca_hip.so's interface stays what it is.  The device code is the per-track bodies of track_kernel.hip.inc
// and the pair functions of pairwise_kernel.hip.inc - the very text libbusca_hip.so compiles - behind slot-indexed kernels.  The list-ordered kernels
// those two files also define come along unused (hidden, a few KB of code object): including the files whole keeps one text for both libraries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here

#pragma GCC visibility push(default)
#include "../../include/busca_track.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"

static_assert(KSTORE_FUSE_MOTION == BUSCA_TRACK_FUSE_MOTION && KSTORE_ONLY_POSITION == BUSCA_TRACK_ONLY_POSITION && KSTORE_GATE_ONLY == BUSCA_TRACK_GATE_ONLY,
              "kalman_store_kernel.hip.inc and busca_track.h disagree on the flags");

#define CAPI_EHIP BUSCA_TRACK_EHIP
#define CAPI_EINVAL BUSCA_TRACK_EINVAL
#define CAPI_STORE_ARGS        // this library's calls take a Kalman store and its slot list
#include "capi_prelude.hpp"

// the measurement operands of initiate / update
static int meas_args(const char* who, int32_t n, const double* meas, const int32_t* det_index, int32_t m) {
    if (m < 0) return refuse(BUSCA_TRACK_EINVAL, "%s: negative size (m %d)", who, m);
    if (n == 0) return 0;
    if (!det_index && n > m) return refuse(BUSCA_TRACK_EINVAL, "%s: %d slots for %d measurements and no det_index", who, n, m);
    if (m > 0 && !meas) return refuse(BUSCA_TRACK_EINVAL, "%s: null pointer (meas)", who);
    if (misaligned(meas, 8) || misaligned(det_index, 4)) return refuse(BUSCA_TRACK_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    return 0;
}

extern "C" int busca_track_version(void) { return 1000; }

extern "C" const char* busca_track_last_error(void) { return g_err; }

extern "C" int busca_track_kalman_initiate(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index,
                                           int32_t m, int32_t device, void* stream) {
    static const char* who = "busca_track_kalman_initiate";
    int rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc == 0) rc = meas_args(who, n, meas, det_index, m);
    if (rc != 0 || n == 0) return rc;
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, kstore_initiate_kernel, dim3((unsigned)n), dim3(64), stream, k, meas, (const int*)det_index, m);
    return 0;
}

extern "C" int busca_track_kalman_predict(double* mean, double* cov, int32_t S, const int32_t* slot, const uint8_t* not_tracked, int32_t n, int32_t device,
                                          void* stream) {
    static const char* who = "busca_track_kalman_predict";
    const int rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc != 0 || n == 0) return rc;
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, kstore_predict_kernel, dim3((unsigned)n), dim3(64), stream, k, not_tracked);
    return 0;
}

extern "C" int busca_track_kalman_update(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index,
                                         int32_t m, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_track_kalman_update";
    int rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc == 0) rc = meas_args(who, n, meas, det_index, m);
    if (rc != 0 || n == 0) return rc;
    if (misaligned(status, 4)) return refuse(BUSCA_TRACK_EINVAL, "%s: misaligned pointer (4 bytes for int32)", who);
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, kstore_update_kernel, dim3((unsigned)n), dim3(64), stream, k, meas, (const int*)det_index, m, (int*)status);
    return 0;
}

extern "C" int busca_track_kalman_boxes(const double* mean, int32_t S, const int32_t* slot, int32_t n, int32_t tlbr, double* out, int32_t device,
                                        void* stream) {
    static const char* who = "busca_track_kalman_boxes";
    const int rc = store_args(who, mean, nullptr, false, S, slot, n, device);
    if (rc != 0) return rc;
    if (tlbr != 0 && tlbr != 1) return refuse(BUSCA_TRACK_EINVAL, "%s: tlbr = %d, it is 0 (tlwh) or 1 (tlbr)", who, tlbr);
    if (n == 0) return 0;
    if (!out) return refuse(BUSCA_TRACK_EINVAL, "%s: null pointer (out)", who);
    if (misaligned(out, 8)) return refuse(BUSCA_TRACK_EINVAL, "%s: misaligned pointer (8 bytes for float64)", who);
    const KStore k{(double*)mean, nullptr, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, kstore_boxes_kernel, dim3((unsigned)((n + 255LL) / 256)), dim3(256), stream, k, tlbr, out);
    return 0;
}

extern "C" int busca_track_round_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_tlbr,
                                      const double* det_xyah, const double* det_score, int32_t m, int32_t flags, double lambda, double* out,
                                      int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_track_round_cost";
    const int known = BUSCA_TRACK_FUSE_MOTION | BUSCA_TRACK_ONLY_POSITION | BUSCA_TRACK_GATE_ONLY;
    if (m < 0) return refuse(BUSCA_TRACK_EINVAL, "%s: negative size (m %d)", who, m);
    if (flags & ~known) return refuse(BUSCA_TRACK_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~known));
    if ((flags & BUSCA_TRACK_FUSE_MOTION) && (flags & BUSCA_TRACK_GATE_ONLY))
        return refuse(BUSCA_TRACK_EINVAL, "%s: FUSE_MOTION and GATE_ONLY exclude each other", who);
    if (lambda != lambda) return refuse(BUSCA_TRACK_EINVAL, "%s: lambda is NaN", who);
    const bool motion = (flags & (BUSCA_TRACK_FUSE_MOTION | BUSCA_TRACK_GATE_ONLY)) != 0;
    const int rc = store_args(who, mean, cov, motion, S, slot, n, device);
    if (rc != 0 || n == 0 || m == 0) return rc;
    if (!det_tlbr || !out) return refuse(BUSCA_TRACK_EINVAL, "%s: null pointer (det_tlbr and out are required)", who);
    if (motion && !det_xyah) return refuse(BUSCA_TRACK_EINVAL, "%s: det_xyah is NULL with a motion flag (0x%x)", who, (unsigned)flags);
    if (misaligned(det_tlbr, 8) || misaligned(det_xyah, 8) || misaligned(det_score, 8) || misaligned(out, 8) || misaligned(status, 4))
        return refuse(BUSCA_TRACK_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const long long row_tiles = ((long long)n + PW_TA - 1) / PW_TA, col_tiles = ((long long)m + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_TRACK_EINVAL, "%s: %d tracks need more workgroups than a grid holds (%d at most)", who, n, 65535 * PW_TA);
    const KStore k{(double*)mean, (double*)cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, kstore_round_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles), dim3(256), stream, k, det_tlbr,
                motion ? det_xyah : nullptr, det_score, m, flags, lambda, out, (int*)status);
    return 0;
}
