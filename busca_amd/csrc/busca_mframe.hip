// libbusca_mframe.so: the ByteTrack frames of many sequences on one resident Kalman store and its C-ABI (include/busca_mframe.h).  A library of its
// own, without a busca_ctx, as libbusca_frame.so and libbusca_rounds.so are: the interfaces of the other libraries stay what they are.  The device
// code is the text libbusca_frame.so compiles - track_kernel.hip.inc, pairwise_kernel.hip.inc, kalman_store_kernel.hip.inc and the tile, row and column
// bodies of frame_kernel.hip.inc - behind the two kernels of mframe_kernel.hip.inc.  The other kernels the four included files define come along
// unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here
#include "../../include/busca_frame.h"      // BUSCA_FRAME_MAX_DETS; declarations only (hidden here): no busca_frame_* function is defined or exported

#pragma GCC visibility push(default)
#include "../../include/busca_mframe.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

static_assert(BUSCA_MFRAME_MAX_DETS == BUSCA_FRAME_MAX_DETS, "one limit for a problem's detections");

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "frame_kernel.hip.inc"
#include "mframe_kernel.hip.inc"

#define CAPI_EHIP BUSCA_MFRAME_EHIP
#include "capi_prelude.hpp"

// the sizes both calls take, judged alike
static int sizes_refused(const char* who, int32_t S, int32_t n_total, int32_t m_total, int32_t f_total, int32_t batch, int32_t N, int32_t M,
                         int32_t device) {
    if (S < 0 || n_total < 0 || m_total < 0 || f_total < 0)
        return refuse(BUSCA_MFRAME_EINVAL, "%s: negative size (S %d, n_total %d, m_total %d, f_total %d)", who, S, n_total, m_total, f_total);
    if (batch < 0 || N < 0 || M < 0) return refuse(BUSCA_MFRAME_EINVAL, "%s: negative size (batch %d, N %d, M %d)", who, batch, N, M);
    if (device < 0) return refuse(BUSCA_MFRAME_EINVAL, "%s: negative device %d", who, device);
    if (batch > BUSCA_MFRAME_MAX_BATCH)
        return refuse(BUSCA_MFRAME_EINVAL, "%s: %d problems are more than a grid holds (%d at most)", who, batch, BUSCA_MFRAME_MAX_BATCH);
    return 0;
}

extern "C" int busca_mframe_version(void) { return 1000; }

extern "C" const char* busca_mframe_last_error(void) { return g_err; }

extern "C" int busca_mframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_tlbr,
                                 const double* det_score, const uint8_t* det_class, int32_t m_total, int32_t f_total, const int32_t* problems,
                                 int32_t batch, int32_t N, int32_t M, double* out, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_mframe_cost";
    if (sizes_refused(who, S, n_total, m_total, f_total, batch, N, M, device)) return BUSCA_MFRAME_EINVAL;
    const long long row_tiles = ((long long)N + PW_TA - 1) / PW_TA, col_tiles = ((long long)M + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_MFRAME_EINVAL, "%s: N = %d tracks need more workgroups than a grid holds (%d at most)", who, N, 65535 * PW_TA);
    if (batch == 0 || N == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;      // with an empty list every problem is empty or skipped
    if (!mean || !slot) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (mean and slot are required)", who);
    if (!problems) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (!det_tlbr || !det_class || !out) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (det_tlbr, det_class and out are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_tlbr, 8) || misaligned(det_score, 8) || misaligned(out, 8) || misaligned(slot, 4) ||
        misaligned(problems, 4) || misaligned(status, 4))
        return refuse(BUSCA_MFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    MFrame b;
    b.slot = (const int*)slot, b.free_slot = nullptr, b.problems = (const int*)problems;
    b.S = S, b.n_total = n_total, b.m_total = m_total, b.f_total = f_total, b.N = N, b.M = M;
    CAPI_LAUNCH(who, device, mframe_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles, (unsigned)batch), dim3(256), stream, b, mean, det_tlbr,
                det_score, det_class, out, (int*)status);
    return 0;
}

extern "C" int busca_mframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, const int32_t* row_to_col,
                                  const int32_t* col_to_row, const double* det_xyah, const double* det_score, const uint8_t* det_class,
                                  int32_t m_total, double det_thresh, const int32_t* free_slot, int32_t f_total, const int32_t* problems,
                                  int32_t batch, int32_t N, int32_t M, int32_t* new_slot, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_mframe_apply";
    if (sizes_refused(who, S, n_total, m_total, f_total, batch, N, M, device)) return BUSCA_MFRAME_EINVAL;
    if (det_thresh != det_thresh) return refuse(BUSCA_MFRAME_EINVAL, "%s: det_thresh is NaN", who);
    if (M > BUSCA_MFRAME_MAX_DETS) return refuse(BUSCA_MFRAME_EINVAL, "%s: M = %d detections, one problem takes %d", who, M, BUSCA_MFRAME_MAX_DETS);
    if ((long long)N + M > 2147483647LL) return refuse(BUSCA_MFRAME_EINVAL, "%s: N = %d rows and M = %d columns need more workgroups than a grid holds", who, N, M);
    if (batch == 0 || (N == 0 && M == 0)) return 0;
    const bool rows = N > 0 && n_total > 0, cols = M > 0 && m_total > 0;       // without either, every problem is empty there or skipped
    if (!rows && !cols) return 0;
    if (!mean || !cov) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (mean and cov are required)", who);
    if (!problems) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (rows && (!slot || !row_to_col)) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (slot and row_to_col are required with N > 0)", who);
    if (cols && (!col_to_row || !det_xyah || !det_class || !new_slot))
        return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (col_to_row, det_xyah, det_class and new_slot are required with M > 0)", who);
    if (cols && f_total > 0 && !free_slot) return refuse(BUSCA_MFRAME_EINVAL, "%s: null pointer (free_slot with f_total %d)", who, f_total);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_score, 8) || misaligned(slot, 4) ||
        misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(free_slot, 4) || misaligned(problems, 4) || misaligned(new_slot, 4) ||
        misaligned(status, 4))
        return refuse(BUSCA_MFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    MFrame b;
    b.slot = (const int*)slot, b.free_slot = (const int*)free_slot, b.problems = (const int*)problems;
    b.S = S, b.n_total = n_total, b.m_total = m_total, b.f_total = f_total, b.N = N, b.M = M;
    FrameApply f;
    f.row_to_col = (const int*)row_to_col, f.col_to_row = (const int*)col_to_row;
    f.det_xyah = det_xyah, f.det_score = det_score, f.det_class = det_class;
    f.free_slot = nullptr, f.new_slot = (int*)new_slot, f.status = (int*)status;
    f.det_thresh = det_thresh, f.m = 0, f.n_free = 0;
    CAPI_LAUNCH(who, device, mframe_apply_kernel, dim3((unsigned)((long long)N + M), (unsigned)batch), dim3(64), stream, b, mean, cov, f);
    return 0;
}
