// libbusca_msframe.so: the StrongSORT frames of many sequences on one resident store and its C-ABI (include/busca_msframe.h).  A library of its own,
// without a busca_ctx, as libbusca_sframe.so and libbusca_mframe.so are: the interfaces of the other libraries stay what they are.  The device code
// is the text libbusca_sframe.so compiles - pairwise_kernel, track_kernel, kalman_store_kernel, sort_kernel, store_kernel and the row, tile, entry and
// column bodies of sframe_kernel.hip.inc - and the tile of appear_kernel.hip.inc that busca_appearance_cost runs, behind the three kernels of
// msframe_kernel.hip.inc.  The other kernels the included files define come along unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here
#include "../../include/busca_appearance.h" // the BUSCA_APPEAR_* codes appear_kernel.hip.inc switches on; declarations only (hidden here)
#include "../../include/busca_sframe.h"     // BUSCA_SFRAME_MAX_DETS and the flags; declarations only (hidden here): no busca_sframe_* function is defined

#pragma GCC visibility push(default)
#include "../../include/busca_msframe.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman, EMA and appearance kernels need IEEE division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "sort_kernel.hip.inc"
#include "store_kernel.hip.inc"
#include "appear_kernel.hip.inc"
#include "sframe_kernel.hip.inc"
#include "msframe_kernel.hip.inc"

static_assert(SORT_MC == BUSCA_MSFRAME_MC && SORT_CLAMP == BUSCA_MSFRAME_CLAMP, "sort_kernel.hip.inc and busca_msframe.h disagree on the flags");
static_assert(BUSCA_MSFRAME_MC == BUSCA_SFRAME_MC && BUSCA_MSFRAME_CLAMP == BUSCA_SFRAME_CLAMP, "one set of flags for both frame libraries");
static_assert(BUSCA_MSFRAME_MAX_DETS == BUSCA_SFRAME_MAX_DETS, "one limit for a problem's detections");
static_assert(BUSCA_MSFRAME_E_MIN == BUSCA_APPEAR_E_MIN && BUSCA_MSFRAME_E_MAX == BUSCA_APPEAR_E_MAX, "the feature widths busca_appearance_cost takes");
static_assert(STORE_THREADS == 256, "sframe_wave_norm restates the norm of a 256-thread store_block_norm");

#define CAPI_EHIP BUSCA_MSFRAME_EHIP
#include "capi_prelude.hpp"

// the sizes all three calls take, judged alike
static int sizes_refused(const char* who, int32_t S, int32_t n_total, int32_t m_total, int32_t f_total, int32_t n_matrices, int32_t batch, int32_t N,
                         int32_t M, int32_t device) {
    if (S < 0 || n_total < 0 || m_total < 0 || f_total < 0 || n_matrices < 0)
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: negative size (S %d, n_total %d, m_total %d, f_total %d, n_matrices %d)", who, S, n_total, m_total,
                      f_total, n_matrices);
    if (batch < 0 || N < 0 || M < 0) return refuse(BUSCA_MSFRAME_EINVAL, "%s: negative size (batch %d, N %d, M %d)", who, batch, N, M);
    if (device < 0) return refuse(BUSCA_MSFRAME_EINVAL, "%s: negative device %d", who, device);
    if (batch > BUSCA_MSFRAME_MAX_BATCH)
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: %d problems are more than a grid holds (%d at most)", who, batch, BUSCA_MSFRAME_MAX_BATCH);
    return 0;
}

static MSFrame table_of(const int32_t* slot, const int32_t* free_slot, const int32_t* problems, const double* matrices, int32_t S, int32_t n_total,
                        int32_t m_total, int32_t f_total, int32_t n_matrices, int32_t N, int32_t M) {
    MSFrame b;
    b.slot = (const int*)slot, b.free_slot = (const int*)free_slot, b.problems = (const int*)problems, b.matrices = matrices;
    b.S = S, b.n_total = n_total, b.m_total = m_total, b.f_total = f_total, b.n_matrices = n_matrices, b.N = N, b.M = M;
    return b;
}

extern "C" int busca_msframe_version(void) { return 1001; }

extern "C" const char* busca_msframe_last_error(void) { return g_err; }

extern "C" int busca_msframe_advance(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total,
                                     const double* matrices, int32_t n_matrices, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                                     int32_t device, void* stream) {
    static const char* who = "busca_msframe_advance";
    if (sizes_refused(who, S, n_total, m_total, f_total, n_matrices, batch, N, M, device)) return BUSCA_MSFRAME_EINVAL;
    if (batch == 0 || N == 0 || n_total == 0) return 0;           // with an empty list every problem is empty or skipped
    if (!mean || !cov || !slot) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (!problems) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (n_matrices > 0 && !matrices) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (matrices with n_matrices %d)", who, n_matrices);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(matrices, 8) || misaligned(slot, 4) || misaligned(problems, 4))
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const MSFrame b = table_of(slot, nullptr, problems, matrices, S, n_total, m_total, f_total, n_matrices, N, M);
    CAPI_LAUNCH(who, device, msframe_advance_kernel, dim3((unsigned)N, (unsigned)batch), dim3(64), stream, b, mean, cov);
    return 0;
}

extern "C" int busca_msframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_xyah,
                                  const double* det_tlwh, const float* det_feat, int32_t m_total, int32_t f_total, int32_t n_matrices,
                                  const uint8_t* stale, const float* feat, int32_t E, double gated_cost, int32_t flags, double mc_lambda,
                                  double max_distance, double max_iou_distance, const int32_t* first, const int32_t* again, int32_t depth,
                                  const int32_t* problems, int32_t batch, int32_t N, int32_t M, double* out, int32_t* status, int32_t device,
                                  void* stream) {
    static const char* who = "busca_msframe_cost";
    if (sizes_refused(who, S, n_total, m_total, f_total, n_matrices, batch, N, M, device)) return BUSCA_MSFRAME_EINVAL;
    if (depth < 0) return refuse(BUSCA_MSFRAME_EINVAL, "%s: negative size (depth %d)", who, depth);
    if (flags & ~(BUSCA_MSFRAME_MC | BUSCA_MSFRAME_CLAMP))
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~(BUSCA_MSFRAME_MC | BUSCA_MSFRAME_CLAMP)));
    if ((flags & BUSCA_MSFRAME_MC) && mc_lambda != mc_lambda) return refuse(BUSCA_MSFRAME_EINVAL, "%s: mc_lambda is NaN with MC", who);
    if ((flags & BUSCA_MSFRAME_CLAMP) && max_distance != max_distance) return refuse(BUSCA_MSFRAME_EINVAL, "%s: max_distance is NaN with CLAMP", who);
    if (max_iou_distance != max_iou_distance) return refuse(BUSCA_MSFRAME_EINVAL, "%s: max_iou_distance is NaN", who);
    if (E < BUSCA_MSFRAME_E_MIN || E > BUSCA_MSFRAME_E_MAX || E % 16)
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: E %d: a feature row holds a multiple of 16 values in %d .. %d", who, E, BUSCA_MSFRAME_E_MIN, BUSCA_MSFRAME_E_MAX);
    const long long row_tiles = ((long long)N + PW_TA - 1) / PW_TA, col_tiles = ((long long)M + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_MSFRAME_EINVAL, "%s: N = %d tracks need more workgroups than a grid holds (%d at most)", who, N, 65535 * PW_TA);
    if (batch == 0 || N == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;      // with an empty list every problem is empty or skipped
    if (!mean || !cov || !slot) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (!problems) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (!det_xyah || !det_tlwh || !det_feat || !feat || !first || !out)
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (det_xyah, det_tlwh, det_feat, feat, first and out are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_tlwh, 8) || misaligned(out, 8) || misaligned(slot, 4) ||
        misaligned(first, 4) || misaligned(again, 4) || misaligned(problems, 4) || misaligned(status, 4))
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    if (misaligned(feat, 16) || misaligned(det_feat, 16))
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: misaligned pointer (16 bytes for feat and det_feat: rows are loaded four values at a time)", who);
    const MSFrame b = table_of(slot, nullptr, problems, nullptr, S, n_total, m_total, f_total, n_matrices, N, M);
    SFrameCost a;
    a.det_xyah = det_xyah, a.det_tlwh = det_tlwh, a.stale = stale, a.cost = nullptr;
    a.first = (const int*)first, a.again = (const int*)again, a.out = out, a.status = (int*)status;
    a.gated_cost = gated_cost, a.lambda = mc_lambda, a.rest = 1.0 - mc_lambda, a.max_distance = max_distance, a.limit = max_distance + 1e-5;
    a.max_iou = max_iou_distance, a.iou_limit = max_iou_distance + 1e-5;
    a.m = 0, a.ld_cost = 0, a.flags = flags, a.depth = depth;
    CAPI_LAUNCH(who, device, msframe_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles, (unsigned)batch), dim3(256), stream, b, mean, cov, a,
                feat, det_feat, (int)E);
    return 0;
}

extern "C" int busca_msframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, const int32_t* row_to_col,
                                   const int32_t* col_to_row, const double* det_xyah, const double* det_conf, const float* det_feat, int32_t m_total,
                                   float* feat, int32_t E, double alpha, const int32_t* free_slot, int32_t f_total, int32_t n_matrices,
                                   const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t* new_slot, int32_t* status, int32_t device,
                                   void* stream) {
    static const char* who = "busca_msframe_apply";
    if (sizes_refused(who, S, n_total, m_total, f_total, n_matrices, batch, N, M, device)) return BUSCA_MSFRAME_EINVAL;
    if (alpha != alpha) return refuse(BUSCA_MSFRAME_EINVAL, "%s: alpha is NaN", who);
    if (M > BUSCA_MSFRAME_MAX_DETS) return refuse(BUSCA_MSFRAME_EINVAL, "%s: M = %d detections, one problem takes %d", who, M, BUSCA_MSFRAME_MAX_DETS);
    if ((long long)N + M > 2147483647LL) return refuse(BUSCA_MSFRAME_EINVAL, "%s: N = %d rows and M = %d columns need more workgroups than a grid holds", who, N, M);
    if (batch == 0 || M == 0 || m_total == 0) return 0;           // without a detection no row has a match and no column is there
    if (E < 1) return refuse(BUSCA_MSFRAME_EINVAL, "%s: E %d: a feature row holds at least 1 value", who, E);
    const bool rows = N > 0 && n_total > 0;
    if (!mean || !cov || !feat) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (mean, cov and feat are required)", who);
    if (!problems) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (rows && (!slot || !row_to_col)) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (slot and row_to_col are required with N > 0)", who);
    if (!col_to_row || !det_xyah || !det_feat || !new_slot)
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (col_to_row, det_xyah, det_feat and new_slot are required with M > 0)", who);
    if (f_total > 0 && !free_slot) return refuse(BUSCA_MSFRAME_EINVAL, "%s: null pointer (free_slot with f_total %d)", who, f_total);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_conf, 8) || misaligned(det_feat, 4) ||
        misaligned(feat, 4) || misaligned(slot, 4) || misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(free_slot, 4) ||
        misaligned(problems, 4) || misaligned(new_slot, 4) || misaligned(status, 4))
        return refuse(BUSCA_MSFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    const MSFrame b = table_of(slot, free_slot, problems, nullptr, S, n_total, m_total, f_total, n_matrices, N, M);
    SFrameApply f;
    f.row_to_col = (const int*)row_to_col, f.col_to_row = (const int*)col_to_row;
    f.det_xyah = det_xyah, f.det_conf = det_conf, f.det_feat = det_feat, f.feat = feat;
    f.free_slot = nullptr, f.new_slot = (int*)new_slot, f.status = (int*)status;
    f.wa = (float)alpha, f.wb = (float)(1.0 - alpha);      // as busca_store_ema_fit forms them: the subtraction in float64, each rounded once
    f.m = 0, f.E = E, f.n_free = 0;
    CAPI_LAUNCH(who, device, msframe_apply_kernel, dim3((unsigned)((long long)N + M), (unsigned)batch), dim3(64), stream, b, mean, cov, f);
    return 0;
}
