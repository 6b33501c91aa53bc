// libbusca_sframe.so: a StrongSORT frame on resident track state and its C-ABI (include/busca_sframe.h).  A library of its own, without a busca_ctx, as
// libbusca_sort.so and libbusca_frame.so are: the interfaces of the other libraries stay what they are.  The device code is the per-track bodies of
// track_kernel.hip.inc and sort_kernel.hip.inc, the addressing of kalman_store_kernel.hip.inc and the float32 arithmetic of store_kernel.hip.inc - the
// very text libbusca_sort.so and libbusca_store.so compile - behind the three kernels of sframe_kernel.hip.inc.  The other kernels the included files
// define come along unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here

#pragma GCC visibility push(default)
#include "../../include/busca_sframe.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman and EMA kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "sort_kernel.hip.inc"
#include "store_kernel.hip.inc"
#include "sframe_kernel.hip.inc"

static_assert(SORT_MC == BUSCA_SFRAME_MC && SORT_CLAMP == BUSCA_SFRAME_CLAMP, "sort_kernel.hip.inc and busca_sframe.h disagree on the flags");
static_assert(STORE_THREADS == 256, "sframe_wave_norm restates the norm of a 256-thread store_block_norm");

#define CAPI_EHIP BUSCA_SFRAME_EHIP
#include "capi_prelude.hpp"

extern "C" int busca_sframe_version(void) { return 1001; }

extern "C" const char* busca_sframe_last_error(void) { return g_err; }

extern "C" int busca_sframe_advance(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* matrix, int32_t device,
                                    void* stream) {
    static const char* who = "busca_sframe_advance";
    if (S < 0 || n < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative size (S %d, n %d)", who, S, n);
    if (device < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative device %d", who, device);
    if (n == 0) return 0;
    if (!mean || !cov || !slot) return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(matrix, 8) || misaligned(slot, 4))
        return refuse(BUSCA_SFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, sframe_advance_kernel, dim3((unsigned)n), dim3(64), stream, k, matrix);
    return 0;
}

extern "C" int busca_sframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_xyah,
                                 const double* det_tlwh, int32_t m, const uint8_t* stale, const double* cost, int32_t ld_cost, double gated_cost,
                                 int32_t flags, double mc_lambda, double max_distance, double max_iou_distance, const int32_t* first,
                                 const int32_t* again, int32_t depth, double* out, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_sframe_cost";
    if (S < 0 || n < 0 || m < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative size (S %d, n %d, m %d)", who, S, n, m);
    if (depth < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative size (depth %d)", who, depth);
    if (device < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative device %d", who, device);
    if (flags & ~(BUSCA_SFRAME_MC | BUSCA_SFRAME_CLAMP))
        return refuse(BUSCA_SFRAME_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~(BUSCA_SFRAME_MC | BUSCA_SFRAME_CLAMP)));
    if ((flags & BUSCA_SFRAME_MC) && mc_lambda != mc_lambda) return refuse(BUSCA_SFRAME_EINVAL, "%s: mc_lambda is NaN with MC", who);
    if ((flags & BUSCA_SFRAME_CLAMP) && max_distance != max_distance) return refuse(BUSCA_SFRAME_EINVAL, "%s: max_distance is NaN with CLAMP", who);
    if (max_iou_distance != max_iou_distance) return refuse(BUSCA_SFRAME_EINVAL, "%s: max_iou_distance is NaN", who);
    if (ld_cost < m) return refuse(BUSCA_SFRAME_EINVAL, "%s: ld_cost %d is below m %d", who, ld_cost, m);
    const long long row_tiles = ((long long)n + PW_TA - 1) / PW_TA, col_tiles = ((long long)m + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_SFRAME_EINVAL, "%s: %d tracks need more workgroups than a grid holds (%d at most)", who, n, 65535 * PW_TA);
    if (n == 0 || m == 0) return 0;
    if (!mean || !cov || !slot) return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (!det_xyah || !det_tlwh || !cost || !first || !out)
        return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (det_xyah, det_tlwh, cost, first and out are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_tlwh, 8) || misaligned(cost, 8) || misaligned(out, 8) ||
        misaligned(slot, 4) || misaligned(first, 4) || misaligned(again, 4) || misaligned(status, 4))
        return refuse(BUSCA_SFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    if ((const double*)out == cost) return refuse(BUSCA_SFRAME_EINVAL, "%s: out must not be cost (a lane reads entries of cost that other lanes' plane writes)", who);
    const KStore k{(double*)mean, (double*)cov, (const int*)slot, S, n};
    SFrameCost a;
    a.det_xyah = det_xyah, a.det_tlwh = det_tlwh, a.stale = stale, a.cost = cost;
    a.first = (const int*)first, a.again = (const int*)again, a.out = out, a.status = (int*)status;
    a.gated_cost = gated_cost, a.lambda = mc_lambda, a.rest = 1.0 - mc_lambda, a.max_distance = max_distance, a.limit = max_distance + 1e-5;
    a.max_iou = max_iou_distance, a.iou_limit = max_iou_distance + 1e-5;
    a.m = m, a.ld_cost = ld_cost, a.flags = flags, a.depth = depth;
    CAPI_LAUNCH(who, device, sframe_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles), dim3(256), stream, k, a);
    return 0;
}

extern "C" int busca_sframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const int32_t* row_to_col,
                                  const int32_t* col_to_row, const double* det_xyah, const double* det_conf, const float* det_feat, int32_t m,
                                  float* feat, int32_t E, double alpha, const int32_t* free_slot, int32_t n_free, int32_t* new_slot, int32_t* status,
                                  int32_t device, void* stream) {
    static const char* who = "busca_sframe_apply";
    if (S < 0 || n < 0 || m < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative size (S %d, n %d, m %d)", who, S, n, m);
    if (n_free < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative size (n_free %d)", who, n_free);
    if (device < 0) return refuse(BUSCA_SFRAME_EINVAL, "%s: negative device %d", who, device);
    if (alpha != alpha) return refuse(BUSCA_SFRAME_EINVAL, "%s: alpha is NaN", who);
    if (m > BUSCA_SFRAME_MAX_DETS) return refuse(BUSCA_SFRAME_EINVAL, "%s: %d detections, one call takes %d", who, m, BUSCA_SFRAME_MAX_DETS);
    if ((long long)n + m > 2147483647LL) return refuse(BUSCA_SFRAME_EINVAL, "%s: %d rows and %d columns need more workgroups than a grid holds", who, n, m);
    if (n == 0 && m == 0) return 0;
    if (E < 1) return refuse(BUSCA_SFRAME_EINVAL, "%s: E %d: a feature row holds at least 1 value", who, E);
    if (!mean || !cov || !feat) return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (mean, cov and feat are required)", who);
    if (n > 0 && (!slot || !row_to_col)) return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (slot and row_to_col are required with n > 0)", who);
    if (m > 0 && (!col_to_row || !det_xyah || !det_feat || !new_slot))
        return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (col_to_row, det_xyah, det_feat and new_slot are required with m > 0)", who);
    if (m > 0 && n_free > 0 && !free_slot) return refuse(BUSCA_SFRAME_EINVAL, "%s: null pointer (free_slot with n_free %d)", who, n_free);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_xyah, 8) || misaligned(det_conf, 8) || misaligned(det_feat, 4) ||
        misaligned(feat, 4) || misaligned(slot, 4) || misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(free_slot, 4) ||
        misaligned(new_slot, 4) || misaligned(status, 4))
        return refuse(BUSCA_SFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    const KStore k{mean, cov, (const int*)slot, S, n};
    SFrameApply f;
    f.row_to_col = (const int*)row_to_col, f.col_to_row = (const int*)col_to_row;
    f.det_xyah = det_xyah, f.det_conf = det_conf, f.det_feat = det_feat, f.feat = feat;
    f.free_slot = (const int*)free_slot, f.new_slot = (int*)new_slot, f.status = (int*)status;
    f.wa = (float)alpha, f.wb = (float)(1.0 - alpha);      // as busca_store_ema_fit forms them: the subtraction in float64, each rounded once
    f.m = m, f.E = E, f.n_free = n_free;
    CAPI_LAUNCH(who, device, sframe_apply_kernel, dim3((unsigned)((long long)n + m)), dim3(64), stream, k, f);
    return 0;
}
