// libbusca_sort.so: StrongSORT's track state resident on the device and its C-ABI (include/busca_sort.h).  A library of its own, without a busca_ctx, as
// libbusca_track.so is: the interfaces of the other libraries stay what they are.  The device code is sort_kernel.hip.inc on the shared bodies of
// track_kernel.hip.inc (Cholesky factor, gating solve, box conversion) and the slot addressing of kalman_store_kernel.hip.inc - the very text
// libbusca_track.so compiles.  The other kernels those files define come along unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here

#pragma GCC visibility push(default)
#include "../../include/busca_sort.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "sort_kernel.hip.inc"

static_assert(SORT_MC == BUSCA_SORT_MC && SORT_CLAMP == BUSCA_SORT_CLAMP, "sort_kernel.hip.inc and busca_sort.h disagree on the flags");

#define CAPI_EHIP BUSCA_SORT_EHIP
#define CAPI_EINVAL BUSCA_SORT_EINVAL
#define CAPI_STORE_ARGS        // this library's calls take a Kalman store and its slot list
#include "capi_prelude.hpp"

// flags, clamp limit and grid of the two cost matrices -> 0, or the refusal already recorded
static int cost_args(const char* who, int32_t n, int32_t m, int32_t flags, int known, double max_distance, dim3& grid) {
    if (m < 0) return refuse(BUSCA_SORT_EINVAL, "%s: negative size (m %d)", who, m);
    if (flags & ~known) return refuse(BUSCA_SORT_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~known));
    if ((flags & BUSCA_SORT_CLAMP) && max_distance != max_distance) return refuse(BUSCA_SORT_EINVAL, "%s: max_distance is NaN with CLAMP", who);
    const long long row_tiles = ((long long)n + PW_TA - 1) / PW_TA, col_tiles = ((long long)m + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_SORT_EINVAL, "%s: %d tracks need more workgroups than a grid holds (%d at most)", who, n, 65535 * PW_TA);
    grid = dim3((unsigned)col_tiles, (unsigned)row_tiles);
    return 0;
}

extern "C" int busca_sort_version(void) { return 1000; }

extern "C" const char* busca_sort_last_error(void) { return g_err; }

extern "C" int busca_sort_predict(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, int32_t device, void* stream) {
    static const char* who = "busca_sort_predict";
    const int rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc != 0 || n == 0) return rc;
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, sort_predict_kernel, dim3((unsigned)n), dim3(64), stream, k);
    return 0;
}

extern "C" int busca_sort_update(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index,
                                 int32_t m, const double* conf, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_sort_update";
    const int rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc != 0) return rc;
    if (m < 0) return refuse(BUSCA_SORT_EINVAL, "%s: negative size (m %d)", who, m);
    if (n == 0) return 0;
    if (!det_index && n > m) return refuse(BUSCA_SORT_EINVAL, "%s: %d slots for %d measurements and no det_index", who, n, m);
    if (m > 0 && !meas) return refuse(BUSCA_SORT_EINVAL, "%s: null pointer (meas)", who);
    if (misaligned(meas, 8) || misaligned(conf, 8) || misaligned(det_index, 4) || misaligned(status, 4))
        return refuse(BUSCA_SORT_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const KStore k{mean, cov, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, sort_update_kernel, dim3((unsigned)n), dim3(64), stream, k, meas, (const int*)det_index, m, conf, (int*)status);
    return 0;
}

extern "C" int busca_sort_gate_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_xyah, int32_t m,
                                    const double* cost, int32_t ld_cost, double gated_cost, int32_t flags, double lambda, double max_distance,
                                    double* out, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_sort_gate_cost";
    dim3 grid;
    int rc = cost_args(who, n, m, flags, BUSCA_SORT_MC | BUSCA_SORT_CLAMP, max_distance, grid);
    if (rc != 0) return rc;
    if ((flags & BUSCA_SORT_MC) && lambda != lambda) return refuse(BUSCA_SORT_EINVAL, "%s: lambda is NaN with MC", who);
    if (ld_cost < m) return refuse(BUSCA_SORT_EINVAL, "%s: ld_cost %d is below m %d", who, ld_cost, m);
    rc = store_args(who, mean, cov, true, S, slot, n, device);
    if (rc != 0 || n == 0 || m == 0) return rc;
    if (!det_xyah || !cost || !out) return refuse(BUSCA_SORT_EINVAL, "%s: null pointer (det_xyah, cost and out are required)", who);
    if (misaligned(det_xyah, 8) || misaligned(cost, 8) || misaligned(out, 8) || misaligned(status, 4))
        return refuse(BUSCA_SORT_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const KStore k{(double*)mean, (double*)cov, (const int*)slot, S, n};
    SortGate a;
    a.det_xyah = det_xyah, a.cost = cost, a.out = out, a.status = (int*)status;
    a.gated_cost = gated_cost, a.lambda = lambda, a.rest = 1.0 - lambda, a.max_distance = max_distance, a.limit = max_distance + 1e-5;
    a.m = m, a.ld_cost = ld_cost, a.flags = flags;
    CAPI_LAUNCH(who, device, sort_gate_cost_kernel, grid, dim3(256), stream, k, a);
    return 0;
}

extern "C" int busca_sort_iou_cost(const double* mean, int32_t S, const int32_t* slot, int32_t n, const uint8_t* stale, const double* det_tlwh, int32_t m,
                                   int32_t flags, double max_distance, double* out, int32_t device, void* stream) {
    static const char* who = "busca_sort_iou_cost";
    dim3 grid;
    int rc = cost_args(who, n, m, flags, BUSCA_SORT_CLAMP, max_distance, grid);
    if (rc != 0) return rc;
    rc = store_args(who, mean, nullptr, false, S, slot, n, device);
    if (rc != 0 || n == 0 || m == 0) return rc;
    if (!det_tlwh || !out) return refuse(BUSCA_SORT_EINVAL, "%s: null pointer (det_tlwh and out are required)", who);
    if (misaligned(det_tlwh, 8) || misaligned(out, 8)) return refuse(BUSCA_SORT_EINVAL, "%s: misaligned pointer (8 bytes for float64)", who);
    const KStore k{(double*)mean, nullptr, (const int*)slot, S, n};
    SortIou a;
    a.stale = stale, a.det_tlwh = det_tlwh, a.out = out;
    a.max_distance = max_distance, a.limit = max_distance + 1e-5;
    a.m = m, a.flags = flags;
    CAPI_LAUNCH(who, device, sort_iou_cost_kernel, grid, dim3(256), stream, k, a);
    return 0;
}

extern "C" int busca_sort_camera_update(double* mean, int32_t S, const int32_t* slot, int32_t n, const double* matrix, int32_t device, void* stream) {
    static const char* who = "busca_sort_camera_update";
    const int rc = store_args(who, mean, nullptr, false, S, slot, n, device);
    if (rc != 0 || n == 0) return rc;
    if (!matrix) return refuse(BUSCA_SORT_EINVAL, "%s: null pointer (matrix)", who);
    if (misaligned(matrix, 8)) return refuse(BUSCA_SORT_EINVAL, "%s: misaligned pointer (8 bytes for float64)", who);
    const KStore k{mean, nullptr, (const int*)slot, S, n};
    CAPI_LAUNCH(who, device, sort_camera_update_kernel, dim3((unsigned)((n + 255LL) / 256)), dim3(256), stream, k, matrix);
    return 0;
}
