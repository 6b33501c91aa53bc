// libbusca_hip.so, GHOST unit: proxy distances, proxy vectors, thresholds and the mask / blend / threshold pass of GHOST's association round, and
// their C-ABI (include/busca_ghost.h).  The distance kernel is built on the tile code of the appearance unit (appear_kernel.hip.inc), included here
// a second time so that both units run the same instructions on a pair.
#include "busca_internal.hpp"

#pragma GCC visibility push(default)
#include "../../include/busca_appearance.h"
#include "../../include/busca_ghost.h"
#pragma GCC visibility pop

#include "appear_kernel.hip.inc"
#include "ghost_kernel.hip.inc"

static inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" int busca_ghost_distance(busca_ctx* c, const float* gallery, const int32_t* slot, const int32_t* count, int32_t n, int32_t budget,
                                    const float* dets, int32_t m, int32_t E, int32_t reduce, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || m < 0) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: negative size (n %d, m %d)", n, m);
    if (budget < 1) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: budget %d, at least 1 row per slot is needed", budget);
    if (E < BUSCA_APPEAR_E_MIN || E > BUSCA_APPEAR_E_MAX || E % 16 != 0)
        return fail(c, BUSCA_EINVAL, "busca_ghost_distance: E = %d is not a multiple of 16 in %d .. %d", E, BUSCA_APPEAR_E_MIN, BUSCA_APPEAR_E_MAX);
    if (reduce < BUSCA_GHOST_MIN || reduce > BUSCA_GHOST_MEDIAN) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: unknown reduce %d", reduce);
    if (reduce == BUSCA_GHOST_MEDIAN && budget > BUSCA_GHOST_MEDIAN_BUDGET_MAX)
        return fail(c, BUSCA_EINVAL, "busca_ghost_distance: MEDIAN stages a track's distances in LDS and takes a budget of at most %d, not %d",
                    BUSCA_GHOST_MEDIAN_BUDGET_MAX, budget);
    if (n == 0 || m == 0) return BUSCA_OK;
    if (!gallery || !dets || !out) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: null pointer");
    if (misaligned(gallery, 16) || misaligned(dets, 16)) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: gallery and dets must be 16-byte aligned");
    if (misaligned(out, 8) || misaligned(slot, 4) || misaligned(count, 4)) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: misaligned out / slot / count");
    const long long mt = ((long long)m + APPEAR_TILE_M - 1) / APPEAR_TILE_M;
    if (mt * n > 0x7fffffffLL) return fail(c, BUSCA_EINVAL, "busca_ghost_distance: %d x %d needs more workgroups than one grid holds", n, m);
    HIP_TRY(c, hipSetDevice(c->device));
    GhostDistArgs a{gallery, (const int*)slot, (const int*)count, dets, out, n, budget, m, E, reduce, (int)mt};
    const dim3 grid((unsigned)(mt * n)), block(64 * APPEAR_WAVES);
    if (reduce == BUSCA_GHOST_MEDIAN) {
        const size_t top = ((size_t)BUSCA_GHOST_MEDIAN_BUDGET_MAX + 2) * APPEAR_TILE_M * sizeof(double);      // the limit is set once per context
        const int rc = ensure_lds(c, (const void*)ghost_distance_kernel<true>, top);
        if (rc != BUSCA_OK) return rc;
        TimedLaunch tl(c, (hipStream_t)stream);
        hipLaunchKernelGGL((ghost_distance_kernel<true>), grid, block, ((size_t)budget + 2) * APPEAR_TILE_M * sizeof(double), (hipStream_t)stream, a);
    } else {
        TimedLaunch tl(c, (hipStream_t)stream);
        hipLaunchKernelGGL((ghost_distance_kernel<false>), grid, block, 0, (hipStream_t)stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ghost_proxies(busca_ctx* c, const float* gallery, const int32_t* slot, const int32_t* count, const int32_t* newest, int32_t n,
                                   int32_t budget, int32_t E, int32_t mode, int32_t window, float* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0) return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: negative size (n %d)", n);
    if (budget < 1) return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: budget %d, at least 1 row per slot is needed", budget);
    if (E < 1) return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: E = %d", E);
    if (mode < BUSCA_GHOST_PROXY_LAST || mode > BUSCA_GHOST_PROXY_MEDIAN) return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: unknown mode %d", mode);
    if (n == 0) return BUSCA_OK;
    if (!gallery || !out) return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: null pointer");
    if (misaligned(gallery, 4) || misaligned(out, 4) || misaligned(slot, 4) || misaligned(count, 4) || misaligned(newest, 4))
        return fail(c, BUSCA_EINVAL, "busca_ghost_proxies: misaligned pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    GhostProxyArgs a{gallery, (const int*)slot, (const int*)count, (const int*)newest, out, n, budget, E, mode, window};
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_proxies_kernel, dim3((unsigned)n), dim3(GHOST_PROXY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ghost_thresholds(busca_ctx* c, const double* cost, int32_t n, int32_t m, int32_t num_active, double k_act, double k_inact,
                                      double* thr_out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || m < 0) return fail(c, BUSCA_EINVAL, "busca_ghost_thresholds: negative size (n %d, m %d)", n, m);
    if (num_active < 0 || num_active > n) return fail(c, BUSCA_EINVAL, "busca_ghost_thresholds: num_active %d outside 0 .. %d", num_active, n);
    if (n == 0 || m == 0) return BUSCA_OK;
    if (!cost || !thr_out) return fail(c, BUSCA_EINVAL, "busca_ghost_thresholds: null pointer");
    if (misaligned(cost, 8) || misaligned(thr_out, 8)) return fail(c, BUSCA_EINVAL, "busca_ghost_thresholds: cost and thr_out must be 8-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_thresholds_kernel, dim3(1), dim3(GHOST_THR_THREADS), 0, (hipStream_t)stream, cost, (long long)num_active * m,
                       (long long)(n - num_active) * m, k_act, k_inact, thr_out);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ghost_combine(busca_ctx* c, const double* app, const double* motion, int32_t n, int32_t m, double alpha, const int32_t* track_label,
                                   const int32_t* det_label, int32_t num_active, const double* thr, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || m < 0) return fail(c, BUSCA_EINVAL, "busca_ghost_combine: negative size (n %d, m %d)", n, m);
    if (alpha != alpha) return fail(c, BUSCA_EINVAL, "busca_ghost_combine: alpha is NaN");
    if ((track_label == nullptr) != (det_label == nullptr)) return fail(c, BUSCA_EINVAL, "busca_ghost_combine: track_label and det_label go together");
    if (n == 0 || m == 0) return BUSCA_OK;
    if (!app || !out) return fail(c, BUSCA_EINVAL, "busca_ghost_combine: null pointer");
    if (misaligned(app, 8) || misaligned(motion, 8) || misaligned(thr, 8) || misaligned(out, 8) || misaligned(track_label, 4) || misaligned(det_label, 4))
        return fail(c, BUSCA_EINVAL, "busca_ghost_combine: misaligned pointer");
    const long long total = (long long)n * m, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(c, BUSCA_EINVAL, "busca_ghost_combine: %d x %d needs more workgroups than one grid holds", n, m);
    HIP_TRY(c, hipSetDevice(c->device));
    GhostCombineArgs a{app, motion, (const int*)track_label, (const int*)det_label, thr, out, total, m, num_active, 1.0 - alpha, alpha};
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}
