// libbusca_store.so: appearance state resident on the device and its C-ABI (include/busca_store.h).  A library of its own, without a busca_ctx: the
// calls need no weights and no workspace, and the interfaces of libbusca_hip.so and libbusca_track.so stay what they are.  The device code is
// store_kernel.hip.inc; nothing here is shared with the other two libraries.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#pragma GCC visibility push(default)
#include "../../include/busca_store.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the EMA kernel needs IEEE float64 division and square root: build without -ffast-math"
#endif

#include "store_kernel.hip.inc"

#define CAPI_EHIP BUSCA_STORE_EHIP
#include "capi_prelude.hpp"

// the sizes every call has: the slots S, the entries n of its list, the device -> 0, or the refusal already recorded
static int size_args(const char* who, int32_t S, int32_t n, const char* n_name, int32_t device) {
    if (S < 0 || n < 0) return refuse(BUSCA_STORE_EINVAL, "%s: negative size (S %d, %s %d)", who, S, n_name, n);
    if (device < 0) return refuse(BUSCA_STORE_EINVAL, "%s: negative device %d", who, device);
    return 0;
}

// the shape of a slot's rows: `rows` of them (budget or ring), E values each
static int row_args(const char* who, const char* rows_name, int32_t rows, int32_t E) {
    if (rows < 1 || E < 1) return refuse(BUSCA_STORE_EINVAL, "%s: %s %d and E %d: a slot holds at least 1 row of at least 1 value", who, rows_name, rows, E);
    return 0;
}

extern "C" int busca_store_version(void) { return 1000; }

extern "C" const char* busca_store_last_error(void) { return g_err; }

extern "C" int busca_store_ring_add(float* gallery, int32_t* count, int32_t* newest, uint8_t* mv_seen, int32_t S, int32_t budget, int32_t E,
                                    const int32_t* slot, int32_t k, const float* feats, int32_t m, const int32_t* det_index, const uint8_t* is_new,
                                    int32_t device, void* stream) {
    static const char* who = "busca_store_ring_add";
    int rc = size_args(who, S, k, "k", device);
    if (rc != 0) return rc;
    if (m < 0) return refuse(BUSCA_STORE_EINVAL, "%s: negative size (m %d)", who, m);
    if (k == 0) return 0;
    if ((rc = row_args(who, "budget", budget, E)) != 0) return rc;
    if (!det_index && k > m) return refuse(BUSCA_STORE_EINVAL, "%s: %d slots for %d features and no det_index", who, k, m);
    if (!gallery || !count || !newest || !mv_seen || !slot)
        return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (gallery, count, newest, mv_seen and slot are required)", who);
    if (m > 0 && !feats) return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (feats)", who);
    if (misaligned(gallery, 4) || misaligned(count, 4) || misaligned(newest, 4) || misaligned(slot, 4) || misaligned(feats, 4) || misaligned(det_index, 4))
        return refuse(BUSCA_STORE_EINVAL, "%s: misaligned pointer (4 bytes for float32 and int32)", who);
    const StoreRingArgs a{gallery, (int*)count, (int*)newest, mv_seen, (const int*)slot, feats, (const int*)det_index, is_new, S, budget, E, m};
    CAPI_LAUNCH(who, device, store_ring_add_kernel, dim3((unsigned)k), dim3(STORE_THREADS), stream, a);
    return 0;
}

extern "C" int busca_store_release(int32_t* count, uint8_t* mv_seen, int32_t S, const int32_t* slot, int32_t k, int32_t device, void* stream) {
    static const char* who = "busca_store_release";
    const int rc = size_args(who, S, k, "k", device);
    if (rc != 0 || k == 0) return rc;
    if (!count || !mv_seen || !slot) return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (count, mv_seen and slot are required)", who);
    if (misaligned(count, 4) || misaligned(slot, 4)) return refuse(BUSCA_STORE_EINVAL, "%s: misaligned pointer (4 bytes for int32)", who);
    CAPI_LAUNCH(who, device, store_release_kernel, dim3((unsigned)((k + (long long)STORE_THREADS - 1) / STORE_THREADS)), dim3(STORE_THREADS), stream,
                (int*)count, mv_seen, S, (const int*)slot, k);
    return 0;
}

extern "C" int busca_store_mv_avg(const float* gallery, const int32_t* count, const int32_t* newest, float* mv_avg, uint8_t* mv_seen, int32_t S,
                                  int32_t budget, int32_t E, const int32_t* slot, int32_t n, int32_t num_active, double a_act, double a_inact,
                                  float* out, int32_t device, void* stream) {
    static const char* who = "busca_store_mv_avg";
    int rc = size_args(who, S, n, "n", device);
    if (rc != 0) return rc;
    if (num_active < 0 || num_active > n) return refuse(BUSCA_STORE_EINVAL, "%s: num_active %d outside 0 .. %d", who, num_active, n);
    if (a_act != a_act || a_inact != a_inact) return refuse(BUSCA_STORE_EINVAL, "%s: a weight is NaN (a_act %g, a_inact %g)", who, a_act, a_inact);
    if (n == 0) return 0;
    if ((rc = row_args(who, "budget", budget, E)) != 0) return rc;
    if (!gallery || !mv_avg || !mv_seen || !slot || !out)
        return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (gallery, mv_avg, mv_seen, slot and out are required)", who);
    if (misaligned(gallery, 4) || misaligned(count, 4) || misaligned(newest, 4) || misaligned(mv_avg, 4) || misaligned(slot, 4) || misaligned(out, 4))
        return refuse(BUSCA_STORE_EINVAL, "%s: misaligned pointer (4 bytes for float32 and int32)", who);
    // the weights as torch forms them from a Python scalar: the subtraction in float64, each value rounded once to float32
    const StoreMvAvgArgs a{gallery, (const int*)count, (const int*)newest, mv_avg, mv_seen, (const int*)slot, out, S, budget, E, num_active,
                           (float)a_act, (float)(1.0 - a_act), (float)a_inact, (float)(1.0 - a_inact)};
    CAPI_LAUNCH(who, device, store_mv_avg_kernel, dim3((unsigned)n), dim3(STORE_THREADS), stream, a);
    return 0;
}

extern "C" int busca_store_ema_fit(float* gallery, int32_t S, int32_t ring, int32_t E, const float* feats, int32_t m, const int32_t* group_slot,
                                   const int32_t* group_old_row, const int32_t* group_start, const int32_t* src, int32_t g, int32_t k, double alpha,
                                   int32_t device, void* stream) {
    static const char* who = "busca_store_ema_fit";
    int rc = size_args(who, S, g, "g", device);
    if (rc != 0) return rc;
    if (m < 0 || k < 0) return refuse(BUSCA_STORE_EINVAL, "%s: negative size (m %d, k %d)", who, m, k);
    if (alpha != alpha) return refuse(BUSCA_STORE_EINVAL, "%s: alpha is NaN", who);
    if (g == 0) return 0;
    if ((rc = row_args(who, "ring", ring, E)) != 0) return rc;
    if (!gallery || !group_slot || !group_old_row || !group_start)
        return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (gallery, group_slot, group_old_row and group_start are required)", who);
    if ((m > 0 && !feats) || (k > 0 && !src)) return refuse(BUSCA_STORE_EINVAL, "%s: null pointer (feats, src)", who);
    if (misaligned(gallery, 4) || misaligned(feats, 4) || misaligned(group_slot, 4) || misaligned(group_old_row, 4) || misaligned(group_start, 4) ||
        misaligned(src, 4))
        return refuse(BUSCA_STORE_EINVAL, "%s: misaligned pointer (4 bytes for float32 and int32)", who);
    const StoreEmaArgs a{gallery, feats, (const int*)group_slot, (const int*)group_old_row, (const int*)group_start, (const int*)src, S, ring, E, m,
                         k, (float)alpha, (float)(1.0 - alpha)};
    CAPI_LAUNCH(who, device, store_ema_fit_kernel, dim3((unsigned)g), dim3(STORE_THREADS), stream, a);
    return 0;
}
