// libbusca_hip.so, appearance unit: the cosine gallery-cost kernel and its C-ABI (include/busca_appearance.h).  A unit of its own so that the core
// unit's compile time does not grow (busca_amd/build.py compiles the units in parallel).
#include "busca_internal.hpp"

#pragma GCC visibility push(default)
#include "../../include/busca_appearance.h"
#pragma GCC visibility pop

#include "appear_kernel.hip.inc"

extern "C" int busca_appearance_cost(busca_ctx* c, const float* gallery, const int32_t* slot, const int32_t* count, int32_t n, int32_t budget,
                                     const float* dets, int32_t m, int32_t E, int32_t reduce, int32_t flags, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || m < 0) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: negative size (n %d, m %d)", n, m);
    if (budget < 1) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: budget %d, at least 1 row per slot is needed", budget);
    if (E < BUSCA_APPEAR_E_MIN || E > BUSCA_APPEAR_E_MAX || E % 16 != 0)
        return fail(c, BUSCA_EINVAL, "busca_appearance_cost: E = %d is not a multiple of 16 in %d .. %d", E, BUSCA_APPEAR_E_MIN, BUSCA_APPEAR_E_MAX);
    if (reduce != BUSCA_APPEAR_MIN && reduce != BUSCA_APPEAR_MEAN && reduce != BUSCA_APPEAR_MAX)
        return fail(c, BUSCA_EINVAL, "busca_appearance_cost: unknown reduce %d", reduce);
    if (flags & ~BUSCA_APPEAR_CLAMP0) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: unknown flag bits 0x%x", flags & ~BUSCA_APPEAR_CLAMP0);
    if (n == 0 || m == 0) return BUSCA_OK;
    if (!gallery || !dets || !out) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: null pointer");
    if (((uintptr_t)gallery | (uintptr_t)dets) & 15) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: gallery and dets must be 16-byte aligned");
    const bool plain = budget == 1 && !slot && !count;
    const long long mt = ((long long)m + APPEAR_TILE_M - 1) / APPEAR_TILE_M, rows = plain ? ((long long)n + 15) / 16 : (long long)n;
    if (mt * rows > 0x7fffffffLL) return fail(c, BUSCA_EINVAL, "busca_appearance_cost: %d x %d needs more workgroups than one grid holds", n, m);
    HIP_TRY(c, hipSetDevice(c->device));
    AppearArgs a{gallery, (const int*)slot, (const int*)count, dets, out, n, budget, m, E, reduce, (flags & BUSCA_APPEAR_CLAMP0) ? 1 : 0, (int)mt};
    TimedLaunch tl(c, (hipStream_t)stream);
    const dim3 grid((unsigned)(mt * rows)), block(64 * APPEAR_WAVES);
    if (plain) hipLaunchKernelGGL((appear_kernel<false>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((appear_kernel<true>), grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}
