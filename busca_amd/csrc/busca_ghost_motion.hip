// libbusca_hip.so, GHOST motion unit: the position rings, the velocity step and the camera warp of GHOST's linear motion model, and their C-ABI
// (include/busca_ghost_motion.h).  The motion cost itself is busca_pairwise(BUSCA_PAIR_IOU_COST) of the positions the step returns (busca_hip.hip).
#include "busca_internal.hpp"

#pragma GCC visibility push(default)
#include "../../include/busca_ghost_motion.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the motion unit needs IEEE float64 division: build it without -ffast-math"
#endif

#include "ghost_motion_kernel.hip.inc"

static inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the checks every entry point makes of the ring geometry -> BUSCA_OK or the error already recorded
static int motion_dims(busca_ctx* c, const char* who, int32_t S, int32_t H, const char* list, int32_t n) {      // `list`: the caller's name of its list length
    if (S < 0 || H < 0 || n < 0) return fail(c, BUSCA_EINVAL, "%s: negative size (S %d, H %d, %s %d)", who, S, H, list, n);
    if (H < 2) return fail(c, BUSCA_EINVAL, "%s: H = %d, a ring needs at least 2 rows to hold one velocity", who, H);
    return BUSCA_OK;
}

extern "C" int busca_ghost_motion_append(busca_ctx* c, double* hist, int32_t* frames, int32_t* count, int32_t* newest, double* pos, double* vel, int32_t S,
                                         int32_t H, const int32_t* slot, const int32_t* det_index, const uint8_t* reset, int32_t k, const double* boxes,
                                         int32_t m, int32_t frame, void* stream) {
    if (!c) return BUSCA_EINVAL;
    const int rc = motion_dims(c, "busca_ghost_motion_append", S, H, "k", k);
    if (rc != BUSCA_OK) return rc;
    if (m < 0) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_append: negative size (m %d)", m);
    if (k == 0 || S == 0 || m == 0) return BUSCA_OK;
    if (!hist || !frames || !count || !newest || !pos || !vel || !slot || !boxes) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_append: null pointer");
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(boxes, 8) || misaligned(frames, 4) || misaligned(count, 4) ||
        misaligned(newest, 4) || misaligned(slot, 4) || misaligned(det_index, 4))
        return fail(c, BUSCA_EINVAL, "busca_ghost_motion_append: misaligned pointer (8 bytes for float64, 4 for int32)");
    HIP_TRY(c, hipSetDevice(c->device));
    GhostMotionAppendArgs a{{hist, (int*)frames, (int*)count, (int*)newest, pos, vel, S, H}, (const int*)slot, (const int*)det_index, reset, boxes, k, m, frame};
    const int blocks = (int)(((long long)k + GHOST_MOTION_THREADS - 1) / GHOST_MOTION_THREADS);
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_motion_append_kernel, dim3((unsigned)blocks), dim3(GHOST_MOTION_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ghost_motion_warp(busca_ctx* c, double* hist, const int32_t* count, const int32_t* newest, int32_t S, int32_t H, const int32_t* slot,
                                       int32_t n, const float* warp, void* stream) {
    if (!c) return BUSCA_EINVAL;
    const int rc = motion_dims(c, "busca_ghost_motion_warp", S, H, "n", slot ? n : 0);
    if (rc != BUSCA_OK) return rc;
    if (!warp) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_warp: null warp");
    const int listed = slot ? n : S;
    if (listed == 0 || S == 0) return BUSCA_OK;
    if (!hist || !count || !newest) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_warp: null pointer");
    if (misaligned(hist, 8) || misaligned(count, 4) || misaligned(newest, 4) || misaligned(slot, 4) || misaligned(warp, 4))
        return fail(c, BUSCA_EINVAL, "busca_ghost_motion_warp: misaligned pointer (8 bytes for float64, 4 for int32 / float32)");
    const long long blocks = (2LL * listed * H + GHOST_MOTION_THREADS - 1) / GHOST_MOTION_THREADS;
    if (blocks > 0x7fffffffLL) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_warp: %d slots x %d rows need more workgroups than one grid holds", listed, H);
    HIP_TRY(c, hipSetDevice(c->device));
    GhostMotionWarpArgs a{{hist, nullptr, (int*)count, (int*)newest, nullptr, nullptr, S, H}, (const int*)slot, listed, {}};
    for (int i = 0; i < 6; ++i) a.w[i] = (double)warp[i];
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_motion_warp_kernel, dim3((unsigned)blocks), dim3(GHOST_MOTION_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ghost_motion_step(busca_ctx* c, const double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos,
                                       double* vel, int32_t S, int32_t H, const int32_t* slot, int32_t n, int32_t num_active, int32_t last_n_frames,
                                       int32_t diff32, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    const int rc = motion_dims(c, "busca_ghost_motion_step", S, H, "n", n);
    if (rc != BUSCA_OK) return rc;
    if (last_n_frames < 2)
        return fail(c, BUSCA_EINVAL, "busca_ghost_motion_step: last_n_frames = %d; at least 2 (with 1 the reference takes the mean of no velocity, NaN for every track)",
                    last_n_frames);
    if (num_active < 0 || num_active > n) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_step: num_active %d outside 0 .. %d", num_active, n);
    if (n == 0) return BUSCA_OK;
    if (!slot || !out) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_step: null slot / out");
    if (S > 0 && (!hist || !frames || !count || !newest || !pos || !vel)) return fail(c, BUSCA_EINVAL, "busca_ghost_motion_step: null pointer");
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(out, 8) || misaligned(frames, 4) || misaligned(count, 4) ||
        misaligned(newest, 4) || misaligned(slot, 4))
        return fail(c, BUSCA_EINVAL, "busca_ghost_motion_step: misaligned pointer (8 bytes for float64, 4 for int32)");
    HIP_TRY(c, hipSetDevice(c->device));
    GhostMotionStepArgs a{{(double*)hist, (int*)frames, (int*)count, (int*)newest, pos, vel, S, H}, (const int*)slot, out, n, num_active, last_n_frames, diff32 != 0};
    const long long blocks = (4LL * n + GHOST_MOTION_THREADS - 1) / GHOST_MOTION_THREADS;
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(ghost_motion_step_kernel, dim3((unsigned)blocks), dim3(GHOST_MOTION_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}
