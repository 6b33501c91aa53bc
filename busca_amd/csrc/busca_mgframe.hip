// libbusca_mgframe.so: the GHOST frames of many sequences on one resident store and its C-ABI (include/busca_mgframe.h).  A library of its own,
// without a busca_ctx, as libbusca_gframe.so and libbusca_msframe.so are: the interfaces of the other libraries stay what they are.  The device code
// is the text libbusca_gframe.so compiles - pairwise_kernel, appear_kernel, ghost_kernel (with ghost_body), ghost_motion_kernel, store_kernel and
// gframe_kernel (with gframe_body) - behind the six kernels of mgframe_kernel.hip.inc.  The other kernels the included files define come along
// unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here
#include "../../include/busca_appearance.h" // the BUSCA_APPEAR_* codes appear_kernel.hip.inc switches on; declarations only (hidden here)
#include "../../include/busca_ghost.h"      // the BUSCA_GHOST_* codes ghost_kernel.hip.inc switches on; declarations only (hidden here)
#include "../../include/busca_gframe.h"     // BUSCA_GFRAME_MAX_DETS; declarations only (hidden here): no busca_gframe_* function is defined

#pragma GCC visibility push(default)
#include "../../include/busca_mgframe.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the motion step and the IoU need IEEE float64 division: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "appear_kernel.hip.inc"
#include "ghost_kernel.hip.inc"
#include "ghost_motion_kernel.hip.inc"
#include "store_kernel.hip.inc"
#include "gframe_kernel.hip.inc"
#include "mgframe_kernel.hip.inc"

static_assert(MGFRAME_WORDS == BUSCA_MGFRAME_PROBLEM_WORDS && MGFRAME_DIFF32 == BUSCA_MGFRAME_DIFF32 && MGFRAME_STEP == BUSCA_MGFRAME_STEP,
              "mgframe_kernel.hip.inc and busca_mgframe.h disagree on the problem table");
static_assert(BUSCA_MGFRAME_MAX_DETS == BUSCA_GFRAME_MAX_DETS, "one limit for a problem's detections");
static_assert(BUSCA_MGFRAME_E_MIN == BUSCA_APPEAR_E_MIN && BUSCA_MGFRAME_E_MAX == BUSCA_APPEAR_E_MAX, "the feature widths busca_ghost_distance takes");
static_assert(BUSCA_MGFRAME_MEDIAN_BUDGET_MAX == BUSCA_GHOST_MEDIAN_BUDGET_MAX, "one budget limit for MEDIAN");

#define CAPI_EHIP BUSCA_MGFRAME_EHIP
#include "capi_prelude.hpp"

// what every call takes, judged alike
struct Sizes {
    int32_t S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row;
};

static int sizes_refused(const char* who, const Sizes& z, int32_t device) {
    if (z.S < 0 || z.n_total < 0 || z.m_total < 0 || z.f_total < 0 || z.n_warps < 0)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: negative size (S %d, n_total %d, m_total %d, f_total %d, n_warps %d)", who, z.S, z.n_total, z.m_total,
                      z.f_total, z.n_warps);
    if (z.batch < 0 || z.N < 0 || z.M < 0 || z.L < 0 || z.R < 0)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: negative size (batch %d, N %d, M %d, L %d, R %d)", who, z.batch, z.N, z.M, z.L, z.R);
    if (device < 0) return refuse(BUSCA_MGFRAME_EINVAL, "%s: negative device %d", who, device);
    if (z.batch > BUSCA_MGFRAME_MAX_BATCH)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: %d problems are more than a grid holds (%d at most)", who, z.batch, BUSCA_MGFRAME_MAX_BATCH);
    if (z.R > BUSCA_MGFRAME_MAX_ROWS || z.L > BUSCA_MGFRAME_MAX_ROWS)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: R %d or L %d rows are more than a grid holds (%d at most)", who, z.R, z.L, BUSCA_MGFRAME_MAX_ROWS);
    if (z.inact_row > z.R) return refuse(BUSCA_MGFRAME_EINVAL, "%s: inact_row %d beyond the slab's %d rows", who, z.inact_row, z.R);
    return 0;
}

static MGFrame table_of(const Sizes& z, const int32_t* slot, const int32_t* free_slot, const int32_t* problems, const float* warps) {
    MGFrame b;
    b.slot = (const int*)slot, b.free_slot = (const int*)free_slot, b.problems = (const int*)problems, b.warps = warps;
    b.S = z.S, b.n_total = z.n_total, b.m_total = z.m_total, b.f_total = z.f_total, b.n_warps = z.n_warps, b.N = z.N, b.M = z.M, b.L = z.L, b.R = z.R;
    b.inact_row = z.inact_row < 0 ? -1 : z.inact_row;
    return b;
}

extern "C" int busca_mgframe_version(void) { return 1000; }

extern "C" const char* busca_mgframe_last_error(void) { return g_err; }

extern "C" int busca_mgframe_advance(double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos, double* vel, int32_t S,
                                     int32_t H, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total, const float* warps,
                                     int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R,
                                     int32_t inact_row, int32_t last_n_frames, double* pos_out, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_advance";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (H < 2) return refuse(BUSCA_MGFRAME_EINVAL, "%s: H = %d, a ring needs at least 2 rows to hold one velocity", who, H);
    if (last_n_frames < 2)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: last_n_frames = %d; at least 2 (with 1 the reference takes the mean of no velocity)", who, last_n_frames);
    if (batch == 0 || L == 0 || n_total == 0) return 0;           // with an empty list every problem is empty or skipped
    if (!hist || !frames || !count || !newest || !pos || !vel || !slot || !pos_out)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (hist, frames, count, newest, pos, vel, slot and pos_out are required)", who);
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (n_warps > 0 && !warps) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (warps with n_warps %d)", who, n_warps);
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(pos_out, 8) || misaligned(frames, 4) || misaligned(count, 4) ||
        misaligned(newest, 4) || misaligned(slot, 4) || misaligned(warps, 4) || misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    const MGFrame b = table_of(z, slot, nullptr, problems, warps);
    const GhostMotionRings r{hist, (int*)frames, (int*)count, (int*)newest, pos, vel, S, H};
    CAPI_SCOPE(who, device);
    CAPI_LAUNCH_IN_SCOPE(who, mgframe_advance_kernel, dim3((unsigned)L, (unsigned)batch), dim3(64), 0, stream, b, r, (int)last_n_frames, pos_out);
    return 0;
}

extern "C" int busca_mgframe_distance(const float* gallery, const int32_t* count, int32_t rows, int32_t by_list, int32_t budget, const float* dets,
                                      int32_t E, int32_t reduce, int32_t groups, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total,
                                      int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L,
                                      int32_t R, int32_t inact_row, double* out, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_distance";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (rows < 0) return refuse(BUSCA_MGFRAME_EINVAL, "%s: negative size (rows %d)", who, rows);
    if (budget < 1) return refuse(BUSCA_MGFRAME_EINVAL, "%s: budget %d, at least 1 row per slot is needed", who, budget);
    if (E < BUSCA_MGFRAME_E_MIN || E > BUSCA_MGFRAME_E_MAX || E % 16)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: E %d: a feature row holds a multiple of 16 values in %d .. %d", who, E, BUSCA_MGFRAME_E_MIN, BUSCA_MGFRAME_E_MAX);
    if (reduce < BUSCA_GHOST_MIN || reduce > BUSCA_GHOST_MEDIAN) return refuse(BUSCA_MGFRAME_EINVAL, "%s: unknown reduce %d", who, reduce);
    if (reduce == BUSCA_GHOST_MEDIAN && budget > BUSCA_MGFRAME_MEDIAN_BUDGET_MAX)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: MEDIAN stages a track's distances in LDS and takes a budget of at most %d, not %d", who,
                      BUSCA_MGFRAME_MEDIAN_BUDGET_MAX, budget);
    if (groups < 1 || groups > 3) return refuse(BUSCA_MGFRAME_EINVAL, "%s: groups %d outside 1 .. 3", who, groups);
    if (by_list && rows != n_total)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: a table indexed as the slot list has n_total = %d rows, not %d", who, n_total, rows);
    if (batch == 0 || R == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;
    if (!gallery || !dets || !out) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (gallery, dets and out are required)", who);
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (!by_list && !slot) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (slot, without by_list)", who);
    if (misaligned(gallery, 16) || misaligned(dets, 16))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (16 bytes for gallery and dets: rows are loaded four values at a time)", who);
    if (misaligned(out, 8) || misaligned(count, 4) || misaligned(slot, 4) || misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    const MGFrame b = table_of(z, slot, nullptr, problems, nullptr);
    const MGFrameDist d{gallery, (const int*)count, dets, out, rows, by_list != 0, budget, E, reduce, groups};
    const dim3 grid((unsigned)(((long long)M + APPEAR_TILE_M - 1) / APPEAR_TILE_M), (unsigned)R, (unsigned)batch), block(64 * APPEAR_WAVES);
    CAPI_SCOPE(who, device);
    if (reduce == BUSCA_GHOST_MEDIAN) {
        const size_t top = ((size_t)BUSCA_MGFRAME_MEDIAN_BUDGET_MAX + 2) * APPEAR_TILE_M * sizeof(double);
        const hipError_t e = hipFuncSetAttribute((const void*)mgframe_distance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)top);
        if (e != hipSuccess) return refuse(BUSCA_MGFRAME_EHIP, "%s: %s", who, hipGetErrorString(e));
        CAPI_LAUNCH_IN_SCOPE(who, (mgframe_distance_kernel<true>), grid, block, ((size_t)budget + 2) * APPEAR_TILE_M * sizeof(double), stream, b, d);
    } else {
        CAPI_LAUNCH_IN_SCOPE(who, (mgframe_distance_kernel<false>), grid, block, 0, stream, b, d);
    }
    return 0;
}

extern "C" int busca_mgframe_thresholds(const double* cost, double k_act, double k_inact, int32_t which, int32_t S, const int32_t* slot, int32_t n_total,
                                        int32_t m_total, int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                                        int32_t L, int32_t R, int32_t inact_row, double* thr, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_thresholds";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (which < 1 || which > 3) return refuse(BUSCA_MGFRAME_EINVAL, "%s: which %d outside 1 .. 3", who, which);
    if (batch == 0 || R == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;
    if (!cost || !thr) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (cost and thr are required)", who);
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (misaligned(cost, 8) || misaligned(thr, 8) || misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    (void)slot;
    const MGFrame b = table_of(z, nullptr, nullptr, problems, nullptr);
    CAPI_SCOPE(who, device);
    CAPI_LAUNCH_IN_SCOPE(who, mgframe_thresholds_kernel, dim3((unsigned)batch), dim3(GHOST_THR_THREADS), 0, stream, b, cost, k_act, k_inact, (int)which, thr);
    return 0;
}

extern "C" int busca_mgframe_cost(double* cost, const double* pos, const double* det_boxes, double alpha, const int32_t* track_label,
                                  const int32_t* det_label, const double* thr, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total,
                                  int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R,
                                  int32_t inact_row, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_cost";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (alpha != alpha) return refuse(BUSCA_MGFRAME_EINVAL, "%s: alpha is NaN", who);
    if ((track_label == nullptr) != (det_label == nullptr)) return refuse(BUSCA_MGFRAME_EINVAL, "%s: track_label and det_label go together", who);
    if (batch == 0 || R == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;
    if (!cost) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (cost)", who);
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (pos && !det_boxes) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (det_boxes with pos)", who);
    if (misaligned(cost, 8) || misaligned(pos, 8) || misaligned(det_boxes, 8) || misaligned(thr, 8) || misaligned(track_label, 4) ||
        misaligned(det_label, 4) || misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    (void)slot;
    const MGFrame b = table_of(z, nullptr, nullptr, problems, nullptr);
    GFrameCost a;
    a.app = cost, a.pos = pos, a.boxes = det_boxes, a.tlabel = (const int*)track_label, a.dlabel = (const int*)det_label, a.thr = thr, a.out = cost;
    a.w_app = 1.0 - alpha, a.w_motion = alpha;                    // as busca_ghost_combine forms them
    a.rows = GFrameRows{0, 0, 0, 0, 0}, a.m = 0, a.ld = 0;        // the problem's: set by the kernel
    const dim3 grid((unsigned)(((long long)M + PW_TB - 1) / PW_TB), (unsigned)(((long long)R + PW_TA - 1) / PW_TA), (unsigned)batch);
    CAPI_SCOPE(who, device);
    CAPI_LAUNCH_IN_SCOPE(who, mgframe_cost_kernel, grid, dim3(256), 0, stream, b, a);
    return 0;
}

extern "C" int busca_mgframe_keep(double* cost, const int32_t* row_to_col, const int32_t* col_to_row, const double* thr, int32_t* track_det,
                                  int32_t* det_track, int32_t stage, int32_t merge, int32_t mask, int32_t S, const int32_t* slot, int32_t n_total,
                                  int32_t m_total, int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                                  int32_t L, int32_t R, int32_t inact_row, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_keep";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (stage < 0 || stage > 2) return refuse(BUSCA_MGFRAME_EINVAL, "%s: stage %d outside 0 .. 2", who, stage);
    if (mask && stage != 1) return refuse(BUSCA_MGFRAME_EINVAL, "%s: the mask goes with stage 1 (the rows it writes lie behind the rows that are read)", who);
    if (batch == 0 || M == 0 || m_total == 0) return 0;
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    if (!det_track || !col_to_row) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (col_to_row and det_track are required)", who);
    if (R > 0 && (!cost || !row_to_col || !thr || !track_det))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (cost, row_to_col, thr and track_det are required with rows)", who);
    if (misaligned(cost, 8) || misaligned(thr, 8) || misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(track_det, 4) ||
        misaligned(det_track, 4) || misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    (void)slot;
    const MGFrame b = table_of(z, nullptr, nullptr, problems, nullptr);
    GFrameKeep a;
    a.cost = cost, a.row_to_col = (const int*)row_to_col, a.col_to_row = (const int*)col_to_row, a.thr = thr;
    a.track_det = (int*)track_det, a.det_track = (int*)det_track;
    a.m = 0, a.ld = 0, a.lo = 0, a.hi = 0, a.num_active = 0, a.merge = merge != 0, a.mask_from = -1, a.mask_to = 0;      // the rest is the problem's
    const int threads = R > M ? R : M;
    CAPI_SCOPE(who, device);
    CAPI_LAUNCH_IN_SCOPE(who, mgframe_keep_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)batch), dim3(256), 0, stream, b, a, (int)stage,
                         (int)(mask != 0));
    return 0;
}

extern "C" int busca_mgframe_apply(double* hist, int32_t* frames, int32_t* m_count, int32_t* m_newest, double* pos, double* vel, int32_t H,
                                   float* gallery, int32_t* g_count, int32_t* g_newest, uint8_t* mv_seen, int32_t budget, int32_t E,
                                   const int32_t* track_det, const int32_t* det_track, const float* det_feat, const double* det_boxes,
                                   const uint8_t* may_start, const int32_t* free_slot, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total,
                                   int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R,
                                   int32_t inact_row, int32_t* det_slot, int32_t device, void* stream) {
    static const char* who = "busca_mgframe_apply";
    const Sizes z{S, n_total, m_total, f_total, n_warps, batch, N, M, L, R, inact_row};
    if (sizes_refused(who, z, device)) return BUSCA_MGFRAME_EINVAL;
    if (H < 0) return refuse(BUSCA_MGFRAME_EINVAL, "%s: negative size (H %d)", who, H);
    if (M > BUSCA_MGFRAME_MAX_DETS) return refuse(BUSCA_MGFRAME_EINVAL, "%s: M = %d detections, one problem takes %d", who, M, BUSCA_MGFRAME_MAX_DETS);
    if (batch == 0 || M == 0 || m_total == 0) return 0;           // without a detection nothing is assigned
    if (H < 2) return refuse(BUSCA_MGFRAME_EINVAL, "%s: H = %d, a ring needs at least 2 rows to hold one velocity", who, H);
    if (budget < 1 || E < 1) return refuse(BUSCA_MGFRAME_EINVAL, "%s: budget %d and E %d: a slot holds at least 1 row of at least 1 value", who, budget, E);
    if (!hist || !frames || !m_count || !m_newest || !pos || !vel)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (the motion state: hist, frames, m_count, m_newest, pos and vel are required)", who);
    if (!gallery || !g_count || !g_newest || !mv_seen)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (the feature rings: gallery, g_count, g_newest and mv_seen are required)", who);
    if (!problems) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (problems)", who);
    const bool rows = R > 0 && n_total > 0;
    if (rows && (!slot || !track_det)) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (slot and track_det are required with rows)", who);
    if (!det_track || !det_feat || !det_boxes || !may_start || !det_slot)
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (det_track, det_feat, det_boxes, may_start and det_slot are required)", who);
    if (f_total > 0 && !free_slot) return refuse(BUSCA_MGFRAME_EINVAL, "%s: null pointer (free_slot with f_total %d)", who, f_total);
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(det_boxes, 8) || misaligned(frames, 4) || misaligned(m_count, 4) ||
        misaligned(m_newest, 4) || misaligned(gallery, 4) || misaligned(g_count, 4) || misaligned(g_newest, 4) || misaligned(slot, 4) ||
        misaligned(track_det, 4) || misaligned(det_track, 4) || misaligned(det_feat, 4) || misaligned(free_slot, 4) || misaligned(det_slot, 4) ||
        misaligned(problems, 4))
        return refuse(BUSCA_MGFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    const MGFrame b = table_of(z, slot, free_slot, problems, nullptr);      // without rows no problem has a track: no row workgroup reads slot
    GFrameApply f;
    f.r = GhostMotionRings{hist, (int*)frames, (int*)m_count, (int*)m_newest, pos, vel, S, H};
    f.gallery = gallery, f.g_count = (int*)g_count, f.g_newest = (int*)g_newest, f.mv_seen = mv_seen;
    f.slot = (const int*)slot, f.track_det = (const int*)track_det, f.det_track = (const int*)det_track;
    f.det_feat = det_feat, f.det_boxes = det_boxes, f.may_start = may_start, f.free_slot = nullptr, f.det_slot = (int*)det_slot;
    f.rows = GFrameRows{0, 0, 0, 0, 0}, f.m = 0, f.budget = budget, f.E = E, f.frame = 0, f.n_free = 0;      // rows, m, frame and n_free are the problem's
    CAPI_SCOPE(who, device);
    CAPI_LAUNCH_IN_SCOPE(who, mgframe_apply_kernel, dim3((unsigned)(b.R + M), (unsigned)batch), dim3(64), 0, stream, b, f);
    return 0;
}
