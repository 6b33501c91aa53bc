// libbusca_gframe.so: a GHOST frame on resident track state and its C-ABI (include/busca_gframe.h).  A library of its own, without a busca_ctx, as
// libbusca_store.so and libbusca_sframe.so are: the interfaces of the other libraries stay what they are.  The device code is the per-entry bodies of
// ghost_motion_kernel.hip.inc, pairwise_kernel.hip.inc, ghost_kernel.hip.inc and store_kernel.hip.inc - the very text libbusca_hip.so and
// libbusca_store.so compile - behind the four kernels of gframe_kernel.hip.inc.  The other kernels the included files define come along unused
// (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here
#include "../../include/busca_appearance.h" // the BUSCA_APPEAR_* codes appear_kernel.hip.inc switches on; declarations only (hidden here)
#include "../../include/busca_ghost.h"      // the BUSCA_GHOST_* codes ghost_kernel.hip.inc switches on; declarations only (hidden here)

#pragma GCC visibility push(default)
#include "../../include/busca_gframe.h"
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

#define CAPI_EHIP BUSCA_GFRAME_EHIP
#include "capi_prelude.hpp"

extern "C" int busca_gframe_version(void) { return 1000; }

extern "C" const char* busca_gframe_last_error(void) { return g_err; }

extern "C" int busca_gframe_advance(double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos, double* vel, int32_t S,
                                    int32_t H, const int32_t* slot, int32_t n, int32_t n_step, int32_t num_active, int32_t last_n_frames, int32_t diff32,
                                    const float* warp, double* pos_out, int32_t device, void* stream) {
    static const char* who = "busca_gframe_advance";
    if (S < 0 || H < 0 || n < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative size (S %d, H %d, n %d)", who, S, H, n);
    if (device < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative device %d", who, device);
    if (H < 2) return refuse(BUSCA_GFRAME_EINVAL, "%s: H = %d, a ring needs at least 2 rows to hold one velocity", who, H);
    if (n_step < 0 || n_step > n) return refuse(BUSCA_GFRAME_EINVAL, "%s: n_step %d outside 0 .. %d", who, n_step, n);
    if (num_active < 0 || num_active > n_step) return refuse(BUSCA_GFRAME_EINVAL, "%s: num_active %d outside 0 .. %d", who, num_active, n_step);
    if (last_n_frames < 2)
        return refuse(BUSCA_GFRAME_EINVAL, "%s: last_n_frames = %d; at least 2 (with 1 the reference takes the mean of no velocity)", who, last_n_frames);
    if (n == 0 || (!warp && n_step == 0)) return 0;
    if (!hist || !frames || !count || !newest || !pos || !vel || !slot)
        return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (hist, frames, count, newest, pos, vel and slot are required)", who);
    if (n_step > 0 && !pos_out) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (pos_out with n_step %d)", who, n_step);
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(pos_out, 8) || misaligned(frames, 4) || misaligned(count, 4) ||
        misaligned(newest, 4) || misaligned(slot, 4) || misaligned(warp, 4))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    GFrameAdvance a;
    a.r = GhostMotionRings{hist, (int*)frames, (int*)count, (int*)newest, pos, vel, S, H};
    a.slot = (const int*)slot, a.warp = warp, a.out = pos_out;
    a.n = warp ? n : n_step, a.n_step = n_step, a.num_active = num_active, a.last_n = last_n_frames, a.diff32 = diff32 != 0;
    CAPI_LAUNCH(who, device, gframe_advance_kernel, dim3((unsigned)a.n), dim3(64), stream, a);
    return 0;
}

extern "C" int busca_gframe_cost(const double* app, const double* pos, const double* det_boxes, int32_t n, int32_t m, double alpha,
                                 const int32_t* track_label, const int32_t* det_label, int32_t num_active, const double* thr, double* out, int32_t device,
                                 void* stream) {
    static const char* who = "busca_gframe_cost";
    if (n < 0 || m < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative size (n %d, m %d)", who, n, m);
    if (device < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative device %d", who, device);
    if (alpha != alpha) return refuse(BUSCA_GFRAME_EINVAL, "%s: alpha is NaN", who);
    if ((track_label == nullptr) != (det_label == nullptr)) return refuse(BUSCA_GFRAME_EINVAL, "%s: track_label and det_label go together", who);
    const long long row_tiles = ((long long)n + PW_TA - 1) / PW_TA, col_tiles = ((long long)m + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_GFRAME_EINVAL, "%s: %d tracks need more workgroups than a grid holds (%d at most)", who, n, 65535 * PW_TA);
    if (n == 0 || m == 0) return 0;
    if (!app || !out) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (app and out are required)", who);
    if (pos && !det_boxes) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (det_boxes with pos)", who);
    if (misaligned(app, 8) || misaligned(pos, 8) || misaligned(det_boxes, 8) || misaligned(thr, 8) || misaligned(out, 8) || misaligned(track_label, 4) ||
        misaligned(det_label, 4))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    GFrameCost a;
    a.app = app, a.pos = pos, a.boxes = det_boxes, a.tlabel = (const int*)track_label, a.dlabel = (const int*)det_label, a.thr = thr, a.out = out;
    a.w_app = 1.0 - alpha, a.w_motion = alpha;                    // as busca_ghost_combine forms them
    const int na = num_active < 0 ? 0 : num_active > n ? n : num_active;      // for a row i < n, i < num_active is i < na
    a.rows = GFrameRows{na, n - na, 0, na, na};                   // row i of the matrix is row i of pos and track_label
    a.m = m, a.ld = m;
    CAPI_LAUNCH(who, device, gframe_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles), dim3(256), stream, a);
    return 0;
}

extern "C" int busca_gframe_keep(double* cost, int32_t n, int32_t m, int32_t lo, int32_t hi, int32_t num_active, const int32_t* row_to_col,
                                 const int32_t* col_to_row, const double* thr, int32_t* track_det, int32_t* det_track, int32_t merge, int32_t mask_from,
                                 int32_t device, void* stream) {
    static const char* who = "busca_gframe_keep";
    if (n < 0 || m < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative size (n %d, m %d)", who, n, m);
    if (device < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative device %d", who, device);
    if (lo < 0 || hi < lo || hi > n) return refuse(BUSCA_GFRAME_EINVAL, "%s: rows %d .. %d outside 0 .. %d", who, lo, hi, n);
    if (num_active < 0 || num_active > n) return refuse(BUSCA_GFRAME_EINVAL, "%s: num_active %d outside 0 .. %d", who, num_active, n);
    if (mask_from >= 0 && (mask_from < hi || mask_from > n))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: mask_from %d outside %d .. %d (the masked rows lie behind the rows that are read)", who, mask_from, hi, n);
    if (m == 0 || (hi == lo && merge != 0)) return 0;
    if (!det_track || !col_to_row) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (col_to_row and det_track are required)", who);
    if (hi > lo && (!cost || !row_to_col || !thr || !track_det))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (cost, row_to_col, thr and track_det are required with rows)", who);
    if (misaligned(cost, 8) || misaligned(thr, 8) || misaligned(row_to_col, 4) || misaligned(col_to_row, 4) || misaligned(track_det, 4) ||
        misaligned(det_track, 4))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    GFrameKeep a;
    a.cost = cost, a.row_to_col = (const int*)row_to_col, a.col_to_row = (const int*)col_to_row, a.thr = thr;
    a.track_det = (int*)track_det, a.det_track = (int*)det_track;
    a.m = m, a.ld = m, a.lo = lo, a.hi = hi, a.num_active = num_active, a.merge = merge != 0, a.mask_from = mask_from, a.mask_to = n;
    const int threads = hi - lo > m ? hi - lo : m;
    CAPI_LAUNCH(who, device, gframe_keep_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), stream, a);
    return 0;
}

extern "C" int busca_gframe_apply(double* hist, int32_t* frames, int32_t* m_count, int32_t* m_newest, double* pos, double* vel, int32_t H, float* gallery,
                                  int32_t* g_count, int32_t* g_newest, uint8_t* mv_seen, int32_t budget, int32_t E, int32_t S, const int32_t* slot,
                                  int32_t n, const int32_t* track_det, const int32_t* det_track, const float* det_feat, const double* det_boxes,
                                  int32_t m, int32_t frame, const uint8_t* may_start, const int32_t* free_slot, int32_t n_free, int32_t* det_slot,
                                  int32_t device, void* stream) {
    static const char* who = "busca_gframe_apply";
    if (S < 0 || n < 0 || m < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative size (S %d, n %d, m %d)", who, S, n, m);
    if (n_free < 0 || H < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative size (n_free %d, H %d)", who, n_free, H);
    if (device < 0) return refuse(BUSCA_GFRAME_EINVAL, "%s: negative device %d", who, device);
    if (m > BUSCA_GFRAME_MAX_DETS) return refuse(BUSCA_GFRAME_EINVAL, "%s: %d detections, one call takes %d", who, m, BUSCA_GFRAME_MAX_DETS);
    if ((long long)n + m > 2147483647LL) return refuse(BUSCA_GFRAME_EINVAL, "%s: %d rows and %d columns need more workgroups than a grid holds", who, n, m);
    if (m == 0) return 0;
    if (H < 2) return refuse(BUSCA_GFRAME_EINVAL, "%s: H = %d, a ring needs at least 2 rows to hold one velocity", who, H);
    if (budget < 1 || E < 1) return refuse(BUSCA_GFRAME_EINVAL, "%s: budget %d and E %d: a slot holds at least 1 row of at least 1 value", who, budget, E);
    if (!hist || !frames || !m_count || !m_newest || !pos || !vel)
        return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (the motion state: hist, frames, m_count, m_newest, pos and vel are required)", who);
    if (!gallery || !g_count || !g_newest || !mv_seen)
        return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (the feature rings: gallery, g_count, g_newest and mv_seen are required)", who);
    if (n > 0 && (!slot || !track_det)) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (slot and track_det are required with n > 0)", who);
    if (!det_track || !det_feat || !det_boxes || !may_start || !det_slot)
        return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (det_track, det_feat, det_boxes, may_start and det_slot are required)", who);
    if (n_free > 0 && !free_slot) return refuse(BUSCA_GFRAME_EINVAL, "%s: null pointer (free_slot with n_free %d)", who, n_free);
    if (misaligned(hist, 8) || misaligned(pos, 8) || misaligned(vel, 8) || misaligned(det_boxes, 8) || misaligned(frames, 4) || misaligned(m_count, 4) ||
        misaligned(m_newest, 4) || misaligned(gallery, 4) || misaligned(g_count, 4) || misaligned(g_newest, 4) || misaligned(slot, 4) ||
        misaligned(track_det, 4) || misaligned(det_track, 4) || misaligned(det_feat, 4) || misaligned(free_slot, 4) || misaligned(det_slot, 4))
        return refuse(BUSCA_GFRAME_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32 and float32)", who);
    GFrameApply f;
    f.r = GhostMotionRings{hist, (int*)frames, (int*)m_count, (int*)m_newest, pos, vel, S, H};
    f.gallery = gallery, f.g_count = (int*)g_count, f.g_newest = (int*)g_newest, f.mv_seen = mv_seen;
    f.slot = (const int*)slot, f.track_det = (const int*)track_det, f.det_track = (const int*)det_track;
    f.det_feat = det_feat, f.det_boxes = det_boxes, f.may_start = may_start, f.free_slot = (const int*)free_slot, f.det_slot = (int*)det_slot;
    f.rows = GFrameRows{n, 0, 0, 0, n};                           // row i of the matrix is slot[i]
    f.m = m, f.budget = budget, f.E = E, f.frame = frame, f.n_free = n_free;
    CAPI_LAUNCH(who, device, gframe_apply_kernel, dim3((unsigned)((long long)n + m)), dim3(64), stream, f, (int)n);
    return 0;
}
