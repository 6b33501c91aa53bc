/*
 * busca_gframe.h - a whole GHOST frame on resident track state, as calls of libbusca_gframe.so: a context-free library next to libbusca_store.so and
 * the GHOST motion unit of libbusca_hip.so, whose state it works on.  Over S track slots (slot lists dev i32 [n]; an entry < 0 or >= S is skipped and
 * touches no memory):
 *   the motion state of busca_ghost_motion.h   hist f64 [S, H, 4], frames i32 [S, H], count i32 [S], newest i32 [S], pos f64 [S, 4], vel f64 [S, 4]
 *   the feature rings of busca_store.h         gallery f32 [S, budget, E], count i32 [S], newest i32 [S], mv_seen u8 [S]
 * Tracker._track of adapters/GHOST/src/tracker.py:203-261 without the BUSCA round - motion_compensation's loop and BaseTracker.motion
 * (base_tracker.py:600-698), get_motion_dist and combine_motion_appearance with the class mask and nan_first (tracker.py:272-275, 388-396),
 * assign_act_inact_same_time / assign_separatly (tracker.py:597-682), Track.add_detection and Track.__init__ (tracking_utils.py:254-370) - forms a
 * chain around busca_ghost_distance / busca_ghost_proxies and busca_linear_assignment; the four calls here are its other links:
 *   busca_gframe_advance  with a warp, the warp of every stored box of the listed tracks, and then the motion step of the first of them, in one launch
 *   busca_gframe_cost     the final cost matrix from the appearance matrix, the stepped positions and the detections' boxes in one pass
 *   busca_gframe_keep     the strict threshold filter on the solver's matches, on the device
 *   busca_gframe_apply    the kept matches and the new tracks applied to both rings - without the host between the assignment and the state
 *
 * Conventions of every call, those of busca_sframe.h and busca_store.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_gframe_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises; one kernel launch per call;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 / float32 pointer not 4-byte
 *     aligned, and what each call lists;
 *   - the arithmetic is that of busca_ghost_motion_warp / _step / _append, busca_pairwise(BUSCA_PAIR_IOU_COST), busca_ghost_combine and
 *     busca_store_ring_add - float64 (float32 where those say so), never contracted to a multiply-add: the same device functions, included.
 */
#ifndef BUSCA_GFRAME_H
#define BUSCA_GFRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_GFRAME_OK 0
#define BUSCA_GFRAME_EINVAL (-1)
#define BUSCA_GFRAME_EHIP (-2)

#define BUSCA_GFRAME_MAX_DETS 2048 /* most detections of one busca_gframe_apply call (BUSCA_ASSIGN_MAX: what the solver before it takes) */

/* 1000 * major + minor; this header is version 1000. */
int busca_gframe_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_gframe_last_error(void);

/* motion_compensation's loop and BaseTracker.motion() in one launch of one 64-lane workgroup per listed slot.
 *   warp    DEVICE f32 [6], row-major 2x3, or NULL.  With it every valid ring row of every listed slot slot[0 .. n-1] is warped first, as
 *           busca_ghost_motion_warp does it (a device pointer, so that an estimate made on the device never has to visit the host)
 *   then, for the first n_step listed slots, busca_ghost_motion_step: the velocity from the window and pos += v for rows < num_active,
 *           pos += vel for the others; the slots from n_step on are warped only.  The step of a slot reads the rows its own workgroup has just
 *           warped, behind a workgroup barrier
 *   pos_out dev f64 [n_step, 4]: the positions after the step, in list order; a skipped slot gets a row of NaN
 * Bit-equal to busca_ghost_motion_warp on the listed slots followed by busca_ghost_motion_step (same last_n_frames, diff32) on the first n_step.
 * The listed slots must be distinct.  Refused: H < 2, n_step outside 0 .. n, num_active outside 0 .. n_step, last_n_frames < 2.
 * n = 0, or warp NULL with n_step = 0: returns 0 and launches nothing. */
int busca_gframe_advance(double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos, double* vel, int32_t S, int32_t H,
                         const int32_t* slot, int32_t n, int32_t n_step, int32_t num_active, int32_t last_n_frames, int32_t diff32, const float* warp,
                         double* pos_out, int32_t device, void* stream);

/* The final cost matrix  out  dev f64 [n, m], tracks x detections, in one pass; every entry in the reference's order:
 *   1. c = app[i, j], NaN where track_label[i] != det_label[j]                       (dev i32 [n] and [m], or both NULL: no mask)
 *   2. with pos (dev f64 [n, 4], busca_gframe_advance's pos_out; NULL: no blend):  c = (1 - alpha) * c + alpha * (1 - IoU(pos[i], det_boxes[j])),
 *      the IoU with the "+1" pixel convention, det_boxes dev f64 [m, 4] tlbr
 *   3. with thr (dev f64 [2], or NULL): NaN where not c <= thr[i < num_active ? 0 : 1]                                   (nan_first)
 * `out` may be `app`.  Bit-equal to busca_pairwise(BUSCA_PAIR_IOU_COST) of pos and det_boxes followed by busca_ghost_combine, without the [n, m]
 * motion matrix ever existing; with pos NULL it is busca_ghost_combine without motion.  A 16 x 64 tile per 256-lane workgroup, the boxes staged
 * once in LDS.  Refused: a NaN alpha, one label vector without the other, det_boxes NULL with pos, more than 65535 * 16 tracks (the grid's second
 * dimension).  n = 0 or m = 0: returns 0 and launches nothing. */
int busca_gframe_cost(const double* app, const double* pos, const double* det_boxes, int32_t n, int32_t m, double alpha, const int32_t* track_label,
                      const int32_t* det_label, int32_t num_active, const double* thr, double* out, int32_t device, void* stream);

/* The filter of assign_act_inact_same_time (tracker.py:611-633) on the match vectors busca_linear_assignment wrote for the rows lo .. hi - 1 of
 * cost dev f64 [n, m] (row_to_col dev i32 [hi - lo], col_to_row dev i32 [m], a row index relative to lo).  The matched pair (i, j),
 * j = row_to_col[i - lo] >= 0 and col_to_row[j] == i - lo, is kept when  cost[i, j] < thr[i < num_active ? 0 : 1]  - strictly, thr dev f64 [2]; a NaN
 * cost or threshold keeps nothing.
 *   track_det  dev i32 [n]: track_det[i] = j for a kept pair, -1 for every other row of the range; rows outside the range are not written
 *   det_track  dev i32 [m]: det_track[j] = i for a kept pair.  merge == 0: -1 for every other column.  merge != 0: the other columns are not
 *              written - a later stage that adds its pairs to an earlier stage's vector
 *   mask_from  >= 0: NaN is written into cost[i', j] for every mask_from <= i' < n at each KEPT column j: assign_separatly's "only use detections
 *              that have not been assigned yet" (tracker.py:660-667) - it withdraws the columns that were assigned, not those merely matched.
 *              < 0: cost is not written
 * One thread per row of the range and per column; no atomics: a column is matched by at most one row.
 * Refused: lo, hi outside 0 <= lo <= hi <= n, num_active outside 0 .. n, a mask_from in 0 .. hi - 1 (the rows this call reads) or beyond n.
 * m = 0 or hi == lo with merge != 0: returns 0 and launches nothing. */
int busca_gframe_keep(double* cost, int32_t n, int32_t m, int32_t lo, int32_t hi, int32_t num_active, const int32_t* row_to_col, const int32_t* col_to_row,
                      const double* thr, int32_t* track_det, int32_t* det_track, int32_t merge, int32_t mask_from, int32_t device, void* stream);

/* The vectors of busca_gframe_keep, enqueued earlier on the same stream, applied to both states in one launch of n + m 64-lane workgroups.
 *   workgroup i < n     with 0 <= j = track_det[i] < m: Track.add_detection of slot[i] - det_feat[j] (dev f32 [m, E]) becomes the newest sample of its
 *                       feature ring (the bits and bookkeeping of busca_store_ring_add) and det_boxes[j] (dev f64 [m, 4]) with `frame` its position
 *                       and the newest row of its position ring (those of busca_ghost_motion_append: pos, ring row, count, newest)
 *   workgroup n + j     with det_track[j] < 0 and may_start[j] != 0 (dev u8 [m]): Track.__init__ into free_slot[k], k its rank among such columns in
 *                       ascending j - counted by the workgroup itself, the same slots run after run.  The slot's feature ring is emptied and
 *                       mv_seen = 0, its history emptied and its velocity zero, then the first sample and box: the is_new / reset paths of
 *                       those two calls
 *   det_slot  dev i32 [m]: the slot written - the track's own (as listed, also when it was skipped), the new one (likewise), -1 when nothing
 *                       happened, -2 for a column that would start a track but has rank >= n_free: the store is full, nothing is written for it
 *   free_slot dev i32 [n_free] (NULL with n_free = 0).  The free slots must be distinct and disjoint from slot[], and the listed slots distinct:
 *                       that is the caller's contract - otherwise two workgroups race on a slot, though every access stays inside the arrays
 *   g_count, g_newest   the feature rings' count and newest; m_count, m_newest the position rings'
 * Refused: n_free < 0, H < 2, budget or E below 1, m beyond BUSCA_GFRAME_MAX_DETS, n + m beyond what a grid holds.  m = 0: returns 0 and
 * launches nothing (without detections nothing is assigned); with n = 0 the row operands may be NULL. */
int busca_gframe_apply(double* hist, int32_t* frames, int32_t* m_count, int32_t* m_newest, double* pos, double* vel, int32_t H, float* gallery,
                       int32_t* g_count, int32_t* g_newest, uint8_t* mv_seen, int32_t budget, int32_t E, int32_t S, const int32_t* slot, int32_t n,
                       const int32_t* track_det, const int32_t* det_track, const float* det_feat, const double* det_boxes, int32_t m, int32_t frame,
                       const uint8_t* may_start, const int32_t* free_slot, int32_t n_free, int32_t* det_slot, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
