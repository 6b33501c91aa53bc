/*
 * busca_sframe.h - a whole StrongSORT frame on resident track state, as calls of libbusca_sframe.so: a context-free library next to
 * libbusca_sort.so, whose store it works on (mean f64 [S, 8], cov f64 [S, 8, 8] over S slots, slot lists dev i32 [n]; an entry < 0 or >= S is
 * skipped and touches no memory), and beside it one float32 feature row per slot (feat f32 [S + 1, E]: the track's features[-1] of
 * adapters/StrongSORT/deep_sort/track.py:85-87, 244-248).  Tracker.predict, Tracker.camera_update, Tracker._match and Tracker.update
 * (deep_sort/tracker.py:74-126, 197-252) form a chain around busca_assign_stages (busca_assign_stages.h); the three calls here are its other links:
 *   busca_sframe_advance  with a warp, Track.camera_update, and then Track.predict of every listed track in one launch
 *   busca_sframe_cost     both planes of the [2, n, m] cost slab of Tracker._match in one launch: the gated appearance cost of the cascade in plane
 *                         0, the IoU cost in plane 1, each only at the rows whose stage reads it
 *   busca_sframe_apply    the solver's match vectors applied to the state: the EMA feature and the NSA Kalman update of every matched track,
 *                         KalmanFilter.initiate and the first feature of every new track - without the host between the assignment and the filter
 *
 * Conventions of every call, those of busca_sort.h and busca_frame.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_sframe_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 / float32 pointer not 4-byte
 *     aligned, and what each call lists;
 *   - the arithmetic is that of the busca_sort_*, busca_track_* and busca_store_ema_fit kernels - float64 for the filter, float32 for the features,
 *     never contracted to a multiply-add: the same device code, included.
 */
#ifndef BUSCA_SFRAME_H
#define BUSCA_SFRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_SFRAME_OK 0
#define BUSCA_SFRAME_EINVAL (-1)
#define BUSCA_SFRAME_EHIP (-2)

/* `flags` of busca_sframe_cost: the values of BUSCA_SORT_MC and BUSCA_SORT_CLAMP (busca_sort.h), for plane 0 */
#define BUSCA_SFRAME_MC 1
#define BUSCA_SFRAME_CLAMP 2

#define BUSCA_SFRAME_MAX_DETS 2048 /* most detections of one busca_sframe_apply call (BUSCA_ASSIGN_MAX: what the solver before it takes) */

/* 1000 * major + minor; this header is version 1001 (1001: busca_sframe_advance warps the stored
 * mean before it predicts, as the reference's loop does; 1000 predicted first). */
int busca_sframe_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_sframe_last_error(void);

/* When `matrix` (dev f64 [3, 3], row-major; NULL: none) is given, Track.camera_update of the stored mean of every listed slot with it - a coordinate
 * is warped as (m00 * x + m01 * y) + m02, left to right - and then Track.predict of the slot in place, which reads the warped height: the order of
 * the reference's loop (deep_sort_app.py:186-189).  One 64-lane workgroup per listed slot.  Bit-equal to busca_sort_camera_update followed by
 * busca_sort_predict.  n = 0: returns 0 and launches nothing. */
int busca_sframe_advance(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* matrix, int32_t device, void* stream);

/* The cost slab of Tracker._match:  out  dev f64 [2, n, m], rows the listed slots, columns the detections; it must not be `cost`.
 *   first, again  dev i32 [n] (again may be NULL: never), depth: the row tables busca_assign_stages is given - stages 0 .. depth - 1 are the levels
 *                 of the matching cascade (or, depth 1, the one appearance stage of opt.woC) and read plane 0, stage `depth` is the IoU stage and
 *                 reads plane 1
 *   plane 0       row i needs it when 0 <= first[i] < depth.  Its entries are then what busca_sort_gate_cost writes for the same states, det_xyah
 *                 dev f64 [m, 4], appearance matrix `cost` dev f64 [n, ld_cost], gated_cost, flags (MC with mc_lambda, CLAMP with max_distance)
 *   plane 1       row i needs it when first[i] == depth or again[i] == depth.  Its entries are then what busca_sort_iou_cost writes for det_tlwh
 *                 dev f64 [m, 4] and `stale` dev u8 [n] (NULL: none) with BUSCA_SORT_CLAMP at max_iou_distance
 *   elsewhere     +inf, and neither the Cholesky factor nor the IoU of that row is computed.  No stage reads such an entry, and the solver admits a
 *                 pair only below its stage's limit: +inf is a row that is not there
 *   status        dev i32 [n] or NULL: 1 where a row that needs plane 0 has a projected covariance that is not positive definite (that row of plane
 *                 0 is NaN), 0 elsewhere - also for a row that is not gated, whatever its covariance
 * Refused: depth < 0, ld_cost < m, unknown flag bits, NaN mc_lambda with MC, NaN max_distance with CLAMP, NaN max_iou_distance, out == cost, more
 * than 65535 * 16 listed tracks (the grid's second dimension).  n = 0 or m = 0: returns 0 and launches nothing. */
int busca_sframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_xyah, const double* det_tlwh,
                      int32_t m, const uint8_t* stale, const double* cost, int32_t ld_cost, double gated_cost, int32_t flags, double mc_lambda,
                      double max_distance, double max_iou_distance, const int32_t* first, const int32_t* again, int32_t depth, double* out,
                      int32_t* status, int32_t device, void* stream);

/* The match vectors of busca_assign_stages, enqueued earlier on the same stream, applied to the state in one launch of n + m 64-lane workgroups.
 *   row_to_col  dev i32 [n]: row i with 0 <= j = row_to_col[i] < m is Track.update (track.py:232-250) of slot[i] with detection j -
 *               first the feature row: f = det_feat[j] / ||det_feat[j]||, smooth = alpha * feat[slot[i]] + (1 - alpha) * f, the row becomes
 *               smooth / ||smooth|| (float32, the weights (float)alpha and (float)(1.0 - alpha), every product, sum, quotient and root rounded once:
 *               bit-equal to busca_store_ema_fit of that row with group_old_row 0 on feat seen as a [S + 1, 1, E] gallery);
 *               then KalmanFilter.update(mean, covariance, det_xyah[j], det_conf[j]), bit-equal to busca_sort_update of the same pair
 *   status      dev i32 [n] or NULL: 1 where the projected covariance is not positive definite (that slot keeps its Kalman state), 0 elsewhere,
 *               also for an unmatched row and a skipped slot.  The feature row of such a track is written all the same: the reference raises
 *               LinAlgError inside kf.update, after the feature was smoothed, and the frame is lost either way
 *   col_to_row  dev i32 [m];  det_xyah  dev f64 [m, 4];  det_conf  dev f64 [m] or NULL (confidence 0);  det_feat  dev f32 [m, E]
 *   a column j with col_to_row[j] < 0 starts a track (tracker.py:197-198): KalmanFilter.initiate (bit-exact) into free_slot[k], k its rank
 *               among such columns in ascending j - the same slots run after run, no atomics -, and feat[that slot] = det_feat[j] / ||det_feat[j]||
 *   free_slot   dev i32 [n_free] (NULL with n_free = 0).  The free slots must be distinct and disjoint from slot[]: that is the caller's contract -
 *               otherwise two workgroups race on a state, though every access stays inside the arrays.  An entry outside 0 .. S-1 is skipped
 *               like any other slot
 *   new_slot    dev i32 [m]: the slot taken (as listed, also when it was skipped); -1 for a matched column; -2 for a column that would start a track
 *               but has rank >= n_free - the store is full, nothing is written for it
 *   feat        dev f32 [S + 1, E], row s the feature of slot s
 * Refused: n_free < 0, E < 1, a NaN alpha, m beyond BUSCA_SFRAME_MAX_DETS, n + m beyond what a grid holds.  n = 0 and m = 0 together: returns 0 and
 * launches nothing; with n = 0 the row operands may be NULL. */
int busca_sframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const int32_t* row_to_col, const int32_t* col_to_row,
                       const double* det_xyah, const double* det_conf, const float* det_feat, int32_t m, float* feat, int32_t E, double alpha,
                       const int32_t* free_slot, int32_t n_free, int32_t* new_slot, int32_t* status, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
