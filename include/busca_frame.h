/*
 * busca_frame.h - a whole ByteTrack frame on resident Kalman state, as calls of libbusca_frame.so: a context-free library next to
 * libbusca_track.so, whose store it works on (mean f64 [S, 8], cov f64 [S, 8, 8] over S slots, slot lists dev i32 [n]; an entry < 0 or >= S is
 * skipped and touches no memory).  The three association rounds of BYTETracker.update (adapters/ByteTrack/yolox/tracker/byte_tracker.py:312-425)
 * form a chain that busca_assign_stages (busca_assign_stages.h) solves in one launch; the two calls here stand on either side of it:
 *   busca_frame_cost   the two-plane cost slab of the frame in one pass over the boxes
 *   busca_frame_apply  the solver's match vectors applied to the state: KalmanFilter.update of every matched track, KalmanFilter.initiate of every
 *                      new track into a free slot - without the host between the assignment and the filter
 *
 * Conventions of every call, those of busca_track.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_frame_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 pointer not 4-byte aligned, and
 *     what each call lists;
 *   - the arithmetic is that of the busca_track_* kernels, float64 and never contracted to a multiply-add: the same device code, included.
 */
#ifndef BUSCA_FRAME_H
#define BUSCA_FRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_FRAME_OK 0
#define BUSCA_FRAME_EINVAL (-1)
#define BUSCA_FRAME_EHIP (-2)

#define BUSCA_FRAME_MAX_DETS 2048 /* most detections of one busca_frame_apply call (BUSCA_ASSIGN_MAX: what the solver before it takes) */

/* 1000 * major + minor; this header is version 1000. */
int busca_frame_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_frame_last_error(void);

/* The cost slab of a frame:  out  dev f64 [2, n, m], rows the listed slots, columns the detections.
 *   det_tlbr   dev f64 [m, 4];  det_score  dev f64 [m] or NULL;  det_class  dev u8 [m]: 0 a first-round (high-score) detection, 1 a second-round
 *              (low-score) one, anything else a detection of neither round
 *   plane 0    matching.fuse_score of matching.iou_distance, 1 - IoU * det_score[j], at the columns of class 0 (det_score NULL: plain 1 - IoU,
 *              args.mot20) and +inf elsewhere: the first round and the round of the unconfirmed tracks read it
 *   plane 1    plain 1 - IoU at the columns of class 1 and +inf elsewhere: the second round reads it
 * At the columns of its class each plane holds the bits busca_track_round_cost gives for the same states and detections without a motion flag (with
 * det_score for plane 0, without for plane 1); the IoU of a pair is computed once.  The row of a skipped slot is +inf in both planes.  A column of
 * +inf is to the solver a column that is not there: it admits a pair only below its limit.
 *   status     dev i32 [n] or NULL: all 0 (nothing is factored here); kept so that the words of a frame have one layout
 * Refused: more than 65535 * 16 listed tracks (the grid's second dimension).  n = 0 or m = 0: returns 0 and launches nothing. */
int busca_frame_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_tlbr, const double* det_score,
                     const uint8_t* det_class, int32_t m, double* out, int32_t* status, int32_t device, void* stream);

/* The match vectors of busca_assign_stages, enqueued earlier on the same stream, applied to the state in one launch of n + m workgroups.
 *   row_to_col  dev i32 [n]: row i with 0 <= row_to_col[i] < m gets KalmanFilter.update of slot[i] with det_xyah[row_to_col[i]] - what STrack.update
 *               and STrack.re_activate do to the state; bit-equal to busca_track_kalman_update of the same pairs
 *   status      dev i32 [n] or NULL: 1 where the projected covariance is not positive definite (that slot keeps its state), 0 elsewhere, also
 *               for an unmatched row and a skipped slot
 *   col_to_row  dev i32 [m];  det_xyah  dev f64 [m, 4];  det_score  dev f64 [m] or NULL;  det_class  dev u8 [m]
 *   a column j starts a track when  col_to_row[j] < 0,  det_class[j] == 0  and not  det_score[j] < det_thresh  (byte_tracker.py:420-423; with
 *               det_score NULL every unmatched column of class 0 does).  It is initiated (KalmanFilter.initiate, bit-exact) into free_slot[k], k
 *               its rank among such columns in ascending j: the same slots run after run, no atomics
 *   free_slot   dev i32 [n_free] (NULL with n_free = 0).  The free slots must be distinct and disjoint from slot[]: that is the caller's contract -
 *               otherwise two workgroups race on a state, though every access stays inside the arrays.  An entry outside 0 .. S-1 is skipped
 *               like any other slot
 *   new_slot    dev i32 [m]: the slot taken (as listed, also when it was skipped); -1 for a column that starts no track; -2 for a column that
 *               would but has rank >= n_free - the store is full, nothing is written for it
 * Refused: n_free < 0, a NaN det_thresh, m beyond BUSCA_FRAME_MAX_DETS.  n = 0 and m = 0 together: returns 0 and launches nothing; with n = 0 the
 * row operands may be NULL, with m = 0 the column operands. */
int busca_frame_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const int32_t* row_to_col, const int32_t* col_to_row,
                      const double* det_xyah, const double* det_score, const uint8_t* det_class, int32_t m, double det_thresh,
                      const int32_t* free_slot, int32_t n_free, int32_t* new_slot, int32_t* status, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
