/*
 * busca_track.h - tracker state that lives on the device, as calls of libbusca_track.so: a second library next to libbusca_hip.so that needs no
 * busca_ctx (no weights, no workspace, no per-context state).  First tenant: ByteTrack's Kalman state (adapters/ByteTrack/yolox/tracker/
 * kalman_filter.py, byte_tracker.py:50-61,67,78,109,142-163, matching.py:132-186), which the busca_kalman_* calls of busca_hip.h take as contiguous
 * arrays in list order and which therefore crossed PCIe on every call.  Here the state stays in two device arrays the caller owns,
 *   mean  f64 [S, 8]      (x, y, a, h, vx, vy, va, vh)
 *   cov   f64 [S, 8, 8]
 * over S slots, and every call names the slots it serves:  slot  dev i32 [n].  An entry < 0 or >= S is skipped and touches no memory.  The slots of
 * one call must be distinct: duplicates race on that slot's state, but every access stays inside the arrays.
 *
 * Conventions of every call:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_track_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and the n = 0 no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 pointer not 4-byte aligned, and
 *     what each call lists;
 *   - the arithmetic is that of the busca_kalman_* kernels, float64 and never contracted to a multiply-add: the same device code, included.
 */
#ifndef BUSCA_TRACK_H
#define BUSCA_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_TRACK_OK 0
#define BUSCA_TRACK_EINVAL (-1)
#define BUSCA_TRACK_EHIP (-2)

/* flags of busca_track_round_cost */
#define BUSCA_TRACK_FUSE_MOTION 1   /* matching.fuse_motion: the gate, then lambda * cost + (1 - lambda) * distance */
#define BUSCA_TRACK_ONLY_POSITION 2 /* gate on (x, y) alone: chi2inv95[2] = 5.9915 instead of chi2inv95[4] = 9.4877 */
#define BUSCA_TRACK_GATE_ONLY 4     /* matching.gate_cost_matrix: the gate without the blend; excludes FUSE_MOTION */

/* 1000 * major + minor; this header is version 1000. */
int busca_track_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_track_last_error(void);

/* KalmanFilter.initiate (kalman_filter.py:54-85): for i < n the state of slot[i] becomes that of measurement j = det_index[i] (NULL: j = i).
 *   meas  dev f64 [m, 4] (x, y, a, h);  det_index  dev i32 [n] or NULL (then n <= m).  A pair whose j is outside 0 .. m-1 is skipped like one whose
 * slot is.  Bit-exact against numpy.  n = 0: returns 0 and launches nothing. */
int busca_track_kalman_initiate(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index,
                                int32_t m, int32_t device, void* stream);

/* STrack.multi_predict (byte_tracker.py:50-61) of the listed slots in place: mean[7] = 0 first where not_tracked[i] != 0, then the
 * constant-velocity prediction.   not_tracked  dev u8 [n] or NULL (every listed track is Tracked).  Bit-exact against numpy. */
int busca_track_kalman_predict(double* mean, double* cov, int32_t S, const int32_t* slot, const uint8_t* not_tracked, int32_t n, int32_t device,
                               void* stream);

/* KalmanFilter.update (kalman_filter.py:193-225) of slot[i] with measurement det_index[i] (NULL: i; then n <= m), in place.
 *   status  dev i32 [n] or NULL: 1 where the projected covariance is not positive definite (scipy raises LinAlgError) - that slot keeps its state -,
 *           0 elsewhere, also for a skipped pair.  Same error bounds as busca_kalman_update. */
int busca_track_kalman_update(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index,
                              int32_t m, int32_t* status, int32_t device, void* stream);

/* STrack.tlwh (tlbr = 0) or STrack.tlbr (tlbr = 1; any other value is refused) of the listed slots.
 *   out  dev f64 [n, 4], in list order; a skipped entry gets a row of NaN. */
int busca_track_kalman_boxes(const double* mean, int32_t S, const int32_t* slot, int32_t n, int32_t tlbr, double* out, int32_t device, void* stream);

/* The cost matrix of one association round in one launch:  out[i, j] = 1 - IoU(tlbr of slot[i]'s state, det_tlbr[j])  with the "+1" pixel
 * convention (matching.iou_distance); with det_score, matching.fuse_score:  1 - IoU * det_score[j].  Then, by `flags`:
 *   BUSCA_TRACK_GATE_ONLY     inf where the squared Mahalanobis distance of det_xyah[j] from the state's projection exceeds the chi-square gate
 *   BUSCA_TRACK_FUSE_MOTION   the same gate, then  lambda * cost + (1 - lambda) * distance
 *   BUSCA_TRACK_ONLY_POSITION with either: distance and gate of (x, y) alone
 * These are busca_kalman_boxes, busca_pairwise(BUSCA_PAIR_IOU_COST), busca_kalman_gating and the element-wise gate and blend, bit for bit.
 *   det_tlbr  dev f64 [m, 4];  det_xyah  dev f64 [m, 4], required with a motion flag, else ignored;  det_score  dev f64 [m] or NULL
 *   out       dev f64 [n, m]; the row of a skipped entry is +inf
 *   status    dev i32 [n] or NULL: 1 where the projected covariance is not positive definite (with FUSE_MOTION that row is NaN, with GATE_ONLY
 *             it is left ungated: a NaN distance passes no comparison), 0 elsewhere - all 0 without a motion flag
 * Refused: det_xyah NULL with a motion flag, flag bits other than the three, FUSE_MOTION together with GATE_ONLY, a NaN lambda, more than
 * 65535 * 16 listed tracks (the grid's second dimension).  n = 0 or m = 0: returns 0 and launches nothing. */
int busca_track_round_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_tlbr,
                           const double* det_xyah, const double* det_score, int32_t m, int32_t flags, double lambda, double* out, int32_t* status,
                           int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
