/*
 * busca_sort.h - StrongSORT's track state on the device, as calls of libbusca_sort.so: a context-free library next to libbusca_track.so (no busca_ctx,
 * no weights, no workspace).  The state is the two arrays of busca_track.h, owned by the caller,
 *   mean  f64 [S, 8]      (x, y, a, h, vx, vy, va, vh)
 *   cov   f64 [S, 8, 8]
 * over S slots, and every call names the slots it serves:  slot  dev i32 [n].  An entry < 0 or >= S is skipped and touches no memory.  The slots of
 * one call must be distinct: duplicates race on that slot's state, but every access stays inside the arrays.  The layout being busca_track.h's,
 * busca_track_kalman_initiate and busca_track_kalman_boxes serve a StrongSORT store unchanged (Track.__init__, to_tlwh, to_tlbr are ByteTrack's
 * arithmetic); what differs from ByteTrack's filter is here: adapters/StrongSORT/deep_sort/track.py:202-250 (predict, camera_update, update),
 * linear_assignment.py:164-210 (gate_cost_matrix) with the clamp of min_cost_matching (:61), and the IoU stage of Tracker._match
 * (tracker.py:238-248).  deep_sort/kalman_filter.py and iou_matching.py are not part of the reference tree: their formulas are restated from
 * upstream StrongSORT (DESIGN K-SORT) and are pinned to numpy / Python restatements, not to the reference's output.
 *
 * Conventions of every call (those of busca_track.h):
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_sort_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and the n = 0 / m = 0 no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 pointer not 4-byte aligned, and
 *     what each call lists;
 *   - float64 throughout, never contracted to a multiply-add.
 */
#ifndef BUSCA_SORT_H
#define BUSCA_SORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_SORT_OK 0
#define BUSCA_SORT_EINVAL (-1)
#define BUSCA_SORT_EHIP (-2)

/* flags of busca_sort_gate_cost and busca_sort_iou_cost */
#define BUSCA_SORT_MC 1    /* opt.MC: after the gate, lambda * value + (1 - lambda) * distance for EVERY entry, the gated ones too */
#define BUSCA_SORT_CLAMP 2 /* min_cost_matching: a value > max_distance becomes max_distance + 1e-5 */

/* 1000 * major + minor; this header is version 1000. */
int busca_sort_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_sort_last_error(void);

/* Track.predict (KalmanFilter.predict of upstream StrongSORT) of the listed slots in place:  mean = F mean,  cov = F (P F^T) + diag(std^2)  in
 * numpy's association order of multi_dot((F, P, F.T)); the standard deviations are ByteTrack's, there is no mean[7] = 0 rule.  One 64-lane
 * workgroup per track.  Bit-exact against numpy.  n = 0: returns 0 and launches nothing. */
int busca_sort_predict(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, int32_t device, void* stream);

/* Track.update's Kalman step, the NSA filter: KalmanFilter.update(mean, cov, meas[j], conf[j]) of slot[i] with measurement j = det_index[i]
 * (NULL: j = i; then n <= m), in place.  It is busca_track_kalman_update with the innovation's standard deviations scaled by (1 - conf[j])
 * before they are squared.
 *   meas    dev f64 [m, 4] (x, y, a, h)
 *   conf    dev f64 [m], indexed by the measurement, or NULL: confidence 0, which is busca_track_kalman_update bit for bit.  A NaN conf[j] is
 *           not refused - it is a device value; it makes that slot's state NaN, as numpy does.
 *   status  dev i32 [n] or NULL: 1 where the projected covariance is not positive definite (scipy raises LinAlgError) - that slot keeps its
 *           state -, 0 elsewhere, also for a skipped pair (a slot outside the store, or j outside 0 .. m-1).
 * Same error bounds as busca_kalman_update. */
int busca_sort_update(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n, const double* meas, const int32_t* det_index, int32_t m,
                      const double* conf, int32_t* status, int32_t device, void* stream);

/* linear_assignment.gate_cost_matrix on a device cost matrix and the clamp of min_cost_matching, one launch.  With g the squared Mahalanobis
 * distance (confidence 0) of det_xyah[j] from the projection of slot[i]'s state:
 *   v = g > 9.4877 ? gated_cost : cost[i * ld_cost + j]
 *   BUSCA_SORT_MC      v = lambda * v + (1 - lambda) * g            (1 - lambda is rounded once, on the host)
 *   BUSCA_SORT_CLAMP   v = v > max_distance ? max_distance + 1e-5 : v   (the sum is rounded once, on the host)
 *   out[i * m + j] = v
 * These are busca_kalman_gating and the element-wise gate, blend and clamp of the object route, bit for bit.
 *   det_xyah  dev f64 [m, 4];  cost  dev f64 [n, ld_cost], ld_cost >= m;  out  dev f64 [n, m], which may be `cost` itself when ld_cost = m
 *   status    dev i32 [n] or NULL: 1 where the projected covariance is not positive definite - that row is NaN -, 0 elsewhere
 * The row of a skipped slot has no distance: it is gated_cost, not blended, and clamped like any other value.
 * A 16 x 64 tile per 256-lane workgroup; a track's Cholesky factor is computed once per tile row.
 * Refused: flag bits other than the two, a NaN lambda with MC, a NaN max_distance with CLAMP, ld_cost < m, more than 65535 * 16 listed tracks.
 * n = 0 or m = 0: returns 0 and launches nothing. */
int busca_sort_gate_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n, const double* det_xyah, int32_t m,
                         const double* cost, int32_t ld_cost, double gated_cost, int32_t flags, double lambda, double max_distance, double* out,
                         int32_t* status, int32_t device, void* stream);

/* iou_matching.iou_cost of upstream StrongSORT: out[i, j] = 1 - IoU(to_tlwh of slot[i]'s state, det_tlwh[j]), boxes (x, y, w, h) without a "+1"
 * pixel:  tl = max(a_tl, b_tl), br = min(a_tl + a_wh, b_tl + b_wh), wh = max(0, br - tl), inter = wh[0] * wh[1],
 * cost = 1 - inter / (a_w * a_h + b_w * b_h - inter).  Bit-exact against numpy.
 *   stale     dev u8 [n] or NULL: a row with stale[i] != 0 (time_since_update > 1) is INFTY_COST = 1e5; so is the row of a skipped slot
 *   det_tlwh  dev f64 [m, 4];  out  dev f64 [n, m]
 *   flags     BUSCA_SORT_CLAMP or 0: the clamp of busca_sort_gate_cost at max_distance (max_iou_distance), of every entry
 * Refused: any other flag bit, a NaN max_distance with CLAMP, more than 65535 * 16 listed tracks.  n = 0 or m = 0: launches nothing. */
int busca_sort_iou_cost(const double* mean, int32_t S, const int32_t* slot, int32_t n, const uint8_t* stale, const double* det_tlwh, int32_t m,
                        int32_t flags, double max_distance, double* out, int32_t device, void* stream);

/* Track.camera_update (track.py:220-230) of the listed slots with one 3 x 3 warp: (x1, y1, x2, y2) = to_tlbr of the state,
 *   x1_ = (m00 * x1 + m01 * y1) + m02,  y1_ = (m10 * x1 + m11 * y1) + m12,  the same for (x2, y2),
 *   w = x2_ - x1_,  h = y2_ - y1_,  mean[:4] = (x1_ + w / 2, y1_ + h / 2, w / h, h).
 * Bit-exact against this left-to-right evaluation in float64 (numpy's matrix @ v may round differently: DESIGN K-SORT has the bound).
 *   matrix  f64 [9], row-major, in device memory or in pinned host memory the device can read; it is read when the kernel runs.
 * One lane per track.  get_matrix's distance rule and the lookup in opt.ecc stay with the caller. */
int busca_sort_camera_update(double* mean, int32_t S, const int32_t* slot, int32_t n, const double* matrix, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
