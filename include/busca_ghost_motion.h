/*
 * busca_ghost_motion.h - GHOST's linear motion model as device calls of libbusca_hip.so: what the third adapter keeps per track in Python
 * lists and recomputes with a numpy loop every frame (adapters/GHOST/src/base_tracker.py:600-711: motion_compensation, motion_step, motion,
 * get_motion_dist; src/tracking_utils.py:167-173 warp_pos, :254-370 Track.__init__ / add_detection) - the position history, the velocity
 * step and the camera warp - on state that stays in HBM.  The motion cost itself is busca_pairwise(BUSCA_PAIR_IOU_COST) of the positions
 * busca_ghost_motion_step returns and the detections' boxes: 1 - bbox_overlaps with the "+1" pixel convention, tracks x detections.
 * Same conventions as busca_hip.h (return codes, dev / host pointers, `stream`, one ctx per GPU/process).
 *
 * The caller owns the state, six device arrays over S slots with a ring of H rows each (H >= 2):
 *   hist    f64 [S, H, 4]  the ring of tlbr boxes: Track.last_pos
 *   frames  i32 [S, H]     the frame number of every ring row: Track.past_frames
 *   count   i32 [S]        valid rows, <= H (read clamped to 0 .. H)
 *   newest  i32 [S]        the ring row of the newest sample; chronological order runs backwards from it, modulo H - the convention of
 *                          busca_ghost_proxies.  A value outside 0 .. H-1 is read as count - 1, the ring that has not wrapped
 *   pos     f64 [S, 4]     Track.pos, the current (extrapolated) position
 *   vel     f64 [S, 4]     Track.last_v
 * A ring holds the newest H samples: it reproduces the reference for last_n_frames <= H, or for tracks no longer than H.
 *
 * All three calls are asynchronous on `stream`, allocate nothing and synchronise nothing.  An entry of a slot list that is < 0 or >= S is
 * skipped and touches no memory.  The slots of one call must be distinct: duplicates race on that slot's state (the result is one of the
 * writers' values, unspecified which) but every access stays inside the arrays.  Every sum, product and quotient is the single IEEE
 * float64 (or, where stated, float32) operation numpy performs, never contracted to a multiply-add; the divide is correctly rounded.
 * Negative sizes, H < 2, a NULL required pointer or a misaligned pointer (8 bytes for f64, 4 for i32): BUSCA_EINVAL with a message.
 */
#ifndef BUSCA_GHOST_MOTION_H
#define BUSCA_GHOST_MOTION_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Track.__init__ / Track.add_detection (tracking_utils.py:276-283, :338-339, :354): for every pair i < k with s = slot[i] and
 * j = det_index[i] (NULL: j = i),  pos[s] = boxes[j];  the box and `frame` are pushed onto the ring of s (row (newest + 1) mod H, row 0 for
 * an empty ring; count grows up to H, the oldest row is overwritten from then on).  reset[i] != 0 marks a new track in that slot: count = 0
 * and vel = 0 first (last_v = zeros).
 *   slot   dev i32 [k];  det_index dev i32 [k] or NULL;  reset dev u8 [k] or NULL (no pair starts a track)
 *   boxes  dev f64 [m, 4] tlbr; a pair whose j is outside 0 .. m-1 is skipped like one whose slot is
 * One thread per pair.  k = 0: returns 0 and launches nothing. */
int busca_ghost_motion_append(busca_ctx* ctx, double* hist, int32_t* frames, int32_t* count, int32_t* newest, double* pos, double* vel, int32_t S,
                              int32_t H, const int32_t* slot, const int32_t* det_index, const uint8_t* reset, int32_t k, const double* boxes, int32_t m,
                              int32_t frame, void* stream);

/* motion_compensation's loop over the tracks (base_tracker.py:623-631, warp_pos): every valid ring row of every listed slot (slot NULL:
 * all S slots, n is ignored) is replaced, corner by corner, by  W . (x, y, 1):  x' = (w0 * x + w1 * y) + w2,  y' = (w3 * x + w4 * y) + w5  in
 * float64, rounded ONCE to float32 and stored widened.  The reference rounds the corner to float32 first and runs a float32 torch.mm: this
 * result is within half a float32 ulp of the exact value, the reference's within its own float32 error of it.  After the call every
 * warped row holds float32 values, which is what `diff32` of busca_ghost_motion_step is about.
 *   warp   HOST f32 [6], row-major 2x3, read before the call returns (as busca_ecc_align's); GHOST's own estimate is busca_ecc_prepare +
 *          busca_ecc_align_planes (busca_ecc.h)
 * pos and vel are not touched: the reference does not warp Track.pos either, so an inactive track's extrapolated position stays in the
 * previous frame's coordinates until its next detection.  One thread per (slot, ring row, corner).  No listed slot: returns 0. */
int busca_ghost_motion_warp(busca_ctx* ctx, double* hist, const int32_t* count, const int32_t* newest, int32_t S, int32_t H, const int32_t* slot, int32_t n,
                            const float* warp, void* stream);

/* BaseTracker.motion(approximate=False) with center_only = False (base_tracker.py:648-698) and motion_step (:635-646) for the n tracks
 * slot[0 .. n-1], ACTIVE TRACKS FIRST:
 *   i < num_active, count > 1   w = min(count, last_n_frames) newest rows p[0 .. w-1] (oldest first) with frames f[0 .. w-1]:
 *                               v = ( (p[1] - p[0]) / (double)(f[1] - f[0])  +  (p[2] - p[1]) / (double)(f[2] - f[1])  +  ... ) / (double)(w - 1)
 *                               summed sequentially from the oldest pair to the newest in float64 - the bits of numpy's vs.mean(axis=0) -,
 *                               then vel = v and pos = pos + v.  A frame difference of 0 gives the IEEE inf / NaN numpy gives.
 *   i >= num_active, count > 1  pos = pos + vel
 *   count <= 1                  nothing changes
 *   diff32 != 0                 the difference is taken in float32, (float)p[k+1] - (float)p[k], and widened before the divide: numpy's
 *                               dtype rule when every row of the window is a float32 array, as all rows are after a warp (the divide and
 *                               the mean are float64 either way, the frames being int64).  diff32 = 0: the float64 difference of a window
 *                               that holds at least one float64 row.
 *   out    dev f64 [n, 4]: the resulting pos of every listed track in list order - operand `a` of busca_pairwise.  A skipped entry
 *          (slot outside 0 .. S-1) gets a row of NaN.
 * last_n_frames >= 2 (the reference default 100000000 = the whole ring); 1 leaves no pair and the reference's mean of nothing is NaN for
 * every track, 0 and less slice differently: BUSCA_EINVAL, like num_active outside 0 .. n.  One thread per (track, coordinate); the work is
 * a dependent chain of w loads per thread, latency-bound.  n = 0: returns 0 and launches nothing. */
int busca_ghost_motion_step(busca_ctx* ctx, const double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos, double* vel,
                            int32_t S, int32_t H, const int32_t* slot, int32_t n, int32_t num_active, int32_t last_n_frames, int32_t diff32, double* out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
