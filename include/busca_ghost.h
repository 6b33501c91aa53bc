/*
 * busca_ghost.h - the GHOST association entry points of libbusca_hip.so: what the third adapter's association round
 * (adapters/GHOST/src/tracker.py:263-412, base_tracker.py:495-531 and :713-731, tracking_utils.py:63-126) computes between the ReID
 * features in HBM and busca_linear_assignment - proxy distances with all five reductions, one proxy vector per track, data-driven
 * thresholds, and the class mask / motion blend / threshold pass - as device calls.  Same conventions as busca_hip.h (return codes,
 * dev / host pointers, `stream`, one ctx per GPU/process); the context and the error codes are the ones declared there.
 *
 * Every matrix is tracks x detections, float64, row-major, like the rest of the library; GHOST's own [detections, tracks] orientation is
 * the transposed view.  Only the cosine distance exists: the reference's other two branches do not work there (`distance != 'cosine'`
 * takes F.pairwise_distance's norm over the gallery axis of the broadcast tensor and returns [m, E], base_tracker.py:101; `use_bism` calls
 * .numpy() on what is already a numpy array, :105-106).
 */
#ifndef BUSCA_GHOST_H
#define BUSCA_GHOST_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `reduce` of busca_ghost_distance: tracker_cfg['avg_inact']['num'] - 1 (tracker.py:287-296) */
#define BUSCA_GHOST_MIN 0
#define BUSCA_GHOST_MEAN 1
#define BUSCA_GHOST_MAX 2
#define BUSCA_GHOST_MIDRANGE 3 /* (max + min) / 2 */
#define BUSCA_GHOST_MEDIAN 4   /* np.median */
#define BUSCA_GHOST_MEDIAN_BUDGET_MAX 256 /* MEDIAN stages [budget][64] float64 distances in LDS: 256 x 64 x 8 B = 128 KiB of the 160 KiB */

/* `mode` of busca_ghost_proxies: tracker_cfg['avg_*']['proxy'] (tracking_utils.py:76-113) */
#define BUSCA_GHOST_PROXY_LAST 0
#define BUSCA_GHOST_PROXY_FIRST 1
#define BUSCA_GHOST_PROXY_MEAN 2
#define BUSCA_GHOST_PROXY_MEANNORM 3
#define BUSCA_GHOST_PROXY_MEDIAN 4

/* proxy_dist (tracker.py:278-296): out[i, j] = reduce over the valid rows g of slot(i) of  1 - <g, d_j> / sqrt(<g, g> * <d_j, d_j>).
 * gallery / slot / count / n / budget / dets / m / E / out and every rule about them are busca_appearance_cost's (busca_appearance.h),
 * without flags: a track with no valid row gives a row of +inf, a zero-norm vector NaN, a NaN among a track's distances a NaN cost, rows
 * beyond the count are never read, E is a multiple of 16 in 16 .. 2048, gallery and dets 16-byte aligned.
 * One workgroup per (track, 64-detection tile), four waves, always - budget = 1 included.  Every pair's distance is computed by the code
 * of busca_appearance_cost and has its bits; MIN / MEAN / MAX fold them in its order and equal its output bit for bit.
 *   MIDRANGE  (max + min) / 2 of those two values
 *   MEDIAN    np.median over the valid rows: the middle element of an odd count, (lo + hi) / 2 of the two middle ones of an even count.
 *             The distances are staged in LDS and selected by rank under the strict order (value, row index): duplicates resolve by
 *             their row, no atomics, the same bits every run.  The selection is quadratic in the count (count^2 / 4 comparisons per
 *             lane).  budget > BUSCA_GHOST_MEDIAN_BUDGET_MAX with MEDIAN: BUSCA_EINVAL; the other reductions have no limit.
 * A track's row of `out` depends on that track's samples and the detections only.  n = 0 or m = 0: returns 0 and launches nothing.
 * Negative sizes, budget < 1, a bad E, an unknown reduce, a NULL gallery / dets / out, a misaligned pointer, more workgroups than a grid
 * holds: BUSCA_EINVAL with a message.  Asynchronous on `stream`, allocates nothing, synchronises nothing. */
int busca_ghost_distance(busca_ctx* ctx, const float* gallery, const int32_t* slot, const int32_t* count, int32_t n, int32_t budget,
                         const float* dets, int32_t m, int32_t E, int32_t reduce, double* out, void* stream);

/* get_proxy (tracking_utils.py:63-126): one vector per track from its stored samples.
 *   gallery  dev f32 [S, budget, E], slot dev i32 [n] or NULL, count dev i32 [S] or NULL: as above
 *   newest   dev i32 [S] or NULL: the ring row that holds a slot's newest sample; chronological order runs backwards from it, modulo
 *            `budget`.  NULL (or a value outside 0 .. budget-1): count - 1, the ring that has not wrapped.  A ring that is not full has
 *            not wrapped, so the walk stays inside the valid rows.
 *   window   the newest `window` valid rows take part; window <= 0 or window > count: all valid rows (the reference's `avg == 'all' or
 *            len(past_feats) < avg` branch)
 *   out      dev f32 [n, E]
 *   LAST      the newest row                      FIRST  the oldest valid row (whatever the window)
 *   MEAN      float64 sum from the oldest to the newest row of the window, divided by their number, rounded once to float32
 *   MEANNORM  that float32 mean divided by max(its L2 norm, 1e-12) (F.normalize(.., p=2, dim=0), :100; the `dim=1` spelling at :112 raises on
 *             a vector).  The norm is float64: each of 256 threads adds the squares of its features e = t, t + 256, .. ascending, a wave's 64
 *             sums are added by xor-shuffles (32, 16, .., 1), the four waves as (w0 + w1) + (w2 + w3).
 *   MEDIAN    per feature the LOWER median of the window (rank (w - 1) / 2), as torch.median returns; a NaN among the values gives NaN
 * `mode` (torch.mode) and `mv_avg` (a stateful moving average: a tensor op of the caller's) are not here.  A track without samples
 * (negative slot, count 0) gets a row of NaN.  E >= 1, no alignment rule.  n = 0: returns 0 and launches nothing.  Negative sizes,
 * budget < 1, E < 1, an unknown mode, a NULL gallery / out: BUSCA_EINVAL. */
int busca_ghost_proxies(busca_ctx* ctx, const float* gallery, const int32_t* slot, const int32_t* count, const int32_t* newest, int32_t n,
                        int32_t budget, int32_t E, int32_t mode, int32_t window, float* out, void* stream);

/* update_thresholds (base_tracker.py:495-531): thr_out[0] = mean - k_act * std over rows 0 .. num_active-1 of `cost` (the active tracks),
 * thr_out[1] = mean - k_inact * std over rows num_active .. n-1; std is the population one (np.std); a NaN entry makes its threshold NaN as
 * numpy does.  A group without rows leaves its entry of thr_out as it was (the reference does not update it either).
 *   cost     dev f64 [n, m]; thr_out dev f64 [2]
 * One workgroup of 256 threads, two passes per group (the mean, then the squared deviations from it).  Each sum: thread t adds the group's
 * entries k = t, t + 256, .. (row-major) in ascending order, a wave's 64 sums are added by xor-shuffles (32, 16, .., 1), the four waves as
 * (w0 + w1) + (w2 + w3) - the same bits every run.  n = 0 or m = 0: returns 0 and launches nothing.  Negative sizes, num_active outside
 * 0 .. n, NULL or misaligned (8 bytes) pointers: BUSCA_EINVAL. */
int busca_ghost_thresholds(busca_ctx* ctx, const double* cost, int32_t n, int32_t m, int32_t num_active, double k_act, double k_inact,
                           double* thr_out, void* stream);

/* The rest of the cost matrix, entry by entry, in the reference's order (tracker.py:263-304, 364-396):
 *   1. track_label[i] != det_label[j] -> NaN                                         (nan_over_classes; both label vectors or neither)
 *   2. motion given: (1 - alpha) * app + alpha * motion, two products and a sum      (combine_motion_appearance, combi 'sum_<alpha>')
 *   3. thr given: an entry that is not <= thr[0] (rows < num_active) / thr[1] (the other rows) -> NaN     (nan_first; np.where(dist <= thr, dist, nan))
 *   app, motion, out  dev f64 [n, m] (out may be app); track_label dev i32 [n], det_label dev i32 [m]; thr dev f64 [2]: a device pointer, so
 *   thresholds from busca_ghost_thresholds flow without a synchronisation.
 * It does nothing else: a caller with data-driven thresholds masks first (motion = thr = NULL), runs busca_ghost_thresholds on the masked
 * appearance matrix - what solve_hungarian does - and then blends and thresholds.  n = 0 or m = 0: returns 0 and launches nothing.
 * Negative sizes, a NaN alpha, one label vector without the other, NULL app / out, a misaligned pointer: BUSCA_EINVAL. */
int busca_ghost_combine(busca_ctx* ctx, const double* app, const double* motion, int32_t n, int32_t m, double alpha, const int32_t* track_label,
                        const int32_t* det_label, int32_t num_active, const double* thr, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
