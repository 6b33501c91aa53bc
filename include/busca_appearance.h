/*
 * busca_appearance.h - the appearance-cost entry point of libbusca_hip.so: the cosine distance between the stored ReID samples of
 * every track (its gallery) and the features of every detection, reduced per track, as a float64 cost matrix on the device - the
 * step between busca_reid_forward* (which writes [n,512] f32 features into HBM) and busca_kalman_gating / busca_linear_assignment.
 * Same conventions as busca_hip.h (return codes, dev / host pointers, `stream`, one ctx per GPU/process); the context and the error
 * codes are the ones declared there.
 */
#ifndef BUSCA_APPEARANCE_H
#define BUSCA_APPEARANCE_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `reduce`: how the distances of one track's samples to a detection become one cost */
#define BUSCA_APPEAR_MIN 0  /* nearest neighbour: DeepSORT's metric.distance (adapters/StrongSORT/deep_sort/tracker.py:216-236); GHOST num == 1 */
#define BUSCA_APPEAR_MEAN 1 /* GHOST num == 2 */
#define BUSCA_APPEAR_MAX 2  /* GHOST num == 3 */
/* `flags` */
#define BUSCA_APPEAR_CLAMP0 1 /* max(0, .) of every pair's distance, before the reduction (adapters/ByteTrack/yolox/tracker/matching.py:128) */

#define BUSCA_APPEAR_E_MIN 16
#define BUSCA_APPEAR_E_MAX 2048

/* out[i, j] = reduce over the valid rows g of slot(i) of  1 - <g, d_j> / sqrt(<g, g> * <d_j, d_j>).
 *   gallery  dev f32 [S, budget, E]: the stored samples of S track slots, a ring of `budget` rows each
 *   slot     dev i32 [n] or NULL: the slot of cost-matrix row i (NULL: row i is slot i); slot[i] < 0 marks a track without samples.
 *            The caller keeps slot[i] < S: S is not an argument
 *   count    dev i32 [S] or NULL: rows 0 .. count-1 of a slot are valid (clipped to 0 .. budget); NULL: all `budget` rows are.  Rows
 *            beyond the count are never read
 *   dets     dev f32 [m, E]
 *   out      dev f64 [n, m], row-major
 * A track with no valid row gives a row of +inf (never admissible to busca_linear_assignment); a zero-norm vector gives NaN as the
 * IEEE division does (never admissible either), and a NaN among a track's distances makes the reduced cost NaN.
 * budget = 1 with slot = count = NULL is the plain [n,E] x [m,E] case (matching.embedding_distance, GHOST with one proxy per track):
 * a 16-track x 64-detection tile per workgroup.  Otherwise one workgroup per (track, 64-detection tile) walks the track's rows 16 at a
 * time.
 *
 * Arithmetic: float64 on operands converted from f32 (v_mfma_f64_16x16x4_f64), every sum in a fixed order, no atomics:
 *   - a dot product <x, y> runs over k in steps of 16; within a step come four matrix instructions t = 0..3, and instruction t adds the
 *     four products at k = 16 s + 4 b + t, b = 0..3, to the accumulator;
 *   - the squared norms <g, g> and <d, d> are dot products of the same kind on the same loaded values, so two identical vectors give
 *     <g, d> = <g, g> = <d, d> bit for bit and a distance of exactly 0 (sqrt(x * x) = x in IEEE arithmetic);
 *   - MEAN: each of the 64 lanes that share a detection column adds its rows r = 16 T + b + 4 q (tile T ascending, q = 0..3 inside it)
 *     to a private sum; the four sums b = 0..3 are then added as (s_b + s_(b^1)) + (s_(b^2) + s_(b^3)) and divided by the count.
 *     MIN / MAX take the same route.
 * A track's row of `out` depends on that track's samples and the detections only - not on n, on the other tracks or on its position in
 * the call - and the result is bit-identical from run to run.
 *
 * E: a multiple of 16 in 16 .. 2048; gallery and dets 16-byte aligned.  n = 0 or m = 0: returns 0 and launches nothing.  Negative
 * sizes, budget < 1, a bad E, an unknown reduce or flag, a NULL gallery / dets / out, a misaligned pointer, more workgroups than a grid
 * holds: BUSCA_EINVAL with a message.  Asynchronous on `stream`, allocates nothing, synchronises nothing. */
int busca_appearance_cost(busca_ctx* ctx, const float* gallery, const int32_t* slot, const int32_t* count, int32_t n, int32_t budget,
                          const float* dets, int32_t m, int32_t E, int32_t reduce, int32_t flags, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
