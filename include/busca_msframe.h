/*
 * busca_msframe.h - the StrongSORT frames of many sequences on one store as one chain, as calls of libbusca_msframe.so: a context-free library next
 * to libbusca_sframe.so (busca_sframe.h), whose interface stays what it is.  The sequences share one store (mean f64 [S, 8], cov f64 [S, 8, 8], feat
 * f32 [S + 1, E], as busca_sframe.h lays them out), one slot list, one detection table, one list of free slots and a list of camera matrices; a table
 * of problems says which rows of each a frame takes.  The cost slabs come out as one padded [batch, 2, N, M] block with the layout
 * busca_assign_stages (busca_assign_stages.h) takes together with its `dims` table, and the solver's padded match vectors [batch, N] and [batch, M]
 * are applied as they are: a time step of any number of sequences is busca_msframe_advance, busca_msframe_cost, one call of the solver and
 * busca_msframe_apply.
 *
 * The problem table:  problems  dev i32 [batch, 7]:  row_begin, n_k, det_begin, m_k, free_begin, n_free_k, matrix_k
 *   problem k is the rows slot[row_begin .. row_begin + n_k) of the slot list [n_total] - `first`, `again` and `stale` are indexed as the slot list
 *   is -, the detections [det_begin .. det_begin + m_k) of the detection tables [m_total], the free slots free_slot[free_begin .. free_begin +
 *   n_free_k) of the free list [f_total] and the camera matrix matrices[matrix_k] of dev f64 [n_matrices, 9] (-1: no camera update).
 *   Skipped problems.  The table lives on the device and is not read back, so a bad row cannot be refused: a row with a negative size or begin, with
 *   a range that leaves [0, n_total], [0, m_total] or [0, f_total], with n_k > N or m_k > M, or with matrix_k < -1 or >= n_matrices skips its
 *   problem in all three calls - nothing of it is read or written.  Every call takes all of n_total, m_total, f_total, n_matrices, N and M, so that
 *   the three judge a row alike.
 *
 * Conventions of every call, those of busca_sframe.h and busca_mframe.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_msframe_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 / float32 pointer not 4-byte
 *     aligned, batch > 65535 (a grid dimension), and what each call lists;
 *   - the arithmetic is that of busca_sframe_advance, busca_appearance_cost, busca_sframe_cost and busca_sframe_apply, never contracted to a
 *     multiply-add: the same device code, included.
 */
#ifndef BUSCA_MSFRAME_H
#define BUSCA_MSFRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_MSFRAME_OK 0
#define BUSCA_MSFRAME_EINVAL (-1)
#define BUSCA_MSFRAME_EHIP (-2)

/* `flags` of busca_msframe_cost: the values of BUSCA_SFRAME_MC and BUSCA_SFRAME_CLAMP (busca_sframe.h), for plane 0 */
#define BUSCA_MSFRAME_MC 1
#define BUSCA_MSFRAME_CLAMP 2

#define BUSCA_MSFRAME_MAX_DETS 2048   /* most detections of one problem of busca_msframe_apply: BUSCA_SFRAME_MAX_DETS */
#define BUSCA_MSFRAME_MAX_BATCH 65535 /* most problems of one call */
#define BUSCA_MSFRAME_E_MIN 16        /* the feature widths of busca_msframe_cost: multiples of 16 in BUSCA_APPEAR_E_MIN .. BUSCA_APPEAR_E_MAX */
#define BUSCA_MSFRAME_E_MAX 2048

/* 1000 * major + minor; this header is version 1001 (1001: busca_msframe_advance warps the stored
 * mean before it predicts, as busca_sframe_advance 1001 does). */
int busca_msframe_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_msframe_last_error(void);

/* For the problems with matrix_k >= 0, Track.camera_update of the stored mean of every row with matrices[matrix_k] (dev f64 [n_matrices, 9],
 * row-major 3 x 3; NULL with n_matrices = 0), and then Track.predict of every row of every problem in place.  A grid of (N, batch) 64-lane workgroups: row x of
 * problem k finds itself from its block index, without a table of its own and without atomics.  Bit-equal to busca_sframe_advance problem by
 * problem.  batch = 0, N = 0 or n_total = 0: returns 0 and launches nothing. */
int busca_msframe_advance(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total,
                          const double* matrices, int32_t n_matrices, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t device,
                          void* stream);

/* The cost slabs of `batch` frames in one launch:  out  dev f64 [batch, 2, N, M], row stride M, plane stride N * M.
 *   det_xyah, det_tlwh  dev f64 [m_total, 4];  det_feat  dev f32 [m_total, E];  feat  dev f32 [S + 1, E] (both 16-byte aligned);
 *   stale  dev u8 [n_total] or NULL;  first, again  dev i32 [n_total] (again may be NULL: never);  depth, gated_cost, flags, mc_lambda, max_distance,
 *   max_iou_distance: the batch's, as busca_sframe_cost reads them
 * Valid region.  out[k, p, i, j] for i < n_k, j < m_k holds the bits busca_sframe_cost writes to out[p, i, j] for problem k alone, given as `cost`
 *   the matrix busca_appearance_cost(feat as a [S + 1, 1, E] gallery, slot, NULL, n_k, 1, det_feat, m_k, E, BUSCA_APPEAR_MIN, 0) writes.  That matrix
 *   is never formed: a workgroup computes the appearance entries of its 16 x 64 tile itself, on the matrix instructions and in the order of sums
 *   of busca_appearance_cost - an entry depends only on its two vectors (busca_appearance.h) -, and only for a tile one of whose rows is gated
 *   (0 <= first < depth and a slot in 0 .. S-1).  Only the diagonal blocks of the batch are computed.
 *   status     dev i32 [batch, N] or NULL: at [k, i] for i < n_k of the problems that have a tile (n_k > 0 and m_k > 0), the word
 *              busca_sframe_cost writes
 * Padding.  Everything else of `out` and `status` is NOT written: the solver never reads outside `dims`.
 * Refused: depth < 0, unknown flag bits, NaN mc_lambda with MC, NaN max_distance with CLAMP, NaN max_iou_distance, E not a multiple of 16 in
 * 16 .. 2048, N beyond 65535 * 16 (the grid's second dimension).  batch = 0, N = 0 or M = 0 (and n_total = 0 or m_total = 0, with which every
 * problem is empty or skipped): returns 0 and launches nothing. */
int busca_msframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_xyah,
                       const double* det_tlwh, const float* det_feat, int32_t m_total, int32_t f_total, int32_t n_matrices, const uint8_t* stale,
                       const float* feat, int32_t E, double gated_cost, int32_t flags, double mc_lambda, double max_distance, double max_iou_distance,
                       const int32_t* first, const int32_t* again, int32_t depth, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                       double* out, int32_t* status, int32_t device, void* stream);

/* The match vectors of busca_assign_stages over the batch, enqueued earlier on the same stream, applied to the state in one launch of
 * (N + M) * batch 64-lane workgroups.
 *   row_to_col  dev i32 [batch, N]: row i < n_k of problem k with 0 <= row_to_col[k, i] < m_k is Track.update of its slot with the matched
 *               detection of its own problem - the EMA feature row, then the NSA Kalman update -, as busca_sframe_apply does it
 *   status      dev i32 [batch, N] or NULL: at [k, i] for i < n_k, 1 where the projected covariance is not positive definite (that slot keeps its
 *               Kalman state, its feature row is written all the same), 0 elsewhere, also for an unmatched row and a skipped slot
 *   col_to_row  dev i32 [batch, M];  det_xyah  dev f64 [m_total, 4];  det_conf  dev f64 [m_total] or NULL (confidence 0);  det_feat  dev f32
 *               [m_total, E];  feat  dev f32 [S + 1, E];  alpha: the batch's
 *   a column j < m_k of problem k with col_to_row[k, j] < 0 starts a track: KalmanFilter.initiate and the normalised feature into
 *               free_slot[free_begin + rank], rank counted among such columns below j of its own problem: the same slots run after run, no
 *               atomics, and no problem takes from another's free range
 *   free_slot   dev i32 [f_total] (NULL with f_total = 0).  The slots >= 0 of the slot list and the free slots must be distinct across the whole
 *               batch: that is the caller's contract - otherwise two workgroups race on a state, though every access stays inside the arrays.
 *               An entry outside 0 .. S-1 is skipped like any other slot
 *   new_slot    dev i32 [batch, M]: at [k, j] for j < m_k the slot taken (as listed, also when it was skipped); -1 for a matched column; -2 for one
 *               that would start a track but has rank >= n_free_k - nothing is written for it
 * Padding.  The words of status and new_slot outside (n_k, m_k), and those of skipped problems, are NOT written.
 * Refused: E < 1, a NaN alpha, M beyond BUSCA_MSFRAME_MAX_DETS, N + M beyond what a grid holds.  batch = 0, M = 0 or m_total = 0 (no row has a
 * match, no column is there): returns 0 and launches nothing - `status` is then not written; with N = 0 or n_total = 0 the row operands may be
 * NULL. */
int busca_msframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, const int32_t* row_to_col,
                        const int32_t* col_to_row, const double* det_xyah, const double* det_conf, const float* det_feat, int32_t m_total,
                        float* feat, int32_t E, double alpha, const int32_t* free_slot, int32_t f_total, int32_t n_matrices, const int32_t* problems,
                        int32_t batch, int32_t N, int32_t M, int32_t* new_slot, int32_t* status, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
