/*
 * busca_mframe.h - the ByteTrack frames of many sequences on one store as one chain, as calls of libbusca_mframe.so: a context-free library next to
 * libbusca_frame.so (busca_frame.h), whose interface stays what it is.  The sequences share one Kalman store (mean f64 [S, 8], cov f64 [S, 8, 8],
 * as busca_track.h lays them out), one slot list, one detection table and one list of free slots; a table of problems says which rows of the three
 * each frame takes.  The cost slabs come out as one padded [batch, 2, N, M] block with the layout busca_assign_stages (busca_assign_stages.h) takes
 * together with its `dims` table, and the solver's padded match vectors [batch, N] and [batch, M] are applied as they are: a time step of any number
 * of sequences is one prediction (busca_track_kalman_predict on the concatenated slot list), busca_mframe_cost, one call of the solver and
 * busca_mframe_apply.
 *
 * The problem table:  problems  dev i32 [batch, 6]:  row_begin, n_k, det_begin, m_k, free_begin, n_free_k
 *   problem k is the rows slot[row_begin .. row_begin + n_k) of the slot list [n_total] (within a problem the pool rows first, then the unconfirmed
 *   ones, as busca_frame.h has them), the detections [det_begin .. det_begin + m_k) of the detection tables [m_total] and the free slots
 *   free_slot[free_begin .. free_begin + n_free_k) of the free list [f_total].
 *   Skipped problems.  The table lives on the device and is not read back, so a bad row cannot be refused: a row with a negative entry, with a range
 *   that leaves [0, n_total], [0, m_total] or [0, f_total], or with n_k > N or m_k > M skips its problem in both calls - nothing of it is read or
 *   written.
 *
 * Conventions of every call, those of busca_frame.h and busca_rounds.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_mframe_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes or device, a NULL required pointer, a float64 pointer not 8-byte or an int32 pointer not 4-byte aligned,
 *     batch > 65535 (a grid dimension), and what each call lists;
 *   - the arithmetic is that of busca_frame_cost and busca_frame_apply, float64 and never contracted to a multiply-add: the same device code, included.
 */
#ifndef BUSCA_MFRAME_H
#define BUSCA_MFRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_MFRAME_OK 0
#define BUSCA_MFRAME_EINVAL (-1)
#define BUSCA_MFRAME_EHIP (-2)

#define BUSCA_MFRAME_MAX_DETS 2048  /* most detections of one problem of busca_mframe_apply: BUSCA_FRAME_MAX_DETS */
#define BUSCA_MFRAME_MAX_BATCH 65535 /* most problems of one call */

/* 1000 * major + minor; this header is version 1000. */
int busca_mframe_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_mframe_last_error(void);

/* The cost slabs of `batch` frames in one launch:  out  dev f64 [batch, 2, N, M], row stride M, plane stride N * M.
 *   det_tlbr   dev f64 [m_total, 4];  det_score  dev f64 [m_total] or NULL;  det_class  dev u8 [m_total], as busca_frame_cost reads them
 *   f_total    the length of the free list busca_mframe_apply will be given: the table is judged here as it is there
 * Valid region.  out[k, p, i, j] for i < n_k, j < m_k holds the bits busca_frame_cost writes to out[p, i, j] for problem k alone: plane 0 fuse_score
 *   (det_score NULL: plain 1 - IoU) at the columns of class 0, plane 1 plain 1 - IoU at the columns of class 1, +inf everywhere else, the rows of
 *   skipped slots (an entry < 0 or >= S) included.
 *   status     dev i32 [batch, N] or NULL: 0 at [k, i] for i < n_k of the problems that have a tile (n_k > 0 and m_k > 0)
 * Padding.  Everything else of `out` and `status` is NOT written: the solver never reads outside `dims`.
 * Refused: N beyond 65535 * 16 (the grid's second dimension).  batch = 0, N = 0 or M = 0 (and n_total = 0 or m_total = 0, with which every problem
 * is empty or skipped): returns 0 and launches nothing. */
int busca_mframe_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_tlbr,
                      const double* det_score, const uint8_t* det_class, int32_t m_total, int32_t f_total, const int32_t* problems, int32_t batch,
                      int32_t N, int32_t M, double* out, int32_t* status, int32_t device, void* stream);

/* The match vectors of busca_assign_stages over the batch, enqueued earlier on the same stream, applied to the state in one launch of
 * (N + M) * batch workgroups.
 *   row_to_col  dev i32 [batch, N]: row i < n_k of problem k with 0 <= row_to_col[k, i] < m_k gets KalmanFilter.update of its slot with the matched
 *               detection of its own problem, det_xyah[det_begin + row_to_col[k, i]]
 *   status      dev i32 [batch, N] or NULL: at [k, i] for i < n_k, 1 where the projected covariance is not positive definite (that slot keeps its
 *               state), 0 elsewhere, also for an unmatched row and a skipped slot
 *   col_to_row  dev i32 [batch, M];  det_xyah  dev f64 [m_total, 4];  det_score  dev f64 [m_total] or NULL;  det_class  dev u8 [m_total]
 *   a column j < m_k of problem k starts a track by the rule of busca_frame_apply, with the one `det_thresh` of the batch, and is initiated into
 *               free_slot[free_begin + rank], rank counted among the starting columns below j of its own problem: the same slots run after run,
 *               no atomics, and no problem takes from another's free range
 *   free_slot   dev i32 [f_total] (NULL with f_total = 0).  The slots >= 0 of the slot list and the free slots must be distinct across the whole
 *               batch: that is the caller's contract - otherwise two workgroups race on a state, though every access stays inside the arrays.
 *               An entry outside 0 .. S-1 is skipped like any other slot
 *   new_slot    dev i32 [batch, M]: at [k, j] for j < m_k the slot taken (as listed, also when it was skipped); -1 for a column that starts no
 *               track; -2 for one that would but has rank >= n_free_k - nothing is written for it
 * Padding.  The words of status and new_slot outside (n_k, m_k), and those of skipped problems, are NOT written.
 * Refused: a NaN det_thresh, M beyond BUSCA_MFRAME_MAX_DETS, N + M beyond what a grid holds.  batch = 0, or N = 0 and M = 0 together: returns 0 and
 * launches nothing; with N = 0 or n_total = 0 the row operands may be NULL, with M = 0 or m_total = 0 the column operands. */
int busca_mframe_apply(double* mean, double* cov, int32_t S, const int32_t* slot, int32_t n_total, const int32_t* row_to_col,
                       const int32_t* col_to_row, const double* det_xyah, const double* det_score, const uint8_t* det_class, int32_t m_total,
                       double det_thresh, const int32_t* free_slot, int32_t f_total, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                       int32_t* new_slot, int32_t* status, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
