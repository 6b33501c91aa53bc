/*
 * busca_mgframe.h - the GHOST frames of many sequences on one store as one chain, as calls of libbusca_mgframe.so: a context-free library next to
 * libbusca_gframe.so (busca_gframe.h), whose interface stays what it is.  The sequences share one store (the motion state and the feature rings of
 * busca_gframe.h, S slots), one slot list, one detection table, one list of free slots and a list of warps; a table of problems says which rows of
 * each a frame takes.  The costs come out as one padded [batch, R, M] block that busca_linear_assignment (busca_assign.h) takes together with its
 * `dims` table, and the match vectors [batch, R] and [batch, M] are filtered and applied as they are: a time step of any number of sequences is
 * busca_mgframe_advance, the proxy launches on the whole slot list, busca_mgframe_distance, (busca_mgframe_thresholds,) busca_mgframe_cost, the
 * solver, busca_mgframe_keep and busca_mgframe_apply.
 *
 * The slot list  slot  dev i32 [n_total]  is ordered group-wise: all problems' active slots, then all problems' in-patience inactive slots, then all
 *   idle ones.  A problem owns one range of each group, so busca_ghost_proxies and busca_store_mv_avg (with its num_active split) run unchanged on
 *   the whole list.  Tables "indexed as the slot list" (pos_out, track_label, a table of proxy rows) have one row per list row.
 *
 * The problem table:  problems  dev i32 [batch, 13]:
 *     act_begin, na_k, inact_begin, ni_k, idle_begin, nidle_k, det_begin, m_k, free_begin, n_free_k, warp_k, frame_k, flags_k
 *   problem k is the active rows slot[act_begin .. act_begin + na_k), the inactive rows slot[inact_begin .. + ni_k) and the idle rows slot[idle_begin
 *   .. + nidle_k) of the slot list, the detections [det_begin .. det_begin + m_k) of the detection tables [m_total], the free slots free_slot[free_begin
 *   .. + n_free_k) of the free list [f_total] and the warp warps[warp_k] of dev f32 [n_warps, 6] (-1: none); frame_k is the frame number its rings
 *   store; flags_k: BUSCA_MGFRAME_DIFF32 (the step's differences are float32) and BUSCA_MGFRAME_STEP (its rows are stepped; without it they are
 *   warped only).  n_k = na_k + ni_k are the rows of its cost matrix.
 *   The slab of problem k is [R, M] with row stride M: its active rows are slab rows 0 .. na_k - 1, its inactive rows start at slab row
 *   inact_row >= 0 (a fixed row, the same for every problem: assign_separately, R = inact_row + max ni_k) or, with inact_row < 0, at slab row na_k
 *   (contiguous: the same-time assignment, R = N = max n_k).  det_track holds slab rows.
 *   Skipped problems.  The table lives on the device and is not read back, so a bad row cannot be refused: a row with a negative size or begin, with
 *   a range that leaves [0, n_total], [0, m_total] or [0, f_total], with n_k > N, m_k > M or n_k + nidle_k > L, with warp_k < -1 or >= n_warps, or
 *   whose inactive rows do not fit the slab (na_k > inact_row or inact_row + ni_k > R; contiguous: n_k > R) skips its problem in every call - nothing
 *   of it is read or written.  Every call takes all of n_total, m_total, f_total, n_warps, N, M, L, R and inact_row, so that all judge a row alike.
 *
 * Conventions of every call, those of busca_gframe.h and busca_msframe.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_mgframe_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises; one kernel launch per call;
 *   - every argument is checked before the first HIP call, so a refusal and a no-op need no GPU;
 *   - refused with -1: negative sizes (inact_row may be negative) or device, inact_row > R, batch > 65535 (a grid dimension), R or L beyond 65535,
 *     a NULL required pointer (`problems` always; `slot` where a call reads it: advance, distance without by_list, apply), a float64 pointer
 *     not 8-byte or an int32 / float32 pointer not 4-byte aligned, and what each call lists;
 *   - a slot outside 0 .. S-1 is skipped and touches no memory;
 *   - padding - what lies outside a problem's rows and columns in a [batch, R, M], [batch, R], [batch, M] or [batch, 2] block - and everything of a
 *     skipped problem is never written;
 *   - the arithmetic is that of busca_gframe_advance / _cost / _keep / _apply, busca_ghost_distance and busca_ghost_thresholds, never contracted
 *     to a multiply-add: the same device functions, included.
 */
#ifndef BUSCA_MGFRAME_H
#define BUSCA_MGFRAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_MGFRAME_OK 0
#define BUSCA_MGFRAME_EINVAL (-1)
#define BUSCA_MGFRAME_EHIP (-2)

#define BUSCA_MGFRAME_PROBLEM_WORDS 13
#define BUSCA_MGFRAME_DIFF32 1 /* flags_k */
#define BUSCA_MGFRAME_STEP 2

#define BUSCA_MGFRAME_MAX_DETS 2048   /* most detections of one problem: BUSCA_GFRAME_MAX_DETS */
#define BUSCA_MGFRAME_MAX_BATCH 65535 /* most problems of one call */
#define BUSCA_MGFRAME_MAX_ROWS 65535  /* most slab rows R and listed rows L of one problem (a grid dimension) */
#define BUSCA_MGFRAME_E_MIN 16        /* the feature widths of busca_mgframe_distance: multiples of 16 in BUSCA_APPEAR_E_MIN .. BUSCA_APPEAR_E_MAX */
#define BUSCA_MGFRAME_E_MAX 2048
#define BUSCA_MGFRAME_MEDIAN_BUDGET_MAX 256 /* BUSCA_GHOST_MEDIAN_BUDGET_MAX */

/* 1000 * major + minor; this header is version 1000. */
int busca_mgframe_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_mgframe_last_error(void);

/* busca_gframe_advance of every problem in one launch of a grid of (L, batch) 64-lane workgroups: listed row x of problem k - its active rows, then
 * its inactive, then its idle ones - is warped with warps[warp_k] (when warp_k >= 0), and then, behind a workgroup barrier, stepped when flags_k
 * has STEP (the velocity from the window for the active rows, the stored one for the others; DIFF32 as flags_k says).
 *   pos_out  dev f64 [n_total, 4], indexed as the slot list: the positions after the step of the rows of the stepped problems (a skipped slot gets
 *            a row of NaN); the other rows are not written
 * Bit-equal to busca_gframe_advance problem by problem.  The listed slots must be distinct across the batch.  Refused: H < 2, last_n_frames < 2,
 * warps NULL with n_warps > 0.  batch = 0, L = 0 or n_total = 0: returns 0 and launches nothing. */
int busca_mgframe_advance(double* hist, const int32_t* frames, const int32_t* count, const int32_t* newest, double* pos, double* vel, int32_t S, int32_t H,
                          const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total, const float* warps, int32_t n_warps,
                          const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R, int32_t inact_row, int32_t last_n_frames,
                          double* pos_out, int32_t device, void* stream);

/* The diagonal blocks of busca_ghost_distance into the slab: out[k, r, j] for slab row r of problem k and j < m_k is the entry busca_ghost_distance
 * writes for that track and that detection, bit for bit.  One workgroup per (slab row, 64-detection tile, problem), four waves; a workgroup whose
 * row is padding, whose tile lies beyond m_k or whose problem is skipped leaves before any barrier, whole.
 *   gallery  dev f32 [rows, budget, E], count dev i32 [rows] or NULL (every row holds `budget` samples), dets dev f32 [m_total, E]; both 16-byte aligned
 *   by_list  0: `gallery` is the store's, rows = S, and a track's samples are those of its slot (a slot outside 0 .. S-1: a row of +inf);
 *            != 0: `gallery` is a table indexed as the slot list (rows = n_total; with budget 1 and MIN, the proxy rows of busca_ghost_proxies or
 *            busca_store_mv_avg on the whole list)
 *   reduce   BUSCA_GHOST_MIN .. BUSCA_GHOST_MEDIAN (busca_ghost.h), MEDIAN with its LDS staging and budget <= 256
 *   groups   bit 0: the active rows are served, bit 1: the inactive rows - two calls where the two groups take different routes
 * Refused: budget < 1, a bad E, an unknown reduce, groups outside 1 .. 3, by_list with rows != n_total.  batch, R, M, n_total or m_total = 0: returns 0
 * and launches nothing. */
int busca_mgframe_distance(const float* gallery, const int32_t* count, int32_t rows, int32_t by_list, int32_t budget, const float* dets, int32_t E,
                           int32_t reduce, int32_t groups, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total,
                           int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R, int32_t inact_row,
                           double* out, int32_t device, void* stream);

/* busca_ghost_thresholds per problem, one 256-lane workgroup each: thr[k, 0] = mean - k_act * std over the active rows of slab k, thr[k, 1] over its
 * inactive rows.  A thread's i-th entry is entry i of the group's [rows, m_k] block in row-major order, not of the padded slab: every sum has the
 * single call's order and bits.  A group without rows (or m_k = 0) leaves its entry as it was.
 *   which    bit 0: thr[k, 0] is computed, bit 1: thr[k, 1]
 *   thr      dev f64 [batch, 2]
 * Refused: which outside 1 .. 3.  batch, R, M, n_total or m_total = 0: returns 0 and launches nothing. */
int busca_mgframe_thresholds(const double* cost, double k_act, double k_inact, int32_t which, int32_t S, const int32_t* slot, int32_t n_total,
                             int32_t m_total, int32_t f_total, int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L,
                             int32_t R, int32_t inact_row, double* thr, int32_t device, void* stream);

/* busca_gframe_cost on every slab, in place: the class mask (track_label dev i32 [n_total] indexed as the slot list, det_label dev i32 [m_total], or
 * both NULL), the blend with 1 - IoU(pos, det_boxes) (pos dev f64 [n_total, 4]: busca_mgframe_advance's pos_out, or NULL: no blend; det_boxes dev
 * f64 [m_total, 4]), nan_first against thr[k] (dev f64 [batch, 2], or NULL).  A grid of (ceil(M / 64), ceil(R / 16), batch) 256-lane workgroups;
 * only the entries of a problem's rows and columns are written.
 * Refused: a NaN alpha, one label vector without the other, det_boxes NULL with pos.  batch, R, M, n_total or m_total = 0: returns 0, launches nothing. */
int busca_mgframe_cost(double* cost, const double* pos, const double* det_boxes, double alpha, const int32_t* track_label, const int32_t* det_label,
                       const double* thr, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total, int32_t n_warps,
                       const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R, int32_t inact_row, int32_t device,
                       void* stream);

/* busca_gframe_keep per problem on the batched match vectors of busca_linear_assignment (row_to_col dev i32 [batch, R], col_to_row dev i32
 * [batch, M]; a row index relative to the first row of the stage).
 *   stage     0: all rows of the problem (contiguous slabs); 1: its active rows; 2: its inactive rows - the solver ran on cost + inact_row * M
 *   track_det dev i32 [batch, R] by slab row, det_track dev i32 [batch, M] holding slab rows, thr dev f64 [batch, 2], merge: as busca_gframe_keep
 *   mask      != 0: NaN is written into the problem's own inactive rows at each kept column (stage 1 only)
 * Refused: stage outside 0 .. 2, mask with a stage other than 1.  batch, M or m_total = 0: returns 0 and launches nothing. */
int busca_mgframe_keep(double* cost, const int32_t* row_to_col, const int32_t* col_to_row, const double* thr, int32_t* track_det, int32_t* det_track,
                       int32_t stage, int32_t merge, int32_t mask, int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total,
                       int32_t n_warps, const int32_t* problems, int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R, int32_t inact_row,
                       int32_t device, void* stream);

/* busca_gframe_apply per problem in one launch of (R + M) * batch 64-lane workgroups: the kept matches of slab row x < R into both rings of its slot
 * with frame_k, and for column j < m_k of problem k Track.__init__ when det_track[k, j] < 0 and may_start[det_begin + j] != 0, into
 * free_slot[free_begin + rank], the rank counted among such columns of its own problem below j.
 *   det_feat  dev f32 [m_total, E], det_boxes dev f64 [m_total, 4], may_start dev u8 [m_total], free_slot dev i32 [f_total] (NULL with f_total = 0)
 *   det_slot  dev i32 [batch, M]: the slot written, -1 where nothing happened, -2 where the problem's free range ran out
 * The listed slots and the free slots must be distinct across the whole batch: the caller's contract.
 * Refused: H < 2, budget or E below 1, M beyond BUSCA_MGFRAME_MAX_DETS.  batch, M or m_total = 0: returns 0 and launches nothing. */
int busca_mgframe_apply(double* hist, int32_t* frames, int32_t* m_count, int32_t* m_newest, double* pos, double* vel, int32_t H, float* gallery,
                        int32_t* g_count, int32_t* g_newest, uint8_t* mv_seen, int32_t budget, int32_t E, const int32_t* track_det,
                        const int32_t* det_track, const float* det_feat, const double* det_boxes, const uint8_t* may_start, const int32_t* free_slot,
                        int32_t S, const int32_t* slot, int32_t n_total, int32_t m_total, int32_t f_total, int32_t n_warps, const int32_t* problems,
                        int32_t batch, int32_t N, int32_t M, int32_t L, int32_t R, int32_t inact_row, int32_t* det_slot, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
