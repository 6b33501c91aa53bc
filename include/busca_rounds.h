/*
 * busca_rounds.h - the association rounds of many sequences in one launch, as calls of libbusca_rounds.so: a context-free library next to
 * libbusca_track.so (busca_track.h), whose interface stays what it is.  The sequences share one Kalman store (mean f64 [S, 8], cov f64 [S, 8, 8],
 * as busca_track.h lays them out), one slot list and one detection table; a table of problems says which rows of the two each round takes.  The
 * cost matrices come out as one padded [batch, N, M] slab with the layout busca_linear_assignment (busca_assign.h) takes together with its `dims`
 * table, so a round of any number of sequences is one prediction (busca_track_kalman_predict on the concatenated slot list), one call of
 * busca_rounds_cost and one call of the solver.
 *
 * Conventions of every call, those of busca_track.h:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_rounds_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises;
 *   - every argument is checked before the first HIP call, so a refusal and the no-ops need no GPU;
 *   - the arithmetic is that of busca_track_round_cost, float64 and never contracted to a multiply-add: the same device code, included.
 */
#ifndef BUSCA_ROUNDS_H
#define BUSCA_ROUNDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_ROUNDS_OK 0
#define BUSCA_ROUNDS_EINVAL (-1)
#define BUSCA_ROUNDS_EHIP (-2)

/* flags of busca_rounds_cost: the values and meanings of BUSCA_TRACK_FUSE_MOTION / _ONLY_POSITION / _GATE_ONLY */
#define BUSCA_ROUNDS_FUSE_MOTION 1
#define BUSCA_ROUNDS_ONLY_POSITION 2
#define BUSCA_ROUNDS_GATE_ONLY 4

/* 1000 * major + minor; this header is version 1000. */
int busca_rounds_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_rounds_last_error(void);

/* The cost matrices of `batch` association rounds in one launch.
 *   mean, cov   the store, dev f64 [S, 8] and [S, 8, 8] (cov is required with a motion flag only); read, never written
 *   slot        dev i32 [n_total]: the slot lists of all problems, one after the other (or overlapping: see "shared rows")
 *   det_tlbr    dev f64 [m_total, 4];  det_xyah  dev f64 [m_total, 4], required with a motion flag, else ignored;  det_score  dev f64 [m_total] or NULL
 *   problems    dev i32 [batch, 4]: slot_begin, n_k, det_begin, m_k - problem k is the tracks slot[slot_begin .. slot_begin + n_k) against the
 *               detections [det_begin .. det_begin + m_k)
 *   out         dev f64 [batch, N, M]: problem k's matrix in the top left corner of slab k, row stride M
 *   status      dev i32 [n_total] or NULL: the status word of slot[i] at position i
 * Valid region.  out[k, i, j] for i < n_k, j < m_k is what busca_track_round_cost writes to out[i, j] for the slot list slot[slot_begin .. + n_k)
 *   against the detections [det_begin .. + m_k) with the same `flags` and `lambda`, bit for bit; status[slot_begin + i] is its status[i] (1 where the
 *   projected covariance is not positive definite, 0 elsewhere; all 0 without a motion flag).
 * Padding.  Everything else in the slab is NOT written: the solver never reads outside `dims`.  The status words of a problem with m_k = 0 are not
 *   written either (it has no tile), nor are those no problem covers.
 * Skipped slots.  A slot entry < 0 or >= S gives a row of +inf, status 0, and touches no state.
 * Skipped problems.  The table lives on the device and is not read back, so a bad row cannot be refused: a row with a negative entry, with a range
 *   that leaves [0, n_total] or [0, m_total], or with n_k > N or m_k > M skips its problem - nothing of it is read or written.
 * Shared rows.  Problems may share rows of `slot` and detections: the inputs are only read, and a shared row's status word is the same from every
 *   problem that writes it.
 * Refused (-1; the message starts with "busca_rounds_cost:"): what busca_track_round_cost refuses - negative S, n_total, m_total or device, a NULL
 *   mean, slot, det_tlbr or out, a NULL cov or det_xyah with a motion flag, a float64 pointer not 8-byte or an int32 pointer not 4-byte aligned,
 *   flag bits other than the three, FUSE_MOTION together with GATE_ONLY, a NaN lambda - and: `problems` NULL or misaligned, a negative batch, N or M,
 *   batch > 65535 (the grid's third dimension), N > 65535 * 16 (its second).
 * batch = 0, N = 0 or M = 0 (and n_total = 0 or m_total = 0, with which every problem is empty): returns 0 and launches nothing. */
int busca_rounds_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_tlbr,
                      const double* det_xyah, const double* det_score, int32_t m_total, const int32_t* problems, int32_t batch, int32_t N, int32_t M,
                      int32_t flags, double lambda, double* out, int32_t* status, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
