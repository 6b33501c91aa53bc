/*
 * busca_assign.h - the linear-assignment entry point of libbusca_hip.so: the last step of a tracker's association round, solved
 * on the device.  Same conventions as busca_hip.h (return codes, dev / host pointers, `stream`, one ctx per GPU/process); the
 * context and the error codes are the ones declared there.
 */
#ifndef BUSCA_ASSIGN_H
#define BUSCA_ASSIGN_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_ASSIGN_MAX 2048 /* largest n and m of one problem (the solver's state lives in LDS) */

/* matching.linear_assignment (adapters/ByteTrack/yolox/tracker/matching.py:39-50: lap.lapjv(cost, extend_cost=True, cost_limit=limit))
 * and the solver inside min_cost_matching (adapters/StrongSORT/deep_sort/linear_assignment.py:15-85, with limit = max_distance + 1e-5)
 * for `batch` problems in one launch.  Both choose a partial matching M of pairs with c_ij < limit that minimises the sum of
 * (c_ij - limit) over M; a NaN or +inf cost is never admissible; a row may always stay unmatched at cost 0.  Exact shortest
 * augmenting paths with row / column potentials in float64, one workgroup per problem; ties go to the lowest column index, so the
 * result is the same from run to run.
 *   cost        dev f64 [batch, n, m], row-major
 *   dims        dev i32 [batch, 2] or NULL: the valid (n_k <= n, m_k <= m) of problem k inside its padded [n, m] slab (what lies outside
 *               is never read); NULL: every problem is n x m.  A pair outside 0..n / 0..m gives that problem status 1.
 *   row_to_col  dev i32 [batch, n]: the matched column or -1; -1 for padding rows
 *   col_to_row  dev i32 [batch, m] or NULL: likewise
 *   duals       dev f64 [batch, n + m] or NULL: the final row potentials u [n] and column potentials v [m] of the reduced problem:
 *               u_i + v_j <= c_ij - limit on admissible pairs with equality on the matches, u <= 0, v <= 0, and 0 on unmatched (and
 *               padding) rows and columns - the certificate of optimality
 *   objective   dev f64 [batch] or NULL: the sum of c_ij over the matches
 *   status      dev i32 [batch] or NULL: 0 = solved; 1 = a loop bound was exhausted (at most n_k augmentations of at most m_k + 1 scan
 *               steps each; only non-finite arithmetic, e.g. a -inf cost, gets there): row_to_col / col_to_row are all -1, duals 0,
 *               objective NaN
 * batch, n or m = 0: returns 0 and launches nothing.  Negative sizes, a NaN limit, NULL cost or row_to_col, n or m beyond
 * BUSCA_ASSIGN_MAX: BUSCA_EINVAL.  Asynchronous on `stream`, allocates nothing.  The cost matrix is staged in LDS when it fits beside
 * the solver's state (160 KiB per workgroup) and read from global memory otherwise, with identical results; option "assign_stage"
 * (BUSCA_ASSIGN_STAGE at busca_ctx_create): -1 = that rule, 0 = never stage (A/B, tests); "last_assign_staged" reads what the last
 * launch did. */
int busca_linear_assignment(busca_ctx* ctx, const double* cost, int32_t batch, int32_t n, int32_t m, const int32_t* dims, double limit,
                            int32_t* row_to_col, int32_t* col_to_row, double* duals, double* objective, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
