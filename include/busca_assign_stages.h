/*
 * busca_assign_stages.h - staged linear assignment of libbusca_hip.so: a chain of assignment problems over one set of rows and columns,
 * each stage choosing among what the earlier ones left over, solved in one launch.  It is what StrongSORT's Tracker._match does with
 * matching_cascade and its IoU stage (adapters/StrongSORT/deep_sort/tracker.py:214-252, deep_sort/linear_assignment.py:88-162).
 * Same conventions as busca_hip.h and busca_assign.h, whose context, error codes and BUSCA_ASSIGN_MAX are used here.  A header of its
 * own: busca_assign.h stays the declaration of the one-problem solver, unchanged.
 */
#ifndef BUSCA_ASSIGN_STAGES_H
#define BUSCA_ASSIGN_STAGES_H

#include "busca_assign.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_ASSIGN_STAGES_MAX 128 /* most stages of one call */

/* One stage: the plane of `cost` it reads and its limit (a pair is admissible when its cost is < limit; with a NaN limit none is). */
typedef struct busca_assign_stage {
    int32_t plane;
    int32_t reserved; /* 0 */
    double limit;
} busca_assign_stage;

/* `batch` chains of n_stages assignment problems in one launch, one workgroup per chain.
 *   cost        dev f64 [batch, planes, n, m], row-major: the matrices the stages choose from (StrongSORT: plane 0 the gated appearance
 *               cost, plane 1 the IoU cost)
 *   dims        dev i32 [batch, 2] or NULL, as in busca_linear_assignment: the valid (n_k, m_k) corner of problem k; a pair outside
 *               0..n / 0..m gives that problem status 1
 *   stages      dev busca_assign_stage [n_stages], 1 <= n_stages <= BUSCA_ASSIGN_STAGES_MAX, shared by all problems of the batch
 *   first       dev i32 [batch, n]: row i takes part in stage first[i]
 *   again       dev i32 [batch, n] or NULL: a row still unmatched when stage again[i] begins takes part in that one too.  In both, a
 *               value outside 0 .. n_stages-1 means "never"; an again[i] <= first[i] (as given) means "never"
 *   row_to_col  dev i32 [batch, n]: the matched column or -1; -1 for padding rows
 *   col_to_row  dev i32 [batch, m] or NULL: likewise
 *   row_stage   dev i32 [batch, n] or NULL: the stage that matched the row, or -1
 *   status      dev i32 [batch] or NULL: 0 = solved; 1 = a loop bound was exhausted, as in busca_linear_assignment (e.g. a -inf cost);
 *               2 = a stage record names a plane outside 0 .. planes-1 (nothing is read through it; the table being the batch's, every
 *               problem of the call gets it).  With 1 or 2 every output of that problem is -1; a problem with status 1 leaves the others
 *               of its batch as they are
 * Stages run in ascending order.  Stage s is exactly the problem busca_linear_assignment solves with that stage's limit on the compacted
 * matrix of its member rows (ascending) and the columns no earlier stage matched (ascending), read from the stage's plane - the same
 * pairs, ties included, not merely an equally cheap matching.  Matches are final: a matched column is withdrawn from all later stages
 * and a matched row never re-enters one.  A stage without member rows or without free columns does nothing, and costs nothing.
 * batch, n or m = 0: returns 0 and launches nothing.  Negative sizes, n_stages out of range, NULL cost / stages / first / row_to_col, n
 * or m beyond BUSCA_ASSIGN_MAX: BUSCA_EINVAL.  Asynchronous on `stream`, allocates nothing.  The member rows of a stage are staged in LDS
 * when they fit beside the solver's state (160 KiB per workgroup) and read from global memory otherwise, with identical results; option
 * "assign_stage" = 0 turns the staging off (A/B, tests) and "last_assign_staged" reads whether the last launch had it on. */
int busca_assign_stages(busca_ctx* ctx, const double* cost, int32_t planes, int32_t batch, int32_t n, int32_t m, const int32_t* dims,
                        const void* stages, int32_t n_stages, const int32_t* first, const int32_t* again,
                        int32_t* row_to_col, int32_t* col_to_row, int32_t* row_stage, int32_t* status, void* stream);

/* The bytes of LDS a busca_assign_stages launch of n x m asks for, by the function that sizes the launch: the solver's state and, with
 * staged != 0, room for the member rows of a stage - n x m doubles where that fits, else what is left of 160 KiB.  -1 for sizes outside
 * 0 .. BUSCA_ASSIGN_MAX.  Host only, touches no device. */
int64_t busca_assign_stages_lds_bytes(int32_t n, int32_t m, int32_t staged);

#ifdef __cplusplus
}
#endif
#endif
