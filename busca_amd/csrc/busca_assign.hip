// libbusca_hip.so, linear-assignment unit: the solver kernel, the staged solver and their C-ABI (include/busca_assign.h, include/busca_assign_stages.h).  A unit of its own so that the core unit's
// compile time does not grow (busca_amd/build.py compiles the units in parallel).
#include "busca_internal.hpp"

#pragma GCC visibility push(default)
#include "../../include/busca_assign.h"
#include "../../include/busca_assign_stages.h"
#pragma GCC visibility pop

#include "assign_kernel.hip.inc"
#include "assign_stages_kernel.hip.inc"

#define ASSIGN_LDS_MAX 163840        // one workgroup may take the CU's whole 160 KiB

extern "C" int busca_linear_assignment(busca_ctx* c, const double* cost, int32_t batch, int32_t n, int32_t m, const int32_t* dims, double limit,
                                       int32_t* row_to_col, int32_t* col_to_row, double* duals, double* objective, int32_t* status, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (batch < 0 || n < 0 || m < 0) return fail(c, BUSCA_EINVAL, "busca_linear_assignment: negative size");
    if (limit != limit) return fail(c, BUSCA_EINVAL, "busca_linear_assignment: the limit is NaN");
    if (batch == 0 || n == 0 || m == 0) return BUSCA_OK;
    if (!cost || !row_to_col) return fail(c, BUSCA_EINVAL, "busca_linear_assignment: null pointer");
    if (n > BUSCA_ASSIGN_MAX || m > BUSCA_ASSIGN_MAX)
        return fail(c, BUSCA_EINVAL, "busca_linear_assignment: %d x %d is beyond the supported %d x %d", n, m, BUSCA_ASSIGN_MAX, BUSCA_ASSIGN_MAX);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t state = assign_state_bytes(n, m), full = state + (size_t)8 * n * m;
    const bool staged = c->opt.assign_stage != 0 && full <= ASSIGN_LDS_MAX;
    const size_t lds = staged ? full : state;
    AssignArgs a{cost, (const int*)dims, n, m, limit, (int*)row_to_col, (int*)col_to_row, duals, objective, (int*)status};
    const bool wide = m > ASSIGN_ONE_WAVE_COLS;
    const void* kern = staged ? (wide ? (const void*)assign_kernel<true, ASSIGN_WAVES> : (const void*)assign_kernel<true, 1>)
                              : (wide ? (const void*)assign_kernel<false, ASSIGN_WAVES> : (const void*)assign_kernel<false, 1>);
    if (lds > 65536) {
        const int rc = ensure_lds(c, kern, ASSIGN_LDS_MAX);
        if (rc != BUSCA_OK) return rc;
    }
    TimedLaunch tl(c, (hipStream_t)stream);
    const dim3 grid(batch), block(wide ? ASSIGN_WAVES * 64 : 64);
    if (staged && wide) hipLaunchKernelGGL((assign_kernel<true, ASSIGN_WAVES>), grid, block, lds, (hipStream_t)stream, a);
    else if (staged) hipLaunchKernelGGL((assign_kernel<true, 1>), grid, block, lds, (hipStream_t)stream, a);
    else if (wide) hipLaunchKernelGGL((assign_kernel<false, ASSIGN_WAVES>), grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((assign_kernel<false, 1>), grid, block, lds, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    c->opt.last_assign_staged = staged ? 1 : 0;
    return BUSCA_OK;
}

static_assert(ASSIGN_STAGES_MAX == BUSCA_ASSIGN_STAGES_MAX, "the kernel's histogram is sized for the header's bound");
static_assert(sizeof(AssignStageRec) == sizeof(busca_assign_stage) && sizeof(AssignStageRec) == 16, "one layout of the stage record");

// bytes of dynamic LDS a launch of n x m asks for: the state and, staged, room for the member rows of a stage - a whole plane if that fits, else
// what is left of the workgroup's 160 KiB.  The one function that sizes the launch.
static size_t assign_stages_lds_bytes(int n, int m, bool staged) {
    const size_t state = assign_stages_state_bytes(n, m);
    return state + (staged ? std::min((size_t)8 * n * m, ((size_t)ASSIGN_LDS_MAX - state) & ~(size_t)7) : 0);
}

extern "C" int64_t busca_assign_stages_lds_bytes(int32_t n, int32_t m, int32_t staged) {
    if (n < 0 || m < 0 || n > BUSCA_ASSIGN_MAX || m > BUSCA_ASSIGN_MAX) return -1;
    return (int64_t)assign_stages_lds_bytes(n, m, staged != 0);
}

extern "C" int busca_assign_stages(busca_ctx* c, const double* cost, int32_t planes, int32_t batch, int32_t n, int32_t m, const int32_t* dims,
                                   const void* stages, int32_t n_stages, const int32_t* first, const int32_t* again,
                                   int32_t* row_to_col, int32_t* col_to_row, int32_t* row_stage, int32_t* status, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (batch < 0 || n < 0 || m < 0 || planes < 0) return fail(c, BUSCA_EINVAL, "busca_assign_stages: negative size");
    if (n_stages < 1 || n_stages > BUSCA_ASSIGN_STAGES_MAX)
        return fail(c, BUSCA_EINVAL, "busca_assign_stages: %d stages, 1 .. %d are supported", n_stages, BUSCA_ASSIGN_STAGES_MAX);
    if (batch == 0 || n == 0 || m == 0) return BUSCA_OK;
    if (!cost || !stages || !first || !row_to_col) return fail(c, BUSCA_EINVAL, "busca_assign_stages: null pointer");
    if (n > BUSCA_ASSIGN_MAX || m > BUSCA_ASSIGN_MAX)
        return fail(c, BUSCA_EINVAL, "busca_assign_stages: %d x %d is beyond the supported %d x %d", n, m, BUSCA_ASSIGN_MAX, BUSCA_ASSIGN_MAX);
    HIP_TRY(c, hipSetDevice(c->device));
    const bool staged = c->opt.assign_stage != 0;
    const size_t lds = assign_stages_lds_bytes(n, m, staged);
    AssignStagesArgs a{cost, (const int*)dims, planes, n, m, (unsigned)((lds - assign_stages_state_bytes(n, m)) >> 3), (const AssignStageRec*)stages, n_stages,
                       (const int*)first, (const int*)again,
                       (int*)row_to_col, (int*)col_to_row, (int*)row_stage, (int*)status};
    const bool wide = m > ASSIGN_ONE_WAVE_COLS;
    const void* kern = staged ? (wide ? (const void*)assign_stages_kernel<true, ASSIGN_WAVES> : (const void*)assign_stages_kernel<true, 1>)
                              : (wide ? (const void*)assign_stages_kernel<false, ASSIGN_WAVES> : (const void*)assign_stages_kernel<false, 1>);
    if (lds > 65536) {
        const int rc = ensure_lds(c, kern, ASSIGN_LDS_MAX);
        if (rc != BUSCA_OK) return rc;
    }
    TimedLaunch tl(c, (hipStream_t)stream);
    const dim3 grid(batch), block(wide ? ASSIGN_WAVES * 64 : 64);
    if (staged && wide) hipLaunchKernelGGL((assign_stages_kernel<true, ASSIGN_WAVES>), grid, block, lds, (hipStream_t)stream, a);
    else if (staged) hipLaunchKernelGGL((assign_stages_kernel<true, 1>), grid, block, lds, (hipStream_t)stream, a);
    else if (wide) hipLaunchKernelGGL((assign_stages_kernel<false, ASSIGN_WAVES>), grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((assign_stages_kernel<false, 1>), grid, block, lds, (hipStream_t)stream, a);
    HIP_TRY(c, hipGetLastError());
    c->opt.last_assign_staged = staged ? 1 : 0;
    return BUSCA_OK;
}
