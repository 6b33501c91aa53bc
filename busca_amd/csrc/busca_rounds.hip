// libbusca_rounds.so: the association rounds of many sequences in one launch and its C-ABI (include/busca_rounds.h).  A library of its own, without
// a busca_ctx, as libbusca_track.so is: the interfaces of the other libraries stay what they are.  The device code is the tile body of
// busca_track_round_cost (kstore_round_cost_tile of kalman_store_kernel.hip.inc) - the very text libbusca_track.so compiles - behind a kernel that
// reads a table of problems.  The other kernels the three included files define come along unused (hidden): including the files whole keeps one text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/busca_hip.h"        // the BUSCA_PAIR_* codes pairwise_kernel.hip.inc switches on; no busca_* function is called or defined here

#pragma GCC visibility push(default)
#include "../../include/busca_rounds.h"
#pragma GCC visibility pop

#ifdef __FAST_MATH__
#error "the Kalman kernels need IEEE float64 division and square root: build without -ffast-math"
#endif

#include "pairwise_kernel.hip.inc"
#include "track_kernel.hip.inc"
#include "kalman_store_kernel.hip.inc"
#include "rounds_kernel.hip.inc"

static_assert(KSTORE_FUSE_MOTION == BUSCA_ROUNDS_FUSE_MOTION && KSTORE_ONLY_POSITION == BUSCA_ROUNDS_ONLY_POSITION && KSTORE_GATE_ONLY == BUSCA_ROUNDS_GATE_ONLY,
              "kalman_store_kernel.hip.inc and busca_rounds.h disagree on the flags");

#define CAPI_EHIP BUSCA_ROUNDS_EHIP
#include "capi_prelude.hpp"

extern "C" int busca_rounds_version(void) { return 1000; }

extern "C" const char* busca_rounds_last_error(void) { return g_err; }

extern "C" int busca_rounds_cost(const double* mean, const double* cov, int32_t S, const int32_t* slot, int32_t n_total, const double* det_tlbr,
                                 const double* det_xyah, const double* det_score, int32_t m_total, const int32_t* problems, int32_t batch, int32_t N,
                                 int32_t M, int32_t flags, double lambda, double* out, int32_t* status, int32_t device, void* stream) {
    static const char* who = "busca_rounds_cost";
    const int known = BUSCA_ROUNDS_FUSE_MOTION | BUSCA_ROUNDS_ONLY_POSITION | BUSCA_ROUNDS_GATE_ONLY;
    if (S < 0 || n_total < 0 || m_total < 0) return refuse(BUSCA_ROUNDS_EINVAL, "%s: negative size (S %d, n_total %d, m_total %d)", who, S, n_total, m_total);
    if (batch < 0 || N < 0 || M < 0) return refuse(BUSCA_ROUNDS_EINVAL, "%s: negative size (batch %d, N %d, M %d)", who, batch, N, M);
    if (device < 0) return refuse(BUSCA_ROUNDS_EINVAL, "%s: negative device %d", who, device);
    if (flags & ~known) return refuse(BUSCA_ROUNDS_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~known));
    if ((flags & BUSCA_ROUNDS_FUSE_MOTION) && (flags & BUSCA_ROUNDS_GATE_ONLY))
        return refuse(BUSCA_ROUNDS_EINVAL, "%s: FUSE_MOTION and GATE_ONLY exclude each other", who);
    if (lambda != lambda) return refuse(BUSCA_ROUNDS_EINVAL, "%s: lambda is NaN", who);
    if (batch > 65535) return refuse(BUSCA_ROUNDS_EINVAL, "%s: %d problems are more than a grid holds (65535 at most)", who, batch);
    const long long row_tiles = ((long long)N + PW_TA - 1) / PW_TA, col_tiles = ((long long)M + PW_TB - 1) / PW_TB;
    if (row_tiles > 65535) return refuse(BUSCA_ROUNDS_EINVAL, "%s: N = %d tracks need more workgroups than a grid holds (%d at most)", who, N, 65535 * PW_TA);
    if (batch == 0 || N == 0 || M == 0 || n_total == 0 || m_total == 0) return 0;      // with an empty list every problem is empty or skipped
    const bool motion = (flags & (BUSCA_ROUNDS_FUSE_MOTION | BUSCA_ROUNDS_GATE_ONLY)) != 0;
    if (!mean || (motion && !cov) || !slot) return refuse(BUSCA_ROUNDS_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (!problems) return refuse(BUSCA_ROUNDS_EINVAL, "%s: null pointer (problems)", who);
    if (!det_tlbr || !out) return refuse(BUSCA_ROUNDS_EINVAL, "%s: null pointer (det_tlbr and out are required)", who);
    if (motion && !det_xyah) return refuse(BUSCA_ROUNDS_EINVAL, "%s: det_xyah is NULL with a motion flag (0x%x)", who, (unsigned)flags);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(det_tlbr, 8) || misaligned(det_xyah, 8) || misaligned(det_score, 8) || misaligned(out, 8) ||
        misaligned(slot, 4) || misaligned(problems, 4) || misaligned(status, 4))
        return refuse(BUSCA_ROUNDS_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    RoundsCost r;
    r.mean = mean, r.cov = cov, r.slot = (const int*)slot;
    r.det_tlbr = det_tlbr, r.det_xyah = motion ? det_xyah : nullptr, r.det_score = det_score;
    r.problems = (const int*)problems, r.out = out, r.status = (int*)status, r.lambda = lambda;
    r.S = S, r.n_total = n_total, r.m_total = m_total, r.N = N, r.M = M, r.flags = flags;
    CAPI_LAUNCH(who, device, rounds_cost_kernel, dim3((unsigned)col_tiles, (unsigned)row_tiles, (unsigned)batch), dim3(256), stream, r);
    return 0;
}
