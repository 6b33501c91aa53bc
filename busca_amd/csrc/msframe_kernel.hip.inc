// The three kernels of the StrongSORT frames of many sequences on one store (include/busca_msframe.h), around the staged assignment over the batch.
// The arithmetic is sframe_advance_track, sframe_stage_row / sframe_stage_dets / sframe_entry, sframe_apply_row and sframe_apply_col of
// sframe_kernel.hip.inc - the bodies libbusca_sframe.so runs - and appear_tile, appear_diag and appear_dist of appear_kernel.hip.inc - the bodies
// busca_appearance_cost runs -, all included by the unit before this file.  Only the addressing is new here: a table of problems over one slot list,
// one detection table, one list of free slots and a list of camera matrices, and padded [batch, 2, N, M] / [batch, N] / [batch, M] blocks for the
// solver between the calls.
//
//  msframe_advance_kernel : grid (N, batch), 64 lanes.  Workgroup (x, k) with x < n_k is row x of problem k: where the problem has a matrix,
//      Track.camera_update with it, and then Track.predict.
//  msframe_cost_kernel    : grid (ceil(M / PW_TB), ceil(N / PW_TA), batch), 256 lanes.  Workgroup (x, y, k) serves tile (y, x) of problem k, if that tile
//      lies inside (n_k, m_k).  The appearance entries of the tile come first, as the plain flavour of appear_kernel forms them: wave w owns the
//      detections 16 w .. 16 w + 15 of the tile, lane (a, b) loads the feature row of tile row a (gathered through the slot list) and of detection
//      16 w + a, and after the matrix instructions holds the entries (row b + 4 r, column 16 w + a), r = 0 .. 3.  The same lane then forms both planes
//      of those four entries from the staged tile - sframe_entry is a function of one entry, so the lane mapping changes no bit.  A tile none of
//      whose rows is gated (0 <= first < depth and a live slot) skips the matrix instructions: every lane of a wave sees all 16 rows, so the ballot
//      of one wave is the workgroup's, and the branch is taken before the barrier.
//  msframe_apply_kernel   : grid (N + M, batch), 64 lanes.  Workgroup (x, k) with x < n_k is row x of problem k, workgroup (N + j, k) with j < m_k its
//      column j, ranked among the starting columns of its own problem; every other workgroup exits at once.
// A row the table should not hold (msframe_problem) skips its problem in all three kernels.  Every exit is taken by the whole workgroup, before a
// barrier.  No multiply-add contraction anywhere in this file.
#pragma clang fp contract(off)

static_assert(PW_TA == 16 && PW_TB == APPEAR_TILE_M, "the tile of sframe_cost_kernel is the workgroup of the plain appear_kernel: 16 tracks x 64 detections");

struct MSFrame {
    const int* slot;            // [n_total]
    const int* free_slot;       // [f_total]
    const int* problems;        // [batch,7]: row_begin, n_k, det_begin, m_k, free_begin, n_free_k, matrix_k
    const double* matrices;     // [n_matrices,9]
    int S, n_total, m_total, f_total, n_matrices, N, M;
};

struct MSFrameProblem {
    int row_begin, n, det_begin, m, free_begin, n_free, matrix;
};

// row k of the table -> false for a row that skips its problem (uniform over the workgroup: the table row is the block's)
__device__ __forceinline__ bool msframe_problem(const MSFrame& b, int k, MSFrameProblem& p) {
    const int* q = b.problems + (size_t)k * 7;
    p.row_begin = q[0], p.n = q[1], p.det_begin = q[2], p.m = q[3], p.free_begin = q[4], p.n_free = q[5], p.matrix = q[6];
    return !(p.row_begin < 0 || p.n < 0 || p.det_begin < 0 || p.m < 0 || p.free_begin < 0 || p.n_free < 0 || p.n > b.N || p.m > b.M ||
             (long long)p.row_begin + p.n > b.n_total || (long long)p.det_begin + p.m > b.m_total || (long long)p.free_begin + p.n_free > b.f_total ||
             p.matrix < -1 || p.matrix >= b.n_matrices);
}

__global__ void __launch_bounds__(64) msframe_advance_kernel(MSFrame b, double* __restrict__ mean, double* __restrict__ cov) {
    MSFrameProblem p;
    if (!msframe_problem(b, blockIdx.y, p)) return;
    const int x = blockIdx.x;
    if (x >= p.n) return;                                          // padding
    const KStore k{mean, cov, b.slot + p.row_begin, b.S, p.n};
    int s;
    if (!kstore_live(k, x, s)) return;                             // uniform over the workgroup
    sframe_advance_track(mean + (size_t)s * 8, cov + (size_t)s * 64, p.matrix >= 0 ? b.matrices + (size_t)p.matrix * 9 : nullptr, threadIdx.x);
}

// `a` holds the whole batch: first / again / stale [n_total], the detection tables [m_total], out [batch,2,N,M], status [batch,N]; m, cost and ld_cost
// are unused
__global__ void __launch_bounds__(256) msframe_cost_kernel(MSFrame b, const double* __restrict__ mean, const double* __restrict__ cov, SFrameCost a,
                                                           const float* __restrict__ feat, const float* __restrict__ det_feat, int E) {
    __shared__ SFrameTile T;
    MSFrameProblem p;
    if (!msframe_problem(b, blockIdx.z, p)) return;
    const int a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (a0 >= p.n || b0 >= p.m) return;                            // padding of the slab (uniform too)
    const KStore k{(double*)mean, (double*)cov, b.slot + p.row_begin, b.S, p.n};
    SFrameCost g = a;
    g.det_xyah = a.det_xyah + (size_t)p.det_begin * 4, g.det_tlwh = a.det_tlwh + (size_t)p.det_begin * 4;
    g.stale = a.stale != nullptr ? a.stale + p.row_begin : nullptr;
    g.first = a.first + p.row_begin, g.again = a.again != nullptr ? a.again + p.row_begin : nullptr;
    g.status = a.status != nullptr ? a.status + (size_t)blockIdx.z * b.N : nullptr;
    g.m = p.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, la = lane & 15, lb = lane >> 4;
    const int col = wave * 16 + la, j = b0 + col;                  // this lane's detection: its B row and the column of its four entries
    // the appearance entries (row lb + 4 r, column col): the plain flavour of appear_kernel on 16 gathered tracks
    double capp[4] = {0.0, 0.0, 0.0, 0.0};
    {
        const int t = a0 + la;                                     // this lane's A row
        const float* arow = nullptr;                               // a row past n_k, a skipped slot, a row no cascade stage reads: masked
        if (t < p.n) {
            const int f = g.first[t];
            int s;
            if (f >= 0 && f < g.depth && kstore_live(k, t, s)) arow = feat + (size_t)s * E;
        }
        if (__ballot(arow != nullptr) != 0) {                      // the same 16 rows in every wave: uniform over the workgroup
            const float* brow = j < p.m ? det_feat + ((size_t)p.det_begin + j) * E : nullptr;
            ap_f64x4 dot, ga, gb;
            appear_tile<true>(arow, brow, E, lb, dot, ga, gb);
            const double da = appear_diag(ga, la), db = appear_diag(gb, la);
            const double nb = __shfl(db, la + 16 * (la & 3));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lb + 4 * r;
                const double na = __shfl(da, row + 16 * lb);       // row & 3 == lb
                capp[r] = appear_dist(dot[r], na, nb, 0);
            }
        }
    }
    if (tid < PW_TA) sframe_stage_row(T, k, g, tid, a0 + tid, b0 == 0);
    sframe_stage_dets(T, g, b0, tid);
    __syncthreads();
    if (j >= p.m) return;
    const size_t plane = (size_t)b.N * (size_t)b.M;
    double* out = a.out + (size_t)blockIdx.z * 2 * plane;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ri = lb + 4 * r, i = a0 + ri;
        if (i >= p.n) continue;
        double v0, v1;
        sframe_entry(T, g, ri, col, &capp[r], v0, v1);
        const size_t at = (size_t)i * b.M + j;
        out[at] = v0;
        out[plane + at] = v1;
    }
}

// `f` holds the whole batch: row_to_col / status [batch,N], col_to_row / new_slot [batch,M], the detection tables [m_total]; free_slot, m and n_free
// are unused
__global__ void __launch_bounds__(64) msframe_apply_kernel(MSFrame b, double* __restrict__ mean, double* __restrict__ cov, SFrameApply f) {
    MSFrameProblem p;
    if (!msframe_problem(b, blockIdx.y, p)) return;
    const int x = blockIdx.x, tid = threadIdx.x;
    const bool row = x < b.N;
    if (row ? x >= p.n : x - b.N >= p.m) return;                   // padding
    const size_t at_n = (size_t)blockIdx.y * b.N, at_m = (size_t)blockIdx.y * b.M;
    const KStore k{mean, cov, b.slot + p.row_begin, b.S, p.n};
    SFrameApply g = f;
    g.row_to_col = f.row_to_col + at_n, g.col_to_row = f.col_to_row + at_m;
    g.det_xyah = f.det_xyah + (size_t)p.det_begin * 4, g.det_conf = f.det_conf != nullptr ? f.det_conf + p.det_begin : nullptr;
    g.det_feat = f.det_feat + (size_t)p.det_begin * f.E;
    g.free_slot = b.free_slot + p.free_begin, g.new_slot = f.new_slot + at_m, g.status = f.status != nullptr ? f.status + at_n : nullptr;
    g.m = p.m, g.n_free = p.n_free;
    if (row) sframe_apply_row(k, g, x, tid);
    else sframe_apply_col(k, g, x - b.N, tid);
}
