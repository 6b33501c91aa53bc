// The two kernels of the ByteTrack frames of many sequences on one store (include/busca_mframe.h; float64, no contraction), on either side of the
// staged assignment over the batch.  The arithmetic is frame_cost_tile, frame_apply_row and frame_apply_col of frame_kernel.hip.inc, included by the
// unit before this file - the bodies libbusca_frame.so runs; only the addressing is new here: a table of problems over one slot list, one detection
// table and one list of free slots, and padded [batch, 2, N, M] / [batch, N] / [batch, M] blocks for the solver between the two.
//
//  mframe_cost_kernel  : grid (ceil(M / PW_TB), ceil(N / PW_TA), batch), 256 lanes.  Workgroup (x, y, k) reads row k of the table and serves tile
//      (y, x) of problem k, if that tile lies inside (n_k, m_k); what lies outside is not written.
//  mframe_apply_kernel : grid (N + M, batch), 64 lanes.  Workgroup (x, k) with x < n_k is row x of problem k, workgroup (N + j, k) with j < m_k its
//      column j, ranked among the starting columns of its own problem; every other workgroup exits at once.
// A row the table should not hold - a negative entry, a range that leaves the slot list, the detections or the free list, n_k > N, m_k > M - skips
// its problem in both kernels.  Every exit is taken by the whole workgroup, before the tile's barrier.

struct MFrame {
    const int* slot;            // [n_total]
    const int* free_slot;       // [f_total]
    const int* problems;        // [batch,6]: row_begin, n_k, det_begin, m_k, free_begin, n_free_k
    int S, n_total, m_total, f_total, N, M;
};

struct MFrameProblem {
    int row_begin, n, det_begin, m, free_begin, n_free;
};

// row k of the table -> false for a row that skips its problem (uniform over the workgroup: the table row is the block's)
__device__ __forceinline__ bool mframe_problem(const MFrame& b, int k, MFrameProblem& p) {
    const int* q = b.problems + (size_t)k * 6;
    p.row_begin = q[0], p.n = q[1], p.det_begin = q[2], p.m = q[3], p.free_begin = q[4], p.n_free = q[5];
    return !(p.row_begin < 0 || p.n < 0 || p.det_begin < 0 || p.m < 0 || p.free_begin < 0 || p.n_free < 0 || p.n > b.N || p.m > b.M ||
             (long long)p.row_begin + p.n > b.n_total || (long long)p.det_begin + p.m > b.m_total || (long long)p.free_begin + p.n_free > b.f_total);
}

__global__ void __launch_bounds__(256) mframe_cost_kernel(MFrame b, const double* __restrict__ mean, const double* __restrict__ det_tlbr,
                                                          const double* __restrict__ det_score, const uint8_t* __restrict__ det_class,
                                                          double* __restrict__ out, int* __restrict__ status) {
    MFrameProblem p;
    if (!mframe_problem(b, blockIdx.z, p)) return;
    const long long a0 = (long long)blockIdx.y * PW_TA, b0 = (long long)blockIdx.x * PW_TB;
    if (a0 >= p.n || b0 >= p.m) return;                            // padding of the slab (uniform too)
    const KStore k{(double*)mean, nullptr, b.slot + p.row_begin, b.S, p.n};     // the covariances are not read: a box is a function of the mean
    const size_t plane = (size_t)b.N * (size_t)b.M;
    frame_cost_tile(k, det_tlbr + (size_t)p.det_begin * 4, det_score != nullptr ? det_score + p.det_begin : nullptr, det_class + p.det_begin, p.m,
                    out + (size_t)blockIdx.z * 2 * plane, (size_t)b.M, plane, status != nullptr ? status + (size_t)blockIdx.z * b.N : nullptr,
                    (int)a0, (int)b0);
}

// `f` holds the whole batch: row_to_col / status [batch,N], col_to_row / new_slot [batch,M], the detection tables [m_total]; m and n_free are unused
__global__ void __launch_bounds__(64) mframe_apply_kernel(MFrame b, double* __restrict__ mean, double* __restrict__ cov, FrameApply f) {
    MFrameProblem p;
    if (!mframe_problem(b, blockIdx.y, p)) return;
    const int x = blockIdx.x, tid = threadIdx.x;
    const bool row = x < b.N;
    if (row ? x >= p.n : x - b.N >= p.m) return;                   // padding
    const size_t at_n = (size_t)blockIdx.y * b.N, at_m = (size_t)blockIdx.y * b.M;
    const KStore k{mean, cov, b.slot + p.row_begin, b.S, p.n};
    FrameApply g;
    g.row_to_col = f.row_to_col + at_n, g.col_to_row = f.col_to_row + at_m;
    g.det_xyah = f.det_xyah + (size_t)p.det_begin * 4, g.det_score = f.det_score != nullptr ? f.det_score + p.det_begin : nullptr;
    g.det_class = f.det_class + p.det_begin;
    g.free_slot = b.free_slot + p.free_begin, g.new_slot = f.new_slot + at_m, g.status = f.status != nullptr ? f.status + at_n : nullptr;
    g.det_thresh = f.det_thresh, g.m = p.m, g.n_free = p.n_free;
    if (row) frame_apply_row(k, g, x, tid);
    else frame_apply_col(k, g, x - b.N, tid);
}
