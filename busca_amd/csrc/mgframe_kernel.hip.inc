// The six kernels of the GHOST frames of many sequences on one store (include/busca_mgframe.h), around the batched linear assignment.  The arithmetic
// is gframe_advance_slot, gframe_cost_tile, gframe_keep_thread, gframe_apply_row and gframe_apply_col of gframe_body.hip.inc - the bodies
// libbusca_gframe.so runs - and ghost_distance_entry and ghost_thresholds_groups of ghost_body.hip.inc - the bodies busca_ghost_distance and
// busca_ghost_thresholds run -, all included by the unit before this file.  Only the addressing is new here: a table of problems over one slot list
// ordered group-wise (all problems' active rows, then all inactive rows, then all idle rows), one detection table, one list of free slots and a list
// of warps, and padded [batch, R, M] / [batch, R] / [batch, M] blocks for the solver between the calls.
//
//  mgframe_advance_kernel    : grid (L, batch), 64 lanes.  Workgroup (x, k) is listed row x of problem k - its active rows, then its inactive, then its
//      idle ones: the warp of the problem (if it has one), a barrier, the step (if the problem is stepped).
//  mgframe_distance_kernel<MEDIAN> : grid (ceil(M / 64), R, batch), 256 lanes.  Workgroup (x, r, k) is slab row r of problem k against its detection
//      tile x, if the row is one of the groups this call serves.
//  mgframe_thresholds_kernel : grid (batch), 256 lanes: the two groups of rows of problem k, entry by entry in the order of its own [rows, m_k] block.
//  mgframe_cost_kernel       : grid (ceil(M / PW_TB), ceil(R / PW_TA), batch), 256 lanes: tile (y, x) of slab k, in place.
//  mgframe_keep_kernel       : grid (ceil(max(R, M) / 256), batch), 256 lanes: thread t is row t of the stage's range and column t of problem k.
//  mgframe_apply_kernel      : grid (R + M, batch), 64 lanes: workgroup (x, k) with x < R is slab row x of problem k, workgroup (R + j, k) its column j.
// A row the table should not hold (mgframe_problem) skips its problem in all six kernels; every exit is taken by the whole workgroup, before any
// barrier.  No multiply-add contraction anywhere in this file.
#pragma clang fp contract(off)

static_assert(PW_TB == APPEAR_TILE_M, "one width of detection tile for the distance and the cost kernels");

#define MGFRAME_WORDS 13
#define MGFRAME_DIFF32 1
#define MGFRAME_STEP 2

struct MGFrame {
    const int* slot;            // [n_total]
    const int* free_slot;       // [f_total]
    const int* problems;        // [batch, MGFRAME_WORDS]
    const float* warps;         // [n_warps, 6]
    int S, n_total, m_total, f_total, n_warps, N, M, L, R, inact_row;
};

struct MGFrameProblem {
    int act_begin, na, inact_begin, ni, idle_begin, n_idle, det_begin, m, free_begin, n_free, warp, frame, flags;
    GFrameRows rows;            // slab row -> list row
};

// row k of the table -> false for a row that skips its problem (uniform over the workgroup: the table row is the block's)
__device__ __forceinline__ bool mgframe_problem(const MGFrame& b, int k, MGFrameProblem& p) {
    const int* q = b.problems + (size_t)k * MGFRAME_WORDS;
    p.act_begin = q[0], p.na = q[1], p.inact_begin = q[2], p.ni = q[3], p.idle_begin = q[4], p.n_idle = q[5], p.det_begin = q[6], p.m = q[7];
    p.free_begin = q[8], p.n_free = q[9], p.warp = q[10], p.frame = q[11], p.flags = q[12];
    if (p.act_begin < 0 || p.na < 0 || p.inact_begin < 0 || p.ni < 0 || p.idle_begin < 0 || p.n_idle < 0 || p.det_begin < 0 || p.m < 0 ||
        p.free_begin < 0 || p.n_free < 0)
        return false;
    if ((long long)p.act_begin + p.na > b.n_total || (long long)p.inact_begin + p.ni > b.n_total || (long long)p.idle_begin + p.n_idle > b.n_total ||
        (long long)p.det_begin + p.m > b.m_total || (long long)p.free_begin + p.n_free > b.f_total)
        return false;
    if ((long long)p.na + p.ni > b.N || p.m > b.M || (long long)p.na + p.ni + p.n_idle > b.L) return false;
    if (p.warp < -1 || p.warp >= b.n_warps) return false;
    const int at = b.inact_row < 0 ? p.na : b.inact_row;           // where the inactive rows start in the slab
    if (p.na > at || (long long)at + p.ni > b.R) return false;
    p.rows = GFrameRows{p.na, p.ni, p.act_begin, p.inact_begin, at};
    return true;
}

__global__ void __launch_bounds__(64) mgframe_advance_kernel(MGFrame b, GhostMotionRings r, int last_n, double* __restrict__ pos_out) {
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.y, p)) return;
    const int x = blockIdx.x;
    if (x >= p.na + p.ni + p.n_idle) return;                       // padding
    const int lr = x < p.na ? p.act_begin + x : x < p.na + p.ni ? p.inact_begin + (x - p.na) : p.idle_begin + (x - p.na - p.ni);
    const float* warp = p.warp >= 0 ? b.warps + (size_t)p.warp * 6 : nullptr;
    const bool step = (p.flags & MGFRAME_STEP) != 0;
    if (warp == nullptr && !step) return;
    gframe_advance_slot(r, b.slot[lr], warp, step, x < p.na, last_n, (p.flags & MGFRAME_DIFF32) != 0, pos_out + (size_t)lr * 4, threadIdx.x);
}

struct MGFrameDist {
    const float* gallery;       // [rows, budget, E]
    const int* count;           // [rows] or nullptr: every row holds `budget` samples
    const float* dets;          // [m_total, E]
    double* out;                // [batch, R, M]
    int rows, by_list, budget, E, reduce, groups;                  // by_list: a track's rows of `gallery` are found by its list row, not by its slot
};

template <bool MEDIAN>
__global__ void __launch_bounds__(64 * APPEAR_WAVES) mgframe_distance_kernel(MGFrame b, MGFrameDist d) {
    extern __shared__ double mgframe_lds[];         // MEDIAN: [budget][64] staged distances, then [2][64] the selected pair
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.z, p)) return;
    const int r = blockIdx.y, b0 = blockIdx.x * APPEAR_TILE_M;
    const int lr = gframe_list_row(p.rows, r);
    if (lr < 0 || b0 >= p.m) return;                               // padding of the slab: the whole workgroup leaves, before any barrier
    if (!(d.groups & (r < p.na ? 1 : 2))) return;                  // a group another call serves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, lb = lane >> 4;
    const int col = wave * 16 + a, j = b0 + col;
    const float* brow = j < p.m ? d.dets + ((size_t)p.det_begin + j) * d.E : nullptr;
    const int s = d.by_list ? lr : b.slot[lr];
    const bool live = s >= 0 && s < d.rows;
    int cnt = !live ? 0 : (d.count ? d.count[s] : d.budget);
    cnt = cnt < 0 ? 0 : cnt > d.budget ? d.budget : cnt;
    const float* base = d.gallery + (size_t)(live ? s : 0) * d.budget * d.E;
    const double res = ghost_distance_entry<MEDIAN>(base, cnt, d.budget, brow, d.E, d.reduce, mgframe_lds, col, a, lb);
    if (lb == 0 && j < p.m) d.out[((size_t)blockIdx.z * b.R + r) * b.M + j] = res;
}

__global__ void __launch_bounds__(GHOST_THR_THREADS) mgframe_thresholds_kernel(MGFrame b, const double* __restrict__ cost, double k_act, double k_inact,
                                                                               int which, double* __restrict__ thr) {
    __shared__ double part[GHOST_THR_THREADS / 64];
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.x, p)) return;
    if (p.m == 0) return;
    const double* slab = cost + (size_t)blockIdx.x * b.R * b.M;
    ghost_thresholds_groups<true>(slab, (long long)p.na * p.m, slab + (size_t)p.rows.inact_row * b.M, (long long)p.ni * p.m, p.m, b.M, k_act, k_inact,
                                  which, thr + (size_t)blockIdx.x * 2, part);
}

// `a` holds the whole batch: app / out [batch, R, M], pos / tlabel [n_total], boxes / dlabel [m_total], thr [batch, 2]; rows, m and ld are the problem's
__global__ void __launch_bounds__(256) mgframe_cost_kernel(MGFrame b, GFrameCost a) {
    __shared__ double sa[PW_TA][4];
    __shared__ double sb[PW_TB][4];
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.z, p)) return;
    const int a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (b0 >= p.m || a0 >= p.rows.inact_row + p.ni) return;        // padding of the slab (uniform too)
    const size_t at = (size_t)blockIdx.z * b.R * b.M;
    GFrameCost g = a;
    g.app = a.app + at, g.out = a.out + at;
    g.boxes = a.boxes != nullptr ? a.boxes + (size_t)p.det_begin * 4 : nullptr;
    g.dlabel = a.dlabel != nullptr ? a.dlabel + p.det_begin : nullptr;
    g.thr = a.thr != nullptr ? a.thr + (size_t)blockIdx.z * 2 : nullptr;
    g.rows = p.rows, g.m = p.m, g.ld = b.M;
    gframe_cost_tile(g, a0, b0, sa, sb, threadIdx.x);
}

// `a` holds the whole batch: cost [batch, R, M], row_to_col / track_det [batch, R], col_to_row / det_track [batch, M], thr [batch, 2].
// stage 0: all rows of the problem, contiguous; 1: its active rows; 2: its inactive rows, from where they start in the slab.  `mask`: the kept
// columns are withdrawn from the problem's inactive rows.
__global__ void __launch_bounds__(256) mgframe_keep_kernel(MGFrame b, GFrameKeep a, int stage, int mask) {
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.y, p)) return;
    if (p.m == 0) return;
    GFrameKeep g = a;
    g.cost = a.cost + (size_t)blockIdx.y * b.R * b.M;
    g.track_det = a.track_det + (size_t)blockIdx.y * b.R, g.det_track = a.det_track + (size_t)blockIdx.y * b.M;
    g.row_to_col = a.row_to_col + (size_t)blockIdx.y * b.R, g.col_to_row = a.col_to_row + (size_t)blockIdx.y * b.M;
    g.thr = a.thr + (size_t)blockIdx.y * 2;
    g.m = p.m, g.ld = b.M, g.num_active = p.na;
    g.lo = stage == 2 ? p.rows.inact_row : 0;
    g.hi = stage == 1 ? p.na : p.rows.inact_row + p.ni;
    g.mask_from = mask ? p.rows.inact_row : -1, g.mask_to = p.rows.inact_row + p.ni;
    gframe_keep_thread(g, (long long)blockIdx.x * 256 + threadIdx.x);
}

// `f` holds the whole batch: track_det [batch, R], det_track / det_slot [batch, M], the detection tables [m_total]
__global__ void __launch_bounds__(64) mgframe_apply_kernel(MGFrame b, GFrameApply f) {
    MGFrameProblem p;
    if (!mgframe_problem(b, blockIdx.y, p)) return;
    const int x = blockIdx.x, tid = threadIdx.x;
    if (p.m == 0) return;                                          // without detections nothing is assigned
    const bool row = x < b.R;
    if (!row && x - b.R >= p.m) return;                            // padding
    GFrameApply g = f;
    g.track_det = f.track_det + (size_t)blockIdx.y * b.R;
    g.det_track = f.det_track + (size_t)blockIdx.y * b.M, g.det_slot = f.det_slot + (size_t)blockIdx.y * b.M;
    g.det_feat = f.det_feat + (size_t)p.det_begin * f.E, g.det_boxes = f.det_boxes + (size_t)p.det_begin * 4;
    g.may_start = f.may_start + p.det_begin;
    g.free_slot = b.free_slot + p.free_begin;
    g.rows = p.rows, g.m = p.m, g.frame = p.frame, g.n_free = p.n_free;
    if (row) gframe_apply_row(g, x, tid);
    else gframe_apply_col(g, x - b.R, tid);
}

#pragma clang fp contract(fast)
