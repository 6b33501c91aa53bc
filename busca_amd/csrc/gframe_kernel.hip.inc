// The four kernels of a GHOST frame on resident track state (include/busca_gframe.h), around the linear assignment.  The arithmetic is included
// text: ghost_motion_warp_corner, ghost_motion_step_coord and ghost_motion_append_one of ghost_motion_kernel.hip.inc, pairwise_iou and
// pairwise_iou_cost of pairwise_kernel.hip.inc, ghost_combine_entry of ghost_kernel.hip.inc, store_ring_push and store_ring_copy of
// store_kernel.hip.inc - all included by the unit before this file, and the very functions the kernels of libbusca_hip.so and libbusca_store.so call.
//
//  gframe_advance_kernel : one 64-lane workgroup per listed slot: (with a warp) every valid ring row of the slot through the warp, one (row, corner)
//      per lane and round, a barrier, then - for the first n_step slots - the motion step, one coordinate per lane 0 .. 3, which reads the rows
//      the workgroup has just warped.
//  gframe_cost_kernel    : the final [n, m] cost.  A PW_TA x PW_TB (16 x 64) tile per 256-lane workgroup, as pairwise_kernel and frame_cost_kernel:
//      the 16 positions and 64 detection boxes staged once in LDS, every lane the four rows of one column: the appearance entry, the class mask,
//      the blend with 1 - IoU, the threshold.  A lane reads and writes its own entries only, so `out` may be `app`.
//  gframe_keep_kernel    : one thread per row of the range and per column: the strict threshold test of the matched pair, read from both match
//      vectors of the solver - the row's thread writes track_det, the column's thread det_track and, with a mask, the NaN of that column in the
//      rows from mask_from on.  Both threads evaluate the same comparison on the same entry; no atomics.
//  gframe_apply_kernel   : n + m workgroups of 64 lanes (one wave).  Workgroup i < n: Track.add_detection of slot[i] with the detection it was
//      assigned.  Workgroup n + j: Track.__init__ of detection j into a free slot, when j was not assigned and may start a track; its rank among
//      such columns is counted by the workgroup itself over the columns below j.  Lane 0 does the bookkeeping of both rings and broadcasts the
//      feature row by a shuffle; the 64 lanes copy the feature.  Both decisions are uniform over the workgroup.
//
// No multiply-add contraction anywhere in this file (the files included before it leave the file-scope mode at `fast`).
#pragma clang fp contract(off)

struct GFrameAdvance {
    GhostMotionRings r;
    const int* slot;            // [n]
    const float* warp;          // dev [6] or nullptr
    double* out;                // [n_step, 4]
    int n, n_step, num_active, last_n, diff32;
};

__global__ void __launch_bounds__(64) gframe_advance_kernel(GFrameAdvance p) {
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= p.n) return;
    const int s = p.slot[i];
    if (s < 0 || s >= p.r.S) {                                     // uniform over the workgroup: a skipped slot touches no state
        if (i < p.n_step && tid < 4) p.out[(size_t)i * 4 + tid] = __builtin_nan("");
        return;
    }
    if (p.warp != nullptr) {                                       // uniform over the workgroup
        double w[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = (double)p.warp[k];      // as busca_ghost_motion_warp widens its host float32 warp
        for (int q = tid; q < 2 * p.r.H; q += 64) ghost_motion_warp_corner(p.r, s, q >> 1, q & 1, w);
        __syncthreads();                                           // the warped rows are what lanes 0 .. 3 read next
    }
    if (i < p.n_step && tid < 4) p.out[(size_t)i * 4 + tid] = ghost_motion_step_coord(p.r, s, tid, i < p.num_active, p.last_n, p.diff32);
}

struct GFrameCost {
    const double* app;          // [n, m]
    const double* pos;          // [n, 4] or nullptr: no blend
    const double* boxes;        // [m, 4]
    const int* tlabel;          // [n] or nullptr
    const int* dlabel;          // [m] or nullptr
    const double* thr;          // [2] or nullptr
    double* out;                // [n, m]; may be app
    double w_app, w_motion;     // 1 - alpha and alpha, rounded on the host as busca_ghost_combine forms them
    int n, m, num_active;
};

__global__ void __launch_bounds__(256) gframe_cost_kernel(GFrameCost p) {
    __shared__ double sa[PW_TA][4];
    __shared__ double sb[PW_TB][4];
    const int tid = threadIdx.x;
    const int a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    const bool blend = p.pos != nullptr;
    if (blend) {                                                   // uniform over the workgroup; the staging of pairwise_kernel
        if (tid < PW_TA * 4) { const int r = a0 + tid / 4; sa[tid / 4][tid % 4] = r < p.n ? p.pos[(size_t)r * 4 + tid % 4] : 0.0; }
        { const int r = b0 + tid / 4; sb[tid / 4][tid % 4] = r < p.m ? p.boxes[(size_t)r * 4 + tid % 4] : 0.0; }
        __syncthreads();
    }
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= p.m) return;
    const int dl = p.tlabel != nullptr ? p.dlabel[j] : 0;
#pragma unroll
    for (int k = 0; k < PW_TA / 4; ++k) {
        const int ri = rg + 4 * k, i = a0 + ri;
        if (i >= p.n) continue;
        double motion = 0.0;
        if (blend)
            motion = pairwise_iou_cost(pairwise_iou(sa[ri][0], sa[ri][1], sa[ri][2], sa[ri][3], sb[col][0], sb[col][1], sb[col][2], sb[col][3]), nullptr);
        const size_t at = (size_t)i * p.m + j;
        p.out[at] = ghost_combine_entry(p.app[at], p.tlabel != nullptr && p.tlabel[i] != dl, blend, motion, p.w_app, p.w_motion,
                                        p.thr != nullptr ? p.thr + (i < p.num_active ? 0 : 1) : nullptr);
    }
}

struct GFrameKeep {
    double* cost;               // [n, m]
    const int* row_to_col;      // [hi - lo]
    const int* col_to_row;      // [m]
    const double* thr;          // [2]
    int* track_det;             // [n]
    int* det_track;             // [m]
    int n, m, lo, hi, num_active, merge, mask_from;
};

// the pair (row r of the range, column j) is one the solver matched and its cost is strictly below the row's threshold; NaN on either side: no
__device__ __forceinline__ bool gframe_kept(const GFrameKeep& p, int r, int j) {
    if (r < 0 || r >= p.hi - p.lo || j < 0 || j >= p.m) return false;
    if (p.row_to_col[r] != j || p.col_to_row[j] != r) return false;        // the two vectors name each other: a column is kept by one row at most
    const int i = p.lo + r;
    return p.cost[(size_t)i * p.m + j] < p.thr[i < p.num_active ? 0 : 1];
}

__global__ void __launch_bounds__(256) gframe_keep_kernel(GFrameKeep p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < p.hi - p.lo) {
        const int r = (int)t, j = p.row_to_col[r];
        p.track_det[p.lo + r] = gframe_kept(p, r, j) ? j : -1;
    }
    if (t < p.m) {
        const int j = (int)t, r = p.col_to_row[j];
        if (gframe_kept(p, r, j)) {
            p.det_track[j] = p.lo + r;
            if (p.mask_from >= 0)                                   // mask_from >= hi: no thread reads what this loop writes
                for (int i = p.mask_from; i < p.n; ++i) p.cost[(size_t)i * p.m + j] = __builtin_nan("");
        } else if (!p.merge) {
            p.det_track[j] = -1;
        }
    }
}

struct GFrameApply {
    GhostMotionRings r;                                            // S is the slot count of both states
    float* gallery; int* g_count; int* g_newest; unsigned char* mv_seen;
    const int* slot;            // [n]
    const int* track_det;       // [n]
    const int* det_track;       // [m]
    const float* det_feat;      // [m, E]
    const double* det_boxes;    // [m, 4]
    const unsigned char* may_start;     // [m]
    const int* free_slot;       // [n_free]
    int* det_slot;              // [m]
    int n, m, budget, E, frame, n_free;
};

// Track.add_detection (fresh false) or Track.__init__ (fresh true) of the valid slot s with detection j.  All 64 lanes of the workgroup call it.
__device__ __forceinline__ void gframe_write_track(const GFrameApply& f, int s, int j, bool fresh, int tid) {
    int row = 0;
    if (tid == 0) {
        row = store_ring_push(f.g_count, f.g_newest, f.mv_seen, f.budget, s, fresh);
        ghost_motion_append_one(f.r, s, f.det_boxes + (size_t)j * 4, f.frame, fresh);
    }
    row = __shfl(row, 0, 64);                                      // the workgroup is one wave
    store_ring_copy(f.gallery, f.det_feat, f.budget, f.E, s, row, j, tid, 64);
}

__global__ void __launch_bounds__(64) gframe_apply_kernel(GFrameApply f) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < f.n) {                                                 // a row: the track's own detection
        const int s = f.slot[b], j = f.track_det[b];
        if (s < 0 || s >= f.r.S || j < 0 || j >= f.m) return;      // uniform over the workgroup
        gframe_write_track(f, s, j, false, tid);
        return;
    }
    const int j = b - f.n;
    if (j >= f.m) return;
    const int i = f.det_track[j];
    if (i >= 0) {                                                  // assigned: the slot as listed, also when it was skipped
        if (tid == 0) f.det_slot[j] = i < f.n ? f.slot[i] : -1;
        return;
    }
    if (f.may_start[j] == 0) {
        if (tid == 0) f.det_slot[j] = -1;
        return;
    }
    int rank = 0;
    for (int c = tid; c < j; c += 64) rank += (f.det_track[c] < 0 && f.may_start[c] != 0) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rank += __shfl_xor(rank, off, 64);      // every lane holds the sum
    if (rank >= f.n_free) {                                        // the store is full
        if (tid == 0) f.det_slot[j] = -2;
        return;
    }
    const int s = f.free_slot[rank];
    if (tid == 0) f.det_slot[j] = s;
    if (s < 0 || s >= f.r.S) return;
    gframe_write_track(f, s, j, true, tid);
}

#pragma clang fp contract(fast)
