// The bodies of the four kernels of gframe_kernel.hip.inc as device functions: gframe_kernel.hip.inc includes this file inside its contract(off)
// region and wraps each in its kernel (libbusca_gframe.so); mgframe_kernel.hip.inc (libbusca_mgframe.so) calls the same functions per problem of a
// batch.  What differs between the two is where a row of the cost matrix finds its track: GFrameRows maps a row of the matrix to a row of the slot
// list (and of every table indexed as the slot list is: the stepped positions, the track labels); the single frame's map is the identity.

// Row r of a cost matrix -> the row of the slot list it stands for, or -1 for padding.  The first `na` rows are the active tracks, list rows act0 ..;
// the `ni` inactive tracks, list rows inact0 .., start at matrix row inact_row >= na.
struct GFrameRows {
    int na, ni, act0, inact0, inact_row;
};

__device__ __forceinline__ int gframe_list_row(const GFrameRows& m, int r) {
    if (r < 0) return -1;
    if (r < m.na) return m.act0 + r;
    const int q = r - m.inact_row;
    return q >= 0 && q < m.ni ? m.inact0 + q : -1;
}

// ---- advance: one listed slot by one 64-lane workgroup; every argument is the workgroup's
// (with a warp) every valid ring row of slot s through it, one (row, corner) per lane and round, a barrier, then - with `step` - the motion step, one
// coordinate per lane 0 .. 3, into out_row[4].  A slot outside 0 .. S-1 touches no state and, with `step`, gets a row of NaN.
__device__ __forceinline__ void gframe_advance_slot(const GhostMotionRings& r, int s, const float* warp, bool step, bool active, int last_n, int diff32,
                                                    double* out_row, int tid) {
    if (s < 0 || s >= r.S) {                                       // uniform over the workgroup: a skipped slot touches no state
        if (step && tid < 4) out_row[tid] = __builtin_nan("");
        return;
    }
    if (warp != nullptr) {                                         // uniform over the workgroup
        double w[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = (double)warp[k];        // as busca_ghost_motion_warp widens its host float32 warp
        for (int q = tid; q < 2 * r.H; q += 64) ghost_motion_warp_corner(r, s, q >> 1, q & 1, w);
        __syncthreads();                                           // the warped rows are what lanes 0 .. 3 read next
    }
    if (step && tid < 4) out_row[tid] = ghost_motion_step_coord(r, s, tid, active, last_n, diff32);
}

// ---- cost: one PW_TA x PW_TB tile by one 256-lane workgroup
struct GFrameCost {
    const double* app;          // [n, ld]
    const double* pos;          // [list rows, 4] or nullptr: no blend
    const double* boxes;        // [m, 4]
    const int* tlabel;          // [list rows] or nullptr
    const int* dlabel;          // [m] or nullptr
    const double* thr;          // [2] or nullptr
    double* out;                // [n, ld]; may be app
    double w_app, w_motion;     // 1 - alpha and alpha, rounded on the host as busca_ghost_combine forms them
    GFrameRows rows;            // rows.na: the rows that read thr[0]
    int m, ld;                  // the columns, and the distance between two rows of app / out
};

// the tile at (a0, b0); sa [PW_TA][4] and sb [PW_TB][4] are the workgroup's LDS.  The barrier is passed by every lane.
__device__ __forceinline__ void gframe_cost_tile(const GFrameCost& p, int a0, int b0, double (*sa)[4], double (*sb)[4], int tid) {
    const bool blend = p.pos != nullptr;
    if (blend) {                                                   // uniform over the workgroup; the staging of pairwise_kernel
        if (tid < PW_TA * 4) { const int r = gframe_list_row(p.rows, a0 + tid / 4); sa[tid / 4][tid % 4] = r >= 0 ? p.pos[(size_t)r * 4 + tid % 4] : 0.0; }
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
        const int lr = gframe_list_row(p.rows, i);
        if (lr < 0) continue;
        double motion = 0.0;
        if (blend)
            motion = pairwise_iou_cost(pairwise_iou(sa[ri][0], sa[ri][1], sa[ri][2], sa[ri][3], sb[col][0], sb[col][1], sb[col][2], sb[col][3]), nullptr);
        const size_t at = (size_t)i * p.ld + j;
        p.out[at] = ghost_combine_entry(p.app[at], p.tlabel != nullptr && p.tlabel[lr] != dl, blend, motion, p.w_app, p.w_motion,
                                        p.thr != nullptr ? p.thr + (i < p.rows.na ? 0 : 1) : nullptr);
    }
}

// ---- keep: thread t serves row t of the range and column t
struct GFrameKeep {
    double* cost;               // [., ld]
    const int* row_to_col;      // [hi - lo]
    const int* col_to_row;      // [m]
    const double* thr;          // [2]
    int* track_det;             // indexed by matrix row
    int* det_track;             // [m]
    int m, ld, lo, hi, num_active, merge, mask_from, mask_to;     // the rows mask_from .. mask_to - 1 are masked (mask_from < 0: none)
};

// the pair (row r of the range, column j) is one the solver matched and its cost is strictly below the row's threshold; NaN on either side: no
__device__ __forceinline__ bool gframe_kept(const GFrameKeep& p, int r, int j) {
    if (r < 0 || r >= p.hi - p.lo || j < 0 || j >= p.m) return false;
    if (p.row_to_col[r] != j || p.col_to_row[j] != r) return false;        // the two vectors name each other: a column is kept by one row at most
    const int i = p.lo + r;
    return p.cost[(size_t)i * p.ld + j] < p.thr[i < p.num_active ? 0 : 1];
}

__device__ __forceinline__ void gframe_keep_thread(const GFrameKeep& p, long long t) {
    if (t < p.hi - p.lo) {
        const int r = (int)t, j = p.row_to_col[r];
        p.track_det[p.lo + r] = gframe_kept(p, r, j) ? j : -1;
    }
    if (t < p.m) {
        const int j = (int)t, r = p.col_to_row[j];
        if (gframe_kept(p, r, j)) {
            p.det_track[j] = p.lo + r;
            if (p.mask_from >= 0)                                   // mask_from >= hi: no thread reads what this loop writes
                for (int i = p.mask_from; i < p.mask_to; ++i) p.cost[(size_t)i * p.ld + j] = __builtin_nan("");
        } else if (!p.merge) {
            p.det_track[j] = -1;
        }
    }
}

// ---- apply: one matrix row, or one column, by one 64-lane workgroup (one wave)
struct GFrameApply {
    GhostMotionRings r;                                            // S is the slot count of both states
    float* gallery; int* g_count; int* g_newest; unsigned char* mv_seen;
    const int* slot;            // the slot list
    const int* track_det;       // indexed by matrix row
    const int* det_track;       // [m]: a matrix row
    const float* det_feat;      // [m, E]
    const double* det_boxes;    // [m, 4]
    const unsigned char* may_start;     // [m]
    const int* free_slot;       // [n_free]
    int* det_slot;              // [m]
    GFrameRows rows;
    int m, budget, E, frame, n_free;
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

// matrix row b: the track's own detection
__device__ __forceinline__ void gframe_apply_row(const GFrameApply& f, int b, int tid) {
    const int lr = gframe_list_row(f.rows, b);
    if (lr < 0) return;                                            // padding
    const int s = f.slot[lr], j = f.track_det[b];
    if (s < 0 || s >= f.r.S || j < 0 || j >= f.m) return;          // uniform over the workgroup
    gframe_write_track(f, s, j, false, tid);
}

// column j < m: its slot, and Track.__init__ when it was not assigned and may start a track
__device__ __forceinline__ void gframe_apply_col(const GFrameApply& f, int j, int tid) {
    const int i = f.det_track[j];
    if (i >= 0) {                                                  // assigned: the slot as listed, also when it was skipped
        const int lr = gframe_list_row(f.rows, i);
        if (tid == 0) f.det_slot[j] = lr >= 0 ? f.slot[lr] : -1;
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
