// The two kernels of a ByteTrack frame on resident Kalman state (include/busca_frame.h; float64, no contraction), on either side of the staged
// assignment.  The arithmetic is the per-track bodies of track_kernel.hip.inc and the pair functions of pairwise_kernel.hip.inc, the addressing that
// of kalman_store_kernel.hip.inc (KStore, kstore_live) - all three included by the unit before this file.
//
//  frame_cost_kernel  : the [2, n, m] slab of the frame.  A PW_TA x PW_TB (16 x 64) tile per 256-lane workgroup, as kstore_round_cost_tile without a
//      motion flag: lanes 0 .. 15 stage one track's box each in LDS, all lanes stage the detections, then every lane produces the four rows of one
//      column - the IoU once, plane 0 (fuse_score) where the column's class is 0, plane 1 (plain) where it is 1, +inf everywhere else.
//  frame_apply_kernel : n + m workgroups of 64 lanes.  Workgroup i < n: KalmanFilter.update of slot[i] with the detection the solver matched it to.
//      Workgroup n + j: KalmanFilter.initiate of detection j into a free slot, when j starts a track; its rank among such columns is counted by
//      the workgroup itself over the columns below j (64 lanes strided, one wave reduction), so the slots are the same from run to run.
//      Both decisions are uniform over the workgroup.
// The bodies are device functions - frame_cost_tile, frame_apply_row, frame_apply_col - which mframe_kernel.hip.inc (libbusca_mframe.so) calls once
// per (problem, tile), (problem, row) and (problem, column) of a batch: one text behind two addressings.

// The tile (a0, b0) of a frame's slab: rows a0 .. a0 + PW_TA - 1 of the list k.slot[0 .. k.n), columns b0 .. b0 + PW_TB - 1 of the m detections,
// written to out[p * plane + i * ld + j].  All 256 lanes of the workgroup call it (it holds a barrier).  `status` [k.n] is written by the tiles of
// column block 0 alone.  frame_cost_kernel and mframe_cost_kernel (mframe_kernel.hip.inc, libbusca_mframe.so) are this function behind two addressings.
__device__ __forceinline__ void frame_cost_tile(const KStore& k, const double* __restrict__ det_tlbr, const double* __restrict__ det_score,
                                                const uint8_t* __restrict__ det_class, int m, double* __restrict__ out, size_t ld, size_t plane,
                                                int* __restrict__ status, int a0, int b0) {
#pragma clang fp contract(off)
    __shared__ double sbox[PW_TA][4];
    __shared__ int slive[PW_TA];
    __shared__ double sb[PW_TB][4];
    const int tid = threadIdx.x;
    if (tid < PW_TA) {
        const int t = a0 + tid;
        int s, live = 0;
        if (t < k.n && kstore_live(k, t, s)) {
            double b[4];
            kalman_box_of(k.mean + (size_t)s * 8, 1, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) sbox[tid][i] = b[i];
            live = 1;
        }
        slive[tid] = live;
        if (b0 == 0 && t < k.n && status != nullptr) status[t] = 0;
    }
    {
        const int r = b0 + tid / 4;
        sb[tid / 4][tid % 4] = r < m ? det_tlbr[(size_t)r * 4 + tid % 4] : 0.0;
    }
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= m) return;
    const int cls = det_class[j];
    const double bx1 = sb[col][0], by1 = sb[col][1], bx2 = sb[col][2], by2 = sb[col][3];
#pragma unroll
    for (int q = 0; q < PW_TA / 4; ++q) {
        const int ri = rg + 4 * q, i = a0 + ri;
        if (i >= k.n) continue;
        double v0 = INFINITY, v1 = INFINITY;
        if (slive[ri] && cls <= 1) {
            const double iou = pairwise_iou(sbox[ri][0], sbox[ri][1], sbox[ri][2], sbox[ri][3], bx1, by1, bx2, by2);
            if (cls == 0) v0 = pairwise_iou_cost(iou, det_score != nullptr ? det_score + j : nullptr);
            else v1 = pairwise_iou_cost(iou, nullptr);
        }
        const size_t at = (size_t)i * ld + j;
        out[at] = v0;
        out[plane + at] = v1;
    }
}

__global__ void __launch_bounds__(256) frame_cost_kernel(KStore k, const double* __restrict__ det_tlbr, const double* __restrict__ det_score,
                                                         const uint8_t* __restrict__ det_class, int m, double* __restrict__ out,
                                                         int* __restrict__ status) {
    frame_cost_tile(k, det_tlbr, det_score, det_class, m, out, (size_t)m, (size_t)k.n * (size_t)m, status, blockIdx.y * PW_TA, blockIdx.x * PW_TB);
}

struct FrameApply {
    const int* row_to_col;      // [n]
    const int* col_to_row;      // [m]
    const double* det_xyah;     // [m,4]
    const double* det_score;    // [m] or nullptr
    const uint8_t* det_class;   // [m]
    const int* free_slot;       // [n_free]
    int* new_slot;              // [m]
    int* status;                // [n] or nullptr
    double det_thresh;
    int m, n_free;
};

// does column j start a track?  (byte_tracker.py:420-423: an unmatched first-round detection, unless its score is below det_thresh)
__device__ __forceinline__ bool frame_starts_track(const FrameApply& f, int j) {
    return f.col_to_row[j] < 0 && f.det_class[j] == 0 && !(f.det_score != nullptr && f.det_score[j] < f.det_thresh);
}

// Row b of the frame (0 <= b < k.n): the update of its match.  All 64 lanes of the workgroup call it; the decision is uniform over them.
__device__ __forceinline__ void frame_apply_row(const KStore& k, const FrameApply& f, int b, int tid) {
    int s;
    const int j = f.row_to_col[b];
    if (!kstore_live(k, b, s) || j < 0 || j >= f.m) {
        if (tid == 0 && f.status != nullptr) f.status[b] = 0;
        return;
    }
    kalman_update_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, f.det_xyah + (size_t)j * 4, f.status != nullptr ? f.status + b : nullptr, tid);
}

// Column j of the frame (0 <= j < f.m): the initiation of a new track, by all 64 lanes of the workgroup.
__device__ __forceinline__ void frame_apply_col(const KStore& k, const FrameApply& f, int j, int tid) {
    if (!frame_starts_track(f, j)) {
        if (tid == 0) f.new_slot[j] = -1;
        return;
    }
    int rank = 0;
    for (int c = tid; c < j; c += 64) rank += frame_starts_track(f, c) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rank += __shfl_xor(rank, off, 64);      // the workgroup is one wave: every lane holds the sum
    if (rank >= f.n_free) {                                        // the store is full
        if (tid == 0) f.new_slot[j] = -2;
        return;
    }
    const int s = f.free_slot[rank];
    if (tid == 0) f.new_slot[j] = s;
    if (s < 0 || s >= k.S) return;
    kalman_initiate_track(f.det_xyah + (size_t)j * 4, k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, tid);
}

__global__ void __launch_bounds__(64) frame_apply_kernel(KStore k, FrameApply f) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < k.n) {                                                 // a row: the update of its match
        frame_apply_row(k, f, b, tid);
        return;
    }
    const int j = b - k.n;                                         // a column: the initiation of a new track
    if (j >= f.m) return;
    frame_apply_col(k, f, j, tid);
}
