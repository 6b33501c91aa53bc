// Slot-indexed kernels of ByteTrack's Kalman state (include/busca_track.h; float64, no contraction): the state of all tracks stays in two device
// arrays over S slots, mean [S,8] and cov [S,8,8], and every kernel takes the list of slots it serves.  The arithmetic is the per-track bodies of
// track_kernel.hip.inc and the pair functions of pairwise_kernel.hip.inc, included by the unit before this file - only the addressing is new here.
// An entry of the slot list outside 0 .. S-1 is skipped: nothing of it is read or written.
//
//  kstore_predict_kernel / _update_kernel / _initiate_kernel : one 64-lane workgroup per listed track, as the list-ordered kernels.
//  kstore_boxes_kernel      : one lane per listed track; a skipped entry gives a row of NaN.
//  kstore_round_cost_kernel : the cost matrix of one association round - kalman_boxes, pairwise(IOU_COST), kalman_gating, the gate and the blend of
//      matching.fuse_motion in one pass.  A PW_TA x PW_TB (16 x 64) tile per 256-lane workgroup, as pairwise_kernel: lanes 0 .. 15 stage one track
//      each in LDS (the four box values, the projected mean and the Cholesky factor: 25 doubles), all lanes stage the detections, then every lane
//      produces four outputs of one column.  The factor is computed once per tile, not once per lane as kalman_gating_kernel does.  The tile body is
//      the device function kstore_round_cost_tile, which rounds_kernel.hip.inc (libbusca_rounds.so) calls once per (problem, tile) of a batch.

#define KSTORE_FUSE_MOTION 1        // BUSCA_TRACK_FUSE_MOTION
#define KSTORE_ONLY_POSITION 2      // BUSCA_TRACK_ONLY_POSITION
#define KSTORE_GATE_ONLY 4          // BUSCA_TRACK_GATE_ONLY

struct KStore {
    double* mean;       // [S,8]
    double* cov;        // [S,8,8]
    const int* slot;    // [n]
    int S, n;
};

__device__ __forceinline__ bool kstore_live(const KStore& k, int t, int& s) {
    s = k.slot[t];
    return s >= 0 && s < k.S;
}

// measurement of list entry t: det_index[t] (NULL: t); false when it is outside 0 .. m-1
__device__ __forceinline__ bool kstore_meas(const int* __restrict__ det_index, int t, int m, int& j) {
    j = det_index != nullptr ? det_index[t] : t;
    return j >= 0 && j < m;
}

__global__ void __launch_bounds__(64) kstore_predict_kernel(KStore k, const uint8_t* __restrict__ not_tracked) {
    const int t = blockIdx.x, tid = threadIdx.x;
    int s;
    if (t >= k.n || !kstore_live(k, t, s)) return;                 // uniform over the workgroup
    kalman_predict_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, not_tracked != nullptr && not_tracked[t], tid);
}

__global__ void __launch_bounds__(64) kstore_update_kernel(KStore k, const double* __restrict__ meas, const int* __restrict__ det_index, int m,
                                                           int* __restrict__ status) {
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= k.n) return;
    int s, j;
    if (!kstore_live(k, t, s) || !kstore_meas(det_index, t, m, j)) {
        if (tid == 0 && status != nullptr) status[t] = 0;
        return;
    }
    kalman_update_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, meas + (size_t)j * 4, status != nullptr ? status + t : nullptr, tid);
}

__global__ void __launch_bounds__(64) kstore_initiate_kernel(KStore k, const double* __restrict__ meas, const int* __restrict__ det_index, int m) {
    const int t = blockIdx.x, tid = threadIdx.x;
    int s, j;
    if (t >= k.n || !kstore_live(k, t, s) || !kstore_meas(det_index, t, m, j)) return;
    kalman_initiate_track(meas + (size_t)j * 4, k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, tid);
}

__global__ void __launch_bounds__(256) kstore_boxes_kernel(KStore k, int tlbr, double* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= k.n) return;
    int s;
    double b[4];
    if (kstore_live(k, (int)t, s)) kalman_box_of(k.mean + (size_t)s * 8, tlbr, b);
    else b[0] = b[1] = b[2] = b[3] = __builtin_nan("");
    double* o = out + t * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = b[c];
}

// The tile (a0, b0) of one round's cost matrix: rows a0 .. a0 + PW_TA - 1 of the list k.slot[0 .. k.n), columns b0 .. b0 + PW_TB - 1 of the m
// detections, written to out[i * ld + j].  All 256 lanes of the workgroup call it (it holds a barrier).  `status` [k.n] is written by the tiles of
// column block 0 alone.  kstore_round_cost_kernel and rounds_cost_kernel (rounds_kernel.hip.inc) are this function behind two addressings.
__device__ __forceinline__ void kstore_round_cost_tile(const KStore& k, const double* __restrict__ det_tlbr, const double* __restrict__ det_xyah,
                                                       const double* __restrict__ det_score, int m, int flags, double lambda,
                                                       double* __restrict__ out, size_t ld, int* __restrict__ status, int a0, int b0) {
#pragma clang fp contract(off)
    __shared__ double sbox[PW_TA][4], smu[PW_TA][4], sL[PW_TA][4][4];
    __shared__ int sstate[PW_TA];                                  // 0 a good track, 1 S not positive definite, 2 skipped
    __shared__ double sb[PW_TB][4], sz[PW_TB][4];
    const int tid = threadIdx.x;
    const bool motion = (flags & (KSTORE_FUSE_MOTION | KSTORE_GATE_ONLY)) != 0;
    const int only_position = (flags & KSTORE_ONLY_POSITION) ? 1 : 0;
    if (tid < PW_TA) {
        const int t = a0 + tid;
        int s, state = 2;
        if (t < k.n && kstore_live(k, t, s)) {
            const double* pm = k.mean + (size_t)s * 8;
            double b[4], mu[4], L[4][4];
            kalman_box_of(pm, 1, b);
            state = 0;
            if (motion && !kalman_gate_factor(pm, k.cov + (size_t)s * 64, only_position, 0, mu, L)) state = 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sbox[tid][i] = b[i];
                if (motion) {
                    smu[tid][i] = mu[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) sL[tid][i][j] = L[i][j];
                }
            }
        }
        sstate[tid] = state;
        if (b0 == 0 && t < k.n && status != nullptr) status[t] = state == 1 ? 1 : 0;
    }
    {
        const int r = b0 + tid / 4;
        sb[tid / 4][tid % 4] = r < m ? det_tlbr[(size_t)r * 4 + tid % 4] : 0.0;
        if (motion) sz[tid / 4][tid % 4] = r < m ? det_xyah[(size_t)r * 4 + tid % 4] : 0.0;
    }
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= m) return;
    const double bx1 = sb[col][0], by1 = sb[col][1], bx2 = sb[col][2], by2 = sb[col][3];
    const double gate_at = only_position ? 5.9915 : 9.4877;        // chi2inv95[2], chi2inv95[4] (kalman_filter.py:10-19)
#pragma unroll
    for (int q = 0; q < PW_TA / 4; ++q) {
        const int ri = rg + 4 * q, i = a0 + ri;
        if (i >= k.n) continue;
        const int state = sstate[ri];
        double v;
        if (state == 2) v = INFINITY;
        else {
            v = pairwise_iou_cost(pairwise_iou(sbox[ri][0], sbox[ri][1], sbox[ri][2], sbox[ri][3], bx1, by1, bx2, by2),
                                  det_score != nullptr ? det_score + j : nullptr);
            if (motion) {
                double g;
                if (state == 1) g = __builtin_nan("");
                else {
                    double d[4], L[4][4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        d[c] = sz[col][c] - smu[ri][c];
#pragma unroll
                        for (int e = 0; e < 4; ++e) L[c][e] = sL[ri][c][e];
                    }
                    g = only_position ? kalman_gate_one<2>(L, d, 0) : kalman_gate_one<4>(L, d, 0);
                }
                if (g > gate_at) v = INFINITY;                      // cost_matrix[row, gating_distance > gating_threshold] = np.inf
                if (flags & KSTORE_FUSE_MOTION) v = lambda * v + (1.0 - lambda) * g;
            }
        }
        out[(size_t)i * ld + j] = v;
    }
}

__global__ void __launch_bounds__(256) kstore_round_cost_kernel(KStore k, const double* __restrict__ det_tlbr, const double* __restrict__ det_xyah,
                                                                const double* __restrict__ det_score, int m, int flags, double lambda,
                                                                double* __restrict__ out, int* __restrict__ status) {
    kstore_round_cost_tile(k, det_tlbr, det_xyah, det_score, m, flags, lambda, out, (size_t)m, status, blockIdx.y * PW_TA, blockIdx.x * PW_TB);
}
