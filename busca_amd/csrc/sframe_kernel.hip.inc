// The three kernels of a StrongSORT frame on resident track state (include/busca_sframe.h), around the staged assignment.  The arithmetic is included
// text: sort_predict_track, sort_update_track, sort_clamp, sort_iou_cost and the camera warp of sort_kernel.hip.inc, kalman_gate_factor,
// kalman_gate_one, kalman_box_of and kalman_initiate_track of track_kernel.hip.inc, store_blend, store_div_rn and store_sqrt_rn of
// store_kernel.hip.inc, the addressing of kalman_store_kernel.hip.inc (KStore, kstore_live) - all included by the unit before this file.
//
//  sframe_advance_kernel : one 64-lane workgroup per listed slot: (with a warp) Track.camera_update of the stored mean by lane 0 - the statements of
//      sort_camera_update_kernel on one track -, a barrier, then Track.predict.
//  sframe_cost_kernel    : the [2, n, m] slab.  A PW_TA x PW_TB (16 x 64) tile per 256-lane workgroup, as sort_gate_cost_kernel and
//      sort_iou_cost_kernel, which it merges: lanes 0 .. 15 stage one track each (projected mean, Cholesky factor, tlwh box - each only where the
//      row's stage reads that plane), all lanes stage the detections, then every lane produces the four rows of one column in both planes.
//  sframe_apply_kernel   : n + m workgroups of 64 lanes.  Workgroup i < n: the EMA feature row and the NSA update of slot[i] with the detection the
//      solver matched it to.  Workgroup n + j: KalmanFilter.initiate and the first feature row of detection j, when j starts a track; its rank
//      among such columns is counted by the workgroup itself over the columns below j, as frame_apply_kernel counts it.  Both decisions are
//      uniform over the workgroup.
//
// The bodies are device functions - sframe_advance_track, sframe_stage_row / sframe_stage_dets / sframe_entry, sframe_apply_row / sframe_apply_col -
// which msframe_kernel.hip.inc (libbusca_msframe.so) calls once per (problem, row), (problem, tile) and (problem, column) of a batch: one text behind
// two addressings.
//
// No multiply-add contraction anywhere in this file (store_kernel.hip.inc, included last, leaves the file-scope mode at `fast`).
#pragma clang fp contract(off)

// With a warp, Track.camera_update of the stored mean by lane 0, a barrier, then Track.predict of the state at (pm, pc): the order of the reference's
// loop (deep_sort_app.py:186-189), so the prediction's process noise reads the warped height.  All 64 lanes of the workgroup call it (with a warp it
// holds a barrier more).  sframe_advance_kernel and msframe_advance_kernel (msframe_kernel.hip.inc, libbusca_msframe.so) are this function behind two
// addressings.
__device__ __forceinline__ void sframe_advance_track(double* pm, double* pc, const double* __restrict__ matrix, int tid) {
    if (matrix != nullptr) {                                       // uniform over the workgroup
        if (tid == 0) {
            double b[4];
            kalman_box_of(pm, 1, b);
            const double m00 = matrix[0], m01 = matrix[1], m02 = matrix[2], m10 = matrix[3], m11 = matrix[4], m12 = matrix[5];
            const double x1 = (m00 * b[0] + m01 * b[1]) + m02, y1 = (m10 * b[0] + m11 * b[1]) + m12;
            const double x2 = (m00 * b[2] + m01 * b[3]) + m02, y2 = (m10 * b[2] + m11 * b[3]) + m12;
            const double w = x2 - x1, h = y2 - y1;
            pm[0] = x1 + w / 2;
            pm[1] = y1 + h / 2;
            pm[2] = w / h;
            pm[3] = h;
        }
        __syncthreads();                                           // the warped mean is what lanes 0 .. 7 read next
    }
    sort_predict_track(pm, pc, tid);
}

__global__ void __launch_bounds__(64) sframe_advance_kernel(KStore k, const double* __restrict__ matrix) {
    const int t = blockIdx.x, tid = threadIdx.x;
    int s;
    if (t >= k.n || !kstore_live(k, t, s)) return;                 // uniform over the workgroup
    sframe_advance_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, matrix, tid);
}

struct SFrameCost {
    const double* det_xyah;     // [m,4]
    const double* det_tlwh;     // [m,4]
    const uint8_t* stale;       // [n] or nullptr
    const double* cost;         // [n, ld_cost]
    const int* first;           // [n]
    const int* again;           // [n] or nullptr
    double* out;                // [2, n, m]
    int* status;                // [n] or nullptr
    double gated_cost, lambda, rest, max_distance, limit;          // plane 0: rest = 1 - lambda, limit = max_distance + 1e-5, rounded on the host
    double max_iou, iou_limit;                                     // plane 1: iou_limit = max_iou + 1e-5
    int m, ld_cost, flags, depth;
};

#define SFRAME_UNREAD 3         // a row state: no stage reads this plane of the row

// what a workgroup stages of its PW_TA x PW_TB tile, in LDS
struct SFrameTile {
    double mu[PW_TA][4], L[PW_TA][4][4], box[PW_TA][4];
    int gate[PW_TA];                                               // plane 0: 0 a good track, 1 S not positive definite, 2 skipped, 3 not read
    int iou[PW_TA];                                                // plane 1: 0 a row of IoU costs, 2 stale or skipped, 3 not read
    double z[PW_TB][4], b[PW_TB][4];
};

// Row r of the tile, row t of the list k.slot[0 .. k.n) (t >= k.n: a row that is not there), staged by one lane: the projected mean, the Cholesky
// factor and the tlwh box, each only where the row's stage reads that plane.  `a.first`, `a.again`, `a.stale` and `a.status` are indexed by t; the
// status word is written where `with_status` (the tiles of column block 0).
__device__ __forceinline__ void sframe_stage_row(SFrameTile& T, const KStore& k, const SFrameCost& a, int r, int t, bool with_status) {
    int gate = SFRAME_UNREAD, iou = SFRAME_UNREAD;
    if (t < k.n) {
        const int f = a.first[t], g = a.again != nullptr ? a.again[t] : -1;
        int s;
        const bool live = kstore_live(k, t, s);
        if (f >= 0 && f < a.depth) {
            gate = 2;
            if (live) {
                double mu[4], L[4][4];
                gate = kalman_gate_factor(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, 0, 0, mu, L) ? 0 : 1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    T.mu[r][i] = mu[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) T.L[r][i][j] = L[i][j];
                }
            }
        }
        if (f == a.depth || g == a.depth) {
            iou = 2;
            if (live && !(a.stale != nullptr && a.stale[t])) {
                double b[4];
                kalman_box_of(k.mean + (size_t)s * 8, 0, b);
#pragma unroll
                for (int i = 0; i < 4; ++i) T.box[r][i] = b[i];
                iou = 0;
            }
        }
        if (with_status && a.status != nullptr) a.status[t] = gate == 1 ? 1 : 0;
    }
    T.gate[r] = gate;
    T.iou[r] = iou;
}

// the detections b0 .. b0 + PW_TB - 1 of a.m, by all 256 lanes
__device__ __forceinline__ void sframe_stage_dets(SFrameTile& T, const SFrameCost& a, int b0, int tid) {
    const int r = b0 + tid / 4;
    T.z[tid / 4][tid % 4] = r < a.m ? a.det_xyah[(size_t)r * 4 + tid % 4] : 0.0;
    T.b[tid / 4][tid % 4] = r < a.m ? a.det_tlwh[(size_t)r * 4 + tid % 4] : 0.0;
}

// The entry (row ri, column col) of the staged tile in both planes.  `appear`: where the appearance cost of the pair stands; it is read only for a
// good track whose gate admits the pair.
__device__ __forceinline__ void sframe_entry(const SFrameTile& T, const SFrameCost& a, int ri, int col, const double* __restrict__ appear, double& v0,
                                             double& v1) {
    const int gate = T.gate[ri], iou = T.iou[ri];
    v0 = INFINITY, v1 = INFINITY;
    if (gate != SFRAME_UNREAD) {                                   // sort_gate_cost_kernel's entry
        double v;
        if (gate == 2) v = a.gated_cost;
        else if (gate == 1) v = __builtin_nan("");
        else {
            double d[4], L[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d[c] = T.z[col][c] - T.mu[ri][c];
#pragma unroll
                for (int e = 0; e < 4; ++e) L[c][e] = T.L[ri][c][e];
            }
            const double g = kalman_gate_one<4>(L, d, 0);
            v = g > 9.4877 ? a.gated_cost : *appear;               // chi2inv95[4]
            if (a.flags & SORT_MC) v = a.lambda * v + a.rest * g;
        }
        v0 = sort_clamp(v, a.flags, a.max_distance, a.limit);
    }
    if (iou != SFRAME_UNREAD) {                                    // sort_iou_cost_kernel's entry
        double v = SORT_INFTY_COST;
        if (iou == 0) {
            const double t[4] = {T.box[ri][0], T.box[ri][1], T.box[ri][2], T.box[ri][3]};
            const double b[4] = {T.b[col][0], T.b[col][1], T.b[col][2], T.b[col][3]};
            v = sort_iou_cost(t, b);
        }
        v1 = sort_clamp(v, SORT_CLAMP, a.max_iou, a.iou_limit);
    }
}

__global__ void __launch_bounds__(256) sframe_cost_kernel(KStore k, SFrameCost a) {
    __shared__ SFrameTile T;
    const int tid = threadIdx.x, a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (tid < PW_TA) sframe_stage_row(T, k, a, tid, a0 + tid, b0 == 0);
    sframe_stage_dets(T, a, b0, tid);
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= a.m) return;
    const size_t plane = (size_t)k.n * (size_t)a.m;
#pragma unroll
    for (int q = 0; q < PW_TA / 4; ++q) {
        const int ri = rg + 4 * q, i = a0 + ri;
        if (i >= k.n) continue;
        double v0, v1;
        sframe_entry(T, a, ri, col, a.cost + ((size_t)i * a.ld_cost + j), v0, v1);
        const size_t at = (size_t)i * a.m + j;
        a.out[at] = v0;
        a.out[plane + at] = v1;
    }
}

struct SFrameApply {
    const int* row_to_col;      // [n]
    const int* col_to_row;      // [m]
    const double* det_xyah;     // [m,4]
    const double* det_conf;     // [m] or nullptr
    const float* det_feat;      // [m,E]
    float* feat;                // [S+1,E]
    const int* free_slot;       // [n_free]
    int* new_slot;              // [m]
    int* status;                // [n] or nullptr
    float wa, wb;               // (float)alpha, (float)(1.0 - alpha)
    int m, E, n_free;
};

// The norm store_block_norm gives its 256 threads, by one wave: lane l holds in sq[w] the sum thread l + 64 w of that kernel holds (the squares of
// elements l + 64 w, l + 64 w + 256, .. in ascending order, in float64).  Each of the four is reduced over the lanes by the same xor-shuffles
// (offsets 32 .. 1) - what the four waves of that kernel do -, then (w0 + w1) + (w2 + w3), rounded once to float32, then the root: the same sums in
// the same order, so the same bits.  No LDS, no barrier.
__device__ __forceinline__ float sframe_wave_norm(double (&sq)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w)
        for (int o = 32; o >= 1; o >>= 1) sq[w] = sq[w] + __shfl_xor(sq[w], o, 64);
    return store_sqrt_rn((float)((sq[0] + sq[1]) + (sq[2] + sq[3])));
}

// ||d|| of the E values at d
__device__ __forceinline__ float sframe_row_norm(const float* __restrict__ d, int E, int lane) {
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < 4; ++w)
        for (int e = lane + 64 * w; e < E; e += STORE_THREADS) sq[w] = sq[w] + (double)d[e] * (double)d[e];
    return sframe_wave_norm(sq);
}

// row = d / ||d||  (track.py:85-87): the `!old` branch of store_ema_fit_kernel
__device__ __forceinline__ void sframe_first_feature(float* row, const float* __restrict__ d, int E, int lane) {
    const float nf = sframe_row_norm(d, E, lane);
    for (int e = lane; e < E; e += 64) row[e] = store_div_rn(d[e], nf);
}

// row = smooth / ||smooth||, smooth = wa * row + wb * d / ||d||  (track.py:244-248): the other branch.  Lane l reads and writes row[l], row[l + 64],
// .. alone, and the second pass recomputes `smooth` from the values the first read - the row is not written before.
__device__ __forceinline__ void sframe_ema_feature(float* row, const float* __restrict__ d, float wa, float wb, int E, int lane) {
    const float nf = sframe_row_norm(d, E, lane);
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < 4; ++w)
        for (int e = lane + 64 * w; e < E; e += STORE_THREADS) {
            const float sm = store_blend(wa, row[e], wb, store_div_rn(d[e], nf));
            sq[w] = sq[w] + (double)sm * (double)sm;
        }
    const float ns = sframe_wave_norm(sq);
    for (int e = lane; e < E; e += 64) {                           // the same operations on the same operands: the same `sm`
        const float sm = store_blend(wa, row[e], wb, store_div_rn(d[e], nf));
        row[e] = store_div_rn(sm, ns);
    }
}

// Row b of the list: Track.update of slot[b] with its match.  All 64 lanes of the workgroup call it.
__device__ __forceinline__ void sframe_apply_row(const KStore& k, const SFrameApply& f, int b, int tid) {
    int s;
    const int j = f.row_to_col[b];
    if (!kstore_live(k, b, s) || j < 0 || j >= f.m) {              // uniform over the workgroup
        if (tid == 0 && f.status != nullptr) f.status[b] = 0;
        return;
    }
    sframe_ema_feature(f.feat + (size_t)s * f.E, f.det_feat + (size_t)j * f.E, f.wa, f.wb, f.E, tid);
    sort_update_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, f.det_xyah + (size_t)j * 4, f.det_conf != nullptr ? f.det_conf[j] : 0.0,
                      f.status != nullptr ? f.status + b : nullptr, tid);
}

// Column j < f.m: Tracker._initiate_track, ranked among the unmatched columns below j of f.col_to_row.  All 64 lanes of the workgroup call it.
__device__ __forceinline__ void sframe_apply_col(const KStore& k, const SFrameApply& f, int j, int tid) {
    if (f.col_to_row[j] >= 0) {
        if (tid == 0) f.new_slot[j] = -1;
        return;
    }
    int rank = 0;
    for (int c = tid; c < j; c += 64) rank += f.col_to_row[c] < 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rank += __shfl_xor(rank, off, 64);      // the workgroup is one wave: every lane holds the sum
    if (rank >= f.n_free) {                                        // the store is full
        if (tid == 0) f.new_slot[j] = -2;
        return;
    }
    const int s = f.free_slot[rank];
    if (tid == 0) f.new_slot[j] = s;
    if (s < 0 || s >= k.S) return;
    sframe_first_feature(f.feat + (size_t)s * f.E, f.det_feat + (size_t)j * f.E, f.E, tid);
    kalman_initiate_track(f.det_xyah + (size_t)j * 4, k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, tid);
}

__global__ void __launch_bounds__(64) sframe_apply_kernel(KStore k, SFrameApply f) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < k.n) {
        sframe_apply_row(k, f, b, tid);
        return;
    }
    const int j = b - k.n;
    if (j >= f.m) return;
    sframe_apply_col(k, f, j, tid);
}
