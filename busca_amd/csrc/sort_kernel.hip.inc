// Slot-indexed kernels of StrongSORT's track state (include/busca_sort.h; float64, no contraction).  The state arrays and the slot addressing are those
// of kalman_store_kernel.hip.inc (KStore, kstore_live, kstore_meas), included by the unit before this file with track_kernel.hip.inc, whose Cholesky
// factor, gating solve and box conversion are used as they are.  New here is what StrongSORT's filter does differently from ByteTrack's:
//
//  sort_predict_kernel       : Track.predict.  numpy evaluates multi_dot((F, P, F.T)) as F (P F^T), kalman_predict_track forms (F P) F^T: the same
//      sums in another order, which differ in the last bit where P is not symmetric to the bit.  No mean[7] = 0 rule.
//  sort_update_kernel        : the NSA Kalman update - kalman_update_track with the innovation's standard deviations scaled by 1 - confidence.
//  sort_gate_cost_kernel     : gate_cost_matrix on a given cost matrix, the MC blend and min_cost_matching's clamp; the tile of kstore_round_cost_tile.
//  sort_iou_cost_kernel      : iou_matching.iou_cost of tlwh boxes without the "+1" pixel, stale rows, the clamp; the same tile.
//  sort_camera_update_kernel : Track.camera_update, one lane per track.

#define SORT_MC 1           // BUSCA_SORT_MC
#define SORT_CLAMP 2        // BUSCA_SORT_CLAMP
#define SORT_INFTY_COST 1e+5    // deep_sort/linear_assignment.py:12

__device__ __forceinline__ void sort_predict_track(double* __restrict__ pm, double* __restrict__ pc, int tid) {
#pragma clang fp contract(off)
    __shared__ double P[8][8], R[8][8], m[8];
    P[tid >> 3][tid & 7] = pc[tid];
    if (tid < 8) m[tid] = pm[tid];
    __syncthreads();
    const int i = tid >> 3, j = tid & 7;
    // right = P F^T : columns 0-3 add the velocity columns
    R[i][j] = j < 4 ? P[i][j] + P[i][j + 4] : P[i][j];
    __syncthreads();
    // (F right)[i][j] = right[i][j] + right[i+4][j] for i < 4
    double v = i < 4 ? R[i][j] + R[i + 4][j] : R[i][j];
    if (i == j) {
        const double h = m[3];
        const double wp = 1.0 / 20, wv = 1.0 / 160;
        double sd;
        if (i == 2) sd = 1e-2;
        else if (i == 6) sd = 1e-5;
        else sd = (i < 4 ? wp : wv) * h;
        v = v + sd * sd;                                   // + diag(square(std))
    } else
        v = v + 0.0;                                       // numpy adds the zero off-diagonal of motion_cov (-0.0 -> +0.0)
    pc[tid] = v;
    if (tid < 8) pm[tid] = tid < 4 ? m[tid] + m[tid + 4] : m[tid];
}

__global__ void __launch_bounds__(64) sort_predict_kernel(KStore k) {
    const int t = blockIdx.x, tid = threadIdx.x;
    int s;
    if (t >= k.n || !kstore_live(k, t, s)) return;                 // uniform over the workgroup
    sort_predict_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, tid);
}

// kalman_innovation_var at confidence c: std = [(1 - c) * x for x in std] before np.square
__device__ __forceinline__ double sort_innovation_var(int i, double h, double keep) {
#pragma clang fp contract(off)
    double sd = i == 2 ? 1e-1 : (1.0 / 20) * h;
    sd = keep * sd;
    return sd * sd;
}

// kalman_update_track (track_kernel.hip.inc) with the innovation covariance of confidence `c`: every line after Ss is that body's.
__device__ __forceinline__ void sort_update_track(double* __restrict__ pm, double* __restrict__ pc, const double* __restrict__ z, double c,
                                                  int* __restrict__ st, int tid) {
#pragma clang fp contract(off)
    __shared__ double P[8][8], Ss[4][4], K[8][4], KS[8][4], m[8], inn[4];
    P[tid >> 3][tid & 7] = pc[tid];
    if (tid < 8) m[tid] = pm[tid];
    __syncthreads();
    if (tid < 16) {
        const int i = tid >> 2, j = tid & 3;
        Ss[i][j] = P[i][j] + (i == j ? sort_innovation_var(i, m[3], 1.0 - c) : 0.0);
    } else if (tid < 20)
        inn[tid - 16] = z[tid - 16] - m[tid - 16];
    __syncthreads();
    double S[4][4], L[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[i][j] = Ss[i][j];
    if (!kalman_cholesky<4>(S, L)) {                       // the same answer in every lane: the whole workgroup leaves
        if (tid == 0 && st != nullptr) *st = 1;
        return;
    }
    if (tid < 8) {                                         // row tid of the gain: S x = P[tid][:4]^T (cho_solve)
        double y[4], x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = P[tid][i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
            y[i] = v / L[i][i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double v = y[i];
#pragma unroll
            for (int k = 3; k > i; --k) v = v - L[k][i] * x[k];
            x[i] = v / L[i][i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) K[tid][i] = x[i];
    }
    __syncthreads();
    if (tid < 32) {
        const int i = tid >> 2, k = tid & 3;
        KS[i][k] = ((K[i][0] * Ss[0][k] + K[i][1] * Ss[1][k]) + K[i][2] * Ss[2][k]) + K[i][3] * Ss[3][k];
    }
    __syncthreads();
    const int i = tid >> 3, j = tid & 7;
    pc[tid] = P[i][j] - (((KS[i][0] * K[j][0] + KS[i][1] * K[j][1]) + KS[i][2] * K[j][2]) + KS[i][3] * K[j][3]);
    if (tid < 8) pm[tid] = m[tid] + (((inn[0] * K[tid][0] + inn[1] * K[tid][1]) + inn[2] * K[tid][2]) + inn[3] * K[tid][3]);
    if (tid == 0 && st != nullptr) *st = 0;
}

__global__ void __launch_bounds__(64) sort_update_kernel(KStore k, const double* __restrict__ meas, const int* __restrict__ det_index, int m,
                                                         const double* __restrict__ conf, int* __restrict__ status) {
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= k.n) return;
    int s, j;
    if (!kstore_live(k, t, s) || !kstore_meas(det_index, t, m, j)) {
        if (tid == 0 && status != nullptr) status[t] = 0;
        return;
    }
    sort_update_track(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, meas + (size_t)j * 4, conf != nullptr ? conf[j] : 0.0,
                      status != nullptr ? status + t : nullptr, tid);
}

// cost_matrix[cost_matrix > max_distance] = max_distance + 1e-5 (linear_assignment.py:61); `limit` is that sum
__device__ __forceinline__ double sort_clamp(double v, int flags, double max_distance, double limit) {
    return (flags & SORT_CLAMP) && v > max_distance ? limit : v;
}

struct SortGate {
    const double* det_xyah;     // [m,4]
    const double* cost;         // [n, ld_cost]
    double* out;                // [n, m]
    int* status;                // [n] or nullptr
    double gated_cost, lambda, rest, max_distance, limit;          // rest = 1 - lambda, limit = max_distance + 1e-5: both rounded on the host
    int m, ld_cost, flags;
};

// Tile (blockIdx.y, blockIdx.x) of PW_TA x PW_TB entries, as kstore_round_cost_tile: lanes 0 .. 15 stage one track each (projected mean and
// Cholesky factor), all lanes stage the measurements, then every lane produces four outputs of one column.  An entry of `cost` is read and the same
// entry of `out` written by one lane, so the two may be one array.
__global__ void __launch_bounds__(256) sort_gate_cost_kernel(KStore k, SortGate a) {
#pragma clang fp contract(off)
    __shared__ double smu[PW_TA][4], sL[PW_TA][4][4];
    __shared__ int sstate[PW_TA];                                  // 0 a good track, 1 S not positive definite, 2 skipped
    __shared__ double sz[PW_TB][4];
    const int tid = threadIdx.x, a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (tid < PW_TA) {
        const int t = a0 + tid;
        int s, state = 2;
        if (t < k.n && kstore_live(k, t, s)) {
            double mu[4], L[4][4];
            state = kalman_gate_factor(k.mean + (size_t)s * 8, k.cov + (size_t)s * 64, 0, 0, mu, L) ? 0 : 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                smu[tid][i] = mu[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) sL[tid][i][j] = L[i][j];
            }
        }
        sstate[tid] = state;
        if (b0 == 0 && t < k.n && a.status != nullptr) a.status[t] = state == 1 ? 1 : 0;
    }
    {
        const int r = b0 + tid / 4;
        sz[tid / 4][tid % 4] = r < a.m ? a.det_xyah[(size_t)r * 4 + tid % 4] : 0.0;
    }
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= a.m) return;
#pragma unroll
    for (int q = 0; q < PW_TA / 4; ++q) {
        const int ri = rg + 4 * q, i = a0 + ri;
        if (i >= k.n) continue;
        const int state = sstate[ri];
        double v;
        if (state == 2) v = a.gated_cost;
        else if (state == 1) v = __builtin_nan("");
        else {
            double d[4], L[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d[c] = sz[col][c] - smu[ri][c];
#pragma unroll
                for (int e = 0; e < 4; ++e) L[c][e] = sL[ri][c][e];
            }
            const double g = kalman_gate_one<4>(L, d, 0);
            v = g > 9.4877 ? a.gated_cost : a.cost[(size_t)i * a.ld_cost + j];      // chi2inv95[4]
            if (a.flags & SORT_MC) v = a.lambda * v + a.rest * g;
        }
        a.out[(size_t)i * a.m + j] = sort_clamp(v, a.flags, a.max_distance, a.limit);
    }
}

// np.maximum / np.minimum: a NaN on either side comes through
__device__ __forceinline__ double sort_np_max(double a, double b) { return a > b || a != a ? a : b; }
__device__ __forceinline__ double sort_np_min(double a, double b) { return a < b || a != a ? a : b; }

// 1 - iou(bbox, candidate) of iou_matching.py for tlwh boxes a (the track) and b (the detection)
__device__ __forceinline__ double sort_iou_cost(const double (&a)[4], const double (&b)[4]) {
#pragma clang fp contract(off)
    const double tlx = sort_np_max(a[0], b[0]), tly = sort_np_max(a[1], b[1]);
    const double brx = sort_np_min(a[0] + a[2], b[0] + b[2]), bry = sort_np_min(a[1] + a[3], b[1] + b[3]);
    const double w = sort_np_max(0.0, brx - tlx), h = sort_np_max(0.0, bry - tly);
    const double inter = w * h;
    return 1.0 - inter / (a[2] * a[3] + b[2] * b[3] - inter);
}

struct SortIou {
    const uint8_t* stale;       // [n] or nullptr
    const double* det_tlwh;     // [m,4]
    double* out;                // [n, m]
    double max_distance, limit;
    int m, flags;
};

__global__ void __launch_bounds__(256) sort_iou_cost_kernel(KStore k, SortIou a) {
#pragma clang fp contract(off)
    __shared__ double sbox[PW_TA][4];
    __shared__ int sstate[PW_TA];                                  // 0 a row of IoU costs, 2 stale or skipped
    __shared__ double sb[PW_TB][4];
    const int tid = threadIdx.x, a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (tid < PW_TA) {
        const int t = a0 + tid;
        int s, state = 2;
        if (t < k.n && kstore_live(k, t, s) && !(a.stale != nullptr && a.stale[t])) {
            double b[4];
            kalman_box_of(k.mean + (size_t)s * 8, 0, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) sbox[tid][i] = b[i];
            state = 0;
        }
        sstate[tid] = state;
    }
    {
        const int r = b0 + tid / 4;
        sb[tid / 4][tid % 4] = r < a.m ? a.det_tlwh[(size_t)r * 4 + tid % 4] : 0.0;
    }
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= a.m) return;
    const double b[4] = {sb[col][0], sb[col][1], sb[col][2], sb[col][3]};
#pragma unroll
    for (int q = 0; q < PW_TA / 4; ++q) {
        const int ri = rg + 4 * q, i = a0 + ri;
        if (i >= k.n) continue;
        double v = SORT_INFTY_COST;
        if (sstate[ri] == 0) {
            const double t[4] = {sbox[ri][0], sbox[ri][1], sbox[ri][2], sbox[ri][3]};
            v = sort_iou_cost(t, b);
        }
        a.out[(size_t)i * a.m + j] = sort_clamp(v, a.flags, a.max_distance, a.limit);
    }
}

__global__ void __launch_bounds__(256) sort_camera_update_kernel(KStore k, const double* __restrict__ matrix) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    int s;
    if (t >= k.n || !kstore_live(k, (int)t, s)) return;
    double* pm = k.mean + (size_t)s * 8;
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
