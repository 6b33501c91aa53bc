// Track-state kernels of ByteTrack's association rounds (SURVEY 8f-2; float64, bit-exact against numpy).
//
//  kalman_predict_kernel : STrack.multi_predict, adapters/ByteTrack/yolox/tracker/byte_tracker.py:50-61, which zeroes
//      mean[7] of every non-Tracked track and calls KalmanFilter.multi_predict (the copy the adapter falls back to:
//      adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py:154-190, matrices :40-52): state (x, y, a, h, vx, vy,
//      va, vh), F = I + shift-by-4, process noise from the box height with weights 1/20 and 1/160.
//      F is a 0/1 matrix, so numpy's  dot(mean, F.T)  and  dot(dot(F, P).transpose, F.T) + Q  reduce to sums of at most two
//      non-zero terms per product - the evaluation order below reproduces them bit for bit whatever BLAS does.
//  kalman_update_kernel  : KalmanFilter.project + update, kalman_filter.py:125-152,193-225 (STrack.update / re_activate,
//      byte_tracker.py:78,109): S = P[:4,:4] + diag(std^2), lower Cholesky factor of S, gain K = P H^T S^-1 by a forward and a
//      back substitution per state row, mean += (z - mean[:4]) K^T, P -= K S K^T.  H = [I 0], so H P H^T and P H^T are blocks of P.
//      The reference factors and solves in LAPACK; the sums below run left to right - another valid float64 order of the same
//      formulas, not a bit-exact one.  A pivot that is not positive and finite (scipy.linalg.cho_factor raises LinAlgError)
//      leaves the track as it was and sets its status word.
//  kalman_initiate_kernel: KalmanFilter.initiate, kalman_filter.py:54-85 (STrack.activate, byte_tracker.py:67), numpy's
//      left-to-right products: bit-exact.
//  kalman_boxes_kernel   : STrack.tlwh / tlbr of a state, byte_tracker.py:142-163: bit-exact.
//  kalman_gating_kernel  : KalmanFilter.gating_distance, kalman_filter.py:227-269 (matching.py:132-156): one track and a tile of
//      KALMAN_GATE_TILE measurements per workgroup; every lane factors the track's S itself (10 products), then solves its own
//      measurements.  np.linalg.cholesky raises where the status word is set; such a row is filled with NaN.
//  duplicate_mark_kernel : remove_duplicate_stracks, byte_tracker.py:685-698 - pairs with IoU cost < 0.15; the track with
//      the shorter life (frame_id - start_frame) is dropped, ties drop the first list's track.

// The per-track bodies below are what one 64-lane workgroup does for ONE track, given where that track's state lives: the kernels of this file index
// the state by list position, the slot-indexed kernels of kalman_store_kernel.hip.inc by slot.  `tid`: the lane, 0 .. 63; every lane of the workgroup calls.
__device__ __forceinline__ void kalman_predict_track(double* __restrict__ pm, double* __restrict__ pc, bool zero_vh, int tid) {
#pragma clang fp contract(off)
    __shared__ double P[8][8], L[8][8], m[8];
    P[tid >> 3][tid & 7] = pc[tid];
    if (tid < 8) m[tid] = (tid == 7 && zero_vh) ? 0.0 : pm[tid];
    __syncthreads();
    const int i = tid >> 3, j = tid & 7;
    // left = F P : rows 0-3 add the velocity rows
    L[i][j] = i < 4 ? P[i][j] + P[i + 4][j] : P[i][j];
    __syncthreads();
    // (left F^T)[i][j] = left[i][j] + left[i][j+4] for j < 4
    double v = j < 4 ? L[i][j] + L[i][j + 4] : L[i][j];
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

__global__ void __launch_bounds__(64) kalman_predict_kernel(double* __restrict__ mean, double* __restrict__ cov, const uint8_t* __restrict__ not_tracked, int n) {
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= n) return;
    kalman_predict_track(mean + (size_t)t * 8, cov + (size_t)t * 64, not_tracked != nullptr && not_tracked[t], tid);
}

// Lower Cholesky factor of the leading DIM x DIM block of S, column by column.  false: a pivot is not positive and finite.
template <int DIM>
__device__ __forceinline__ bool kalman_cholesky(const double (&S)[4][4], double (&L)[4][4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
        double d = S[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > 0.0) || d == INFINITY) return false;
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < DIM; ++i) {
            double v = S[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    return true;
}

// diag(square(std)) of KalmanFilter.project (kalman_filter.py:142-147) for box height h
__device__ __forceinline__ double kalman_innovation_var(int i, double h) {
#pragma clang fp contract(off)
    const double sd = i == 2 ? 1e-1 : (1.0 / 20) * h;
    return sd * sd;
}

// `z`: the track's measurement [4];  `st`: its status word, or nullptr
__device__ __forceinline__ void kalman_update_track(double* __restrict__ pm, double* __restrict__ pc, const double* __restrict__ z, int* __restrict__ st, int tid) {
#pragma clang fp contract(off)
    __shared__ double P[8][8], Ss[4][4], K[8][4], KS[8][4], m[8], inn[4];
    P[tid >> 3][tid & 7] = pc[tid];
    if (tid < 8) m[tid] = pm[tid];
    __syncthreads();
    if (tid < 16) {
        const int i = tid >> 2, j = tid & 3;
        Ss[i][j] = P[i][j] + (i == j ? kalman_innovation_var(i, m[3]) : 0.0);
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

__global__ void __launch_bounds__(64) kalman_update_kernel(double* __restrict__ mean, double* __restrict__ cov, const double* __restrict__ meas, int n,
                                                           int* __restrict__ status) {
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= n) return;
    kalman_update_track(mean + (size_t)t * 8, cov + (size_t)t * 64, meas + (size_t)t * 4, status != nullptr ? status + t : nullptr, tid);
}

__device__ __forceinline__ void kalman_initiate_track(const double* __restrict__ z, double* __restrict__ pm, double* __restrict__ pc, int tid) {
#pragma clang fp contract(off)
    const int i = tid >> 3, j = tid & 7;
    double v = 0.0;
    if (i == j) {
        const double h = z[3];
        const double wp = 1.0 / 20, wv = 1.0 / 160;
        double sd;
        if (i == 2) sd = 1e-2;
        else if (i == 6) sd = 1e-5;
        else sd = i < 4 ? (2 * wp) * h : (10 * wv) * h;    // 2 * w * h evaluates left to right in Python
        v = sd * sd;
    }
    pc[tid] = v;
    if (tid < 8) pm[tid] = tid < 4 ? z[tid] : 0.0;
}

__global__ void __launch_bounds__(64) kalman_initiate_kernel(const double* __restrict__ meas, int n, double* __restrict__ mean, double* __restrict__ cov) {
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= n) return;
    kalman_initiate_track(meas + (size_t)t * 4, mean + (size_t)t * 8, cov + (size_t)t * 64, tid);
}

// STrack.tlwh (tlbr = 0) / STrack.tlbr of one state
__device__ __forceinline__ void kalman_box_of(const double* __restrict__ pm, int tlbr, double (&o)[4]) {
#pragma clang fp contract(off)
    const double h = pm[3];
    const double w = pm[2] * h;                            // ret[2] *= ret[3]
    const double x = pm[0] - w / 2, y = pm[1] - h / 2;     // ret[:2] -= ret[2:] / 2
    o[0] = x;
    o[1] = y;
    o[2] = tlbr ? w + x : w;                               // ret[2:] += ret[:2]
    o[3] = tlbr ? h + y : h;
}

__global__ void __launch_bounds__(256) kalman_boxes_kernel(const double* __restrict__ mean, int n, int tlbr, double* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double b[4];
    kalman_box_of(mean + t * 8, tlbr, b);
    double* o = out + t * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = b[k];
}

#define KALMAN_GATE_TILE 256

template <int DIM>
__device__ __forceinline__ double kalman_gate_one(const double (&L)[4][4], const double (&d)[4], int metric) {
#pragma clang fp contract(off)
    double z[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        double v = d[i];
        if (metric == 0) {                                 // solve_triangular(L, d, lower=True)
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - L[i][k] * z[k];
            v = v / L[i][i];
        }
        z[i] = v;
    }
    double s = z[0] * z[0];
#pragma unroll
    for (int i = 1; i < DIM; ++i) s = s + z[i] * z[i];
    return s;
}

// What every measurement of a track's gating row shares: the projected mean mu = mean[:4] and, for the Mahalanobis metric, the lower Cholesky factor
// of S = P[:4,:4] + diag(std^2) - its leading 2 x 2 block with `only_position`.  false: S is not positive definite.
__device__ __forceinline__ bool kalman_gate_factor(const double* __restrict__ pm, const double* __restrict__ pc, int only_position, int metric,
                                                   double (&mu)[4], double (&L)[4][4]) {
#pragma clang fp contract(off)
    double S[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mu[i] = pm[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) L[i][j] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[i][j] = pc[i * 8 + j] + (i == j ? kalman_innovation_var(i, mu[3]) : 0.0);
    bool ok = true;
    if (metric == 0) ok = only_position ? kalman_cholesky<2>(S, L) : kalman_cholesky<4>(S, L);
    return ok;
}

__global__ void __launch_bounds__(64) kalman_gating_kernel(const double* __restrict__ mean, const double* __restrict__ cov, int n,
                                                           const double* __restrict__ meas, int m, int only_position, int metric,
                                                           double* __restrict__ out, int* __restrict__ status) {
#pragma clang fp contract(off)
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= n) return;
    double mu[4], L[4][4];
    const bool ok = kalman_gate_factor(mean + (size_t)t * 8, cov + (size_t)t * 64, only_position, metric, mu, L);
    if (blockIdx.y == 0 && tid == 0 && status != nullptr) status[t] = ok ? 0 : 1;
    for (int q = 0; q < KALMAN_GATE_TILE / 64; ++q) {
        const long j = (long)blockIdx.y * KALMAN_GATE_TILE + q * 64 + tid;
        if (j >= m) return;
        double d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = meas[j * 4 + i] - mu[i];
        double v;
        if (!ok) v = __builtin_nan("");
        else v = only_position ? kalman_gate_one<2>(L, d, metric) : kalman_gate_one<4>(L, d, metric);
        out[(size_t)t * m + j] = v;
    }
}

__global__ void __launch_bounds__(256) duplicate_mark_kernel(const double* __restrict__ cost, int nA, int nB, const int* __restrict__ ageA,
                                                             const int* __restrict__ ageB, double thresh, uint8_t* __restrict__ keepA, uint8_t* __restrict__ keepB) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nA * nB) return;
    const int p = (int)(idx / nB), q = (int)(idx % nB);
    if (cost[idx] < thresh) {
        if (ageA[p] > ageB[q]) keepB[q] = 0;               // every racing writer stores the same value
        else keepA[p] = 0;
    }
}
