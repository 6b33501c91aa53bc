// Proposal-side geometry kernels (HBM-bound; float64, bit-exact against the numpy/scipy/cython_bbox path).
//
//  pairwise_kernel : busca/tracking.py:23-60 (center_distance) and
//                    adapters/ByteTrack/yolox/tracker/matching.py:53-91,173-186 (ious / iou_distance / fuse_score)
//  topk_rows_kernel: busca/network.py:333-338 (np.argsort(row)[:P], ties broken by the lower index)
//
// A 16 x 64 output tile per 256-thread block: the 16 A boxes and 64 B boxes are staged once in LDS
// (coalesced 32-byte box loads), every thread produces 4 outputs of one column, and each output row is
// written as 64 consecutive doubles (512 B per wave-row).  No FMA contraction anywhere: scipy/cython
// evaluate sqrt(dx*dx + dy*dy) and (area_a + area_b) - iw*ih with separate roundings.

#define PW_TA 16
#define PW_TB 64

// bbox_overlaps of one pair, "+1" pixel convention (matching.py:53-91, cython_bbox)
__device__ __forceinline__ double pairwise_iou(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2, double by2) {
#pragma clang fp contract(off)
    const double iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1) + 1.0;
    double iou = 0.0;
    if (iw > 0) {
        const double ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1) + 1.0;
        if (ih > 0) {
            const double area_a = (ax2 - ax1 + 1.0) * (ay2 - ay1 + 1.0);
            const double area_b = (bx2 - bx1 + 1.0) * (by2 - by1 + 1.0);
            const double inter = iw * ih;
            const double ua = (area_a + area_b) - inter;
            iou = inter / ua;
        }
    }
    return iou;
}

// iou_distance of one pair and, with the detection's score (`score` not NULL), fuse_score (matching.py:173-186)
__device__ __forceinline__ double pairwise_iou_cost(double iou, const double* __restrict__ score) {
#pragma clang fp contract(off)
    double v = 1.0 - iou;                                   // iou_distance
    if (score != nullptr) {                                 // fuse_score: 1 - (1 - cost) * score
        const double sim = 1.0 - v;
        const double fs = sim * *score;
        v = 1.0 - fs;
    }
    return v;
}

__global__ void __launch_bounds__(256) pairwise_kernel(const double* __restrict__ A, int nA, const double* __restrict__ Bx, int nB,
                                                       int mode, const double* __restrict__ scores, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sa[PW_TA][4];
    __shared__ double sb[PW_TB][4];
    const int tid = threadIdx.x;
    const int a0 = blockIdx.y * PW_TA, b0 = blockIdx.x * PW_TB;
    if (tid < PW_TA * 4) { const int r = a0 + tid / 4; sa[tid / 4][tid % 4] = r < nA ? A[(size_t)r * 4 + tid % 4] : 0.0; }
    { const int r = b0 + tid / 4; sb[tid / 4][tid % 4] = r < nB ? Bx[(size_t)r * 4 + tid % 4] : 0.0; }
    __syncthreads();
    const int col = tid & 63, rg = tid >> 6;
    const int j = b0 + col;
    if (j >= nB) return;
    const double bx1 = sb[col][0], by1 = sb[col][1], bx2 = sb[col][2], by2 = sb[col][3];
#pragma unroll
    for (int k = 0; k < PW_TA / 4; ++k) {
        const int ri = rg + 4 * k, i = a0 + ri;
        if (i >= nA) continue;
        const double ax1 = sa[ri][0], ay1 = sa[ri][1], ax2 = sa[ri][2], ay2 = sa[ri][3];
        double v;
        if (mode == BUSCA_PAIR_CENTER || mode == BUSCA_PAIR_CENTER_WEIGHTED) {
            const double acx = (ax1 + ax2) / 2.0, acy = (ay1 + ay2) / 2.0;
            const double bcx = (bx1 + bx2) / 2.0, bcy = (by1 + by2) / 2.0;
            const double dx = acx - bcx, dy = acy - bcy;
            const double sx = dx * dx, sy = dy * dy;
            v = sqrt(sx + sy);
            if (mode == BUSCA_PAIR_CENTER_WEIGHTED) {
                const double as = sqrt((ax2 - ax1) * (ay2 - ay1)), bs = sqrt((bx2 - bx1) * (by2 - by1));
                const double r1 = as / bs, r2 = bs / as;
                const double w = (r1 != r1 || r2 != r2) ? (r1 + r2) : (r1 > r2 ? r1 : r2);   // np.maximum propagates NaN
                v = v * w;
            }
        } else {
            const double iou = pairwise_iou(ax1, ay1, ax2, ay2, bx1, by1, bx2, by2);
            if (mode == BUSCA_PAIR_IOU) v = iou;
            else v = pairwise_iou_cost(iou, scores != nullptr ? scores + j : nullptr);
        }
        out[(size_t)i * nB + j] = v;
    }
}

// total order of np.argsort on float64: ascending, -0.0 == +0.0, NaN last; ties by index (stable).
static __device__ __forceinline__ unsigned long long sort_key(double x) {
    if (x != x) return 0xFFFFFFFFFFFFFFFFull;
    x = x + 0.0;                                                // -0.0 -> +0.0
    unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// K10 (busca/network.py:333-338: np.argsort(dists, axis=1)[:, :num_candidates]).  Two flavours, both bit-exact:
//  * topk_rank_kernel (N <= 256 EPT, EPT = 1 / 2: rows of up to 512 columns): one workgroup per row.  The row's keys go to LDS ONCE; thread t holds EPT of them in registers and counts, over one
//    broadcast pass through the LDS copy, how many (key, index) pairs precede each of its own - its RANK in the stable ascending order.  Ranks are a
//    permutation of 0 .. N-1, so "rank < P writes idx[rank]" fills every output slot exactly once: no selection rounds, no cross-lane traffic, no
//    dependent global loads (the round-5 kernel made P serial passes over the row from global memory with 64-bit shuffles: 45-80 us at 128 x 150).
//  * topk_rows_kernel (longer rows): one wavefront per row, P rounds of (key, index) lexicographic arg-min over the entries after the last selected pair.
template <int EPT>
__global__ void __launch_bounds__(256) topk_rank_kernel(const double* __restrict__ dist, int N, int P, int* __restrict__ idx) {
    __shared__ __attribute__((aligned(16))) unsigned long long sk[256 * EPT + 2];
    const int tid = threadIdx.x, row = blockIdx.x;
    const double* d = dist + (size_t)row * N;
    unsigned long long mk[EPT]; int rank[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int c = tid + 256 * e;
        mk[e] = c < N ? sort_key(d[c]) : 0xFFFFFFFFFFFFFFFFull;
        sk[c] = mk[e];
        rank[e] = 0;
    }
    if (tid < 2) sk[256 * EPT + tid] = 0xFFFFFFFFFFFFFFFFull;
    __syncthreads();
    const int N2 = (N + 1) & ~1;                                // (an odd row reads one padding key: its index N is never below a real one's... and its key is the maximum)
    for (int c = 0; c < N2; c += 2) {
        const unsigned long long k0 = sk[c], k1 = sk[c + 1];    // same address in every lane: one broadcast ds_read_b128
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int me = tid + 256 * e;
            rank[e] += (k0 < mk[e] || (k0 == mk[e] && c < me)) ? 1 : 0;
            rank[e] += (c + 1 < N && (k1 < mk[e] || (k1 == mk[e] && c + 1 < me))) ? 1 : 0;
        }
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int c = tid + 256 * e;
        if (c < N && rank[e] < P) idx[(size_t)row * P + rank[e]] = c;
    }
    for (int p = N + tid; p < P; p += 256) idx[(size_t)row * P + p] = -1;      // fewer entries than requested: -1 padding
}

__global__ void __launch_bounds__(256) topk_rows_kernel(const double* __restrict__ dist, int B, int N, int P, int* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const double* d = dist + (size_t)row * N;
    unsigned long long lk = 0; int li = -1;                     // last selected (key, index)
    bool first = true;
    for (int p = 0; p < P; ++p) {
        unsigned long long bk = 0xFFFFFFFFFFFFFFFFull; int bi = 0x7FFFFFFF;
        if (p < N) {
            for (int c = lane; c < N; c += 64) {
                const unsigned long long k = sort_key(d[c]);
                const bool after = first || k > lk || (k == lk && c > li);
                if (after && (k < bk || (k == bk && c < bi))) { bk = k; bi = c; }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long ok = __shfl_xor(bk, o);
                const int oi = __shfl_xor(bi, o);
                if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
            }
            lk = bk; li = bi; first = false;
        }
        if (lane == 0) idx[(size_t)row * P + p] = p < N ? bi : -1;
    }
}


// Detection coverage (adapters/ByteTrack/yolox/tracker/byte_tracker.py:574-623, reliability gate :459-465): number of
// pixels of an H x W frame covered by the union of n filled rectangles.  cv2.rectangle(thickness=-1) semantics: corners
// are int()-truncated by the caller, either order, both corner pixels included, clipped to the frame.
// One thread per pixel, boxes staged in LDS in chunks, block reduction, one atomic per block.  HBM traffic: none but
// the boxes - the reference's H x W x 3 uint8 canvas never exists.
__global__ void __launch_bounds__(256) coverage_kernel(const int* __restrict__ rect /* [n][4] x1,y1,x2,y2 (ordered, clipped) */, int n,
                                                       int H, int W, unsigned long long* __restrict__ count) {
    __shared__ int sr[256][4];
    __shared__ unsigned int part[4];
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    const int y = (int)(pix / W), x = (int)(pix % W);
    const bool in_img = pix < (long)H * W;
    bool hit = false;
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sr[threadIdx.x][k] = rect[(size_t)(base + threadIdx.x) * 4 + k];
        }
        __syncthreads();
        if (in_img && !hit)
            for (int i = 0; i < m; ++i)
                if (x >= sr[i][0] && x <= sr[i][2] && y >= sr[i][1] && y <= sr[i][3]) { hit = true; break; }
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (unsigned int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(count, (unsigned long long)t);
    }
}
