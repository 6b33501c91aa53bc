// GHOST association (include/busca_ghost.h): proxy distances with the two reductions busca_appearance_cost lacks, one proxy vector per track,
// data-driven thresholds, and the mask / blend / threshold pass.  Four kernels:
//
//   ghost_distance_kernel   the gallery flavour of appear_kernel (appear_kernel.hip.inc) with its tile code: appear_tile / appear_diag / appear_dist give
//                           every (sample, detection) pair the bits busca_appearance_cost gives it, and the running min / max / sum are folded in the same
//                           order, so MIN / MEAN / MAX are that entry point's output bit for bit.  MIDRANGE = (max + min) / 2 of the two registers.  MEDIAN
//                           (template flag, the only flavour with LDS) also stages the distances as [count][64] float64 and selects by rank: the lanes
//                           (a, b = 0..3) of a detection column share its rows (row = b mod 4), each ranks its rows under the strict order (value, row)
//                           against all rows, and the two rows of rank (count - 1) / 2 and count / 2 are the median's operands.  Ranks under a strict
//                           order are a permutation, so exactly one row has each rank: no atomics, no ties, the same bits every run.
//   ghost_proxies_kernel    one workgroup per track, thread = feature (coalesced over E), rows walked in chronological order from the ring's newest
//   ghost_thresholds_kernel one workgroup, two passes (mean, then squared deviations) per group of rows, every sum in a fixed order
//   (the bodies of the first and the third are device functions of ghost_body.hip.inc, which mgframe_kernel.hip.inc, libbusca_mgframe.so, calls too)
//   ghost_combine_kernel    one thread per matrix entry (ghost_combine_entry: a device function that gframe_cost_kernel, libbusca_gframe.so, applies
//                           to each motion cost where it is produced)
// No multiply-add contraction anywhere: every formula is written out.
#pragma clang fp contract(off)

#include "ghost_body.hip.inc"   // ghost_distance_entry, ghost_block_sum and ghost_thresholds_groups: the bodies, shared with mgframe_kernel.hip.inc

struct GhostDistArgs {
    const float* gallery; const int* slot; const int* count; const float* dets; double* out;
    int n, budget, m, E, reduce, mt;               // mt = detection tiles per track
};

template <bool MEDIAN>
__global__ void __launch_bounds__(64 * APPEAR_WAVES) ghost_distance_kernel(GhostDistArgs p) {
    extern __shared__ double ghost_lds[];           // MEDIAN: [budget][64] staged distances, then [2][64] the selected pair
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, b = lane >> 4;
    const int tm = blockIdx.x % p.mt, ti = blockIdx.x / p.mt;
    const int col = wave * 16 + a;                                        // this lane's column of the 64-detection tile
    const int j = tm * APPEAR_TILE_M + col;
    const float* brow = j < p.m ? p.dets + (size_t)j * p.E : nullptr;
    const int s = p.slot ? p.slot[ti] : ti;
    int cnt = s < 0 ? 0 : (p.count ? p.count[s] : p.budget);
    cnt = cnt < 0 ? 0 : cnt > p.budget ? p.budget : cnt;
    const float* base = p.gallery + (size_t)(s < 0 ? 0 : s) * p.budget * p.E;
    const double res = ghost_distance_entry<MEDIAN>(base, cnt, p.budget, brow, p.E, p.reduce, ghost_lds, col, a, b);
    if (b == 0 && j < p.m) p.out[(size_t)ti * p.m + j] = res;
}

// ---- proxies ---------------------------------------------------------------------------------------------------------------------
#define GHOST_PROXY_THREADS 256

struct GhostProxyArgs {
    const float* gallery; const int* slot; const int* count; const int* newest; float* out;
    int n, budget, E, mode, window;
};

// chronological row k (0 = oldest of the window) of a ring whose newest row is `nw`: w rows back from it, modulo the budget
__device__ __forceinline__ int ghost_ring_row(int nw, int w, int k, int budget) {
    int r = (nw - (w - 1) + k) % budget;
    return r < 0 ? r + budget : r;
}

__global__ void __launch_bounds__(GHOST_PROXY_THREADS) ghost_proxies_kernel(GhostProxyArgs p) {
    __shared__ double part[GHOST_PROXY_THREADS / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int s = p.slot ? p.slot[i] : i;
    int cnt = s < 0 ? 0 : (p.count ? p.count[s] : p.budget);
    cnt = cnt < 0 ? 0 : cnt > p.budget ? p.budget : cnt;
    float* out = p.out + (size_t)i * p.E;
    if (cnt == 0) {                                                       // a track without samples: NaN, never admissible downstream
        for (int e = tid; e < p.E; e += GHOST_PROXY_THREADS) out[e] = __builtin_nanf("");
        return;
    }
    int nw = p.newest ? p.newest[s] : cnt - 1;
    if (nw < 0 || nw >= p.budget) nw = cnt - 1;
    const int w = (p.window <= 0 || p.window > cnt) ? cnt : p.window;
    const float* base = p.gallery + (size_t)s * p.budget * p.E;
    if (p.mode == BUSCA_GHOST_PROXY_LAST || p.mode == BUSCA_GHOST_PROXY_FIRST) {
        const float* row = base + (size_t)(p.mode == BUSCA_GHOST_PROXY_LAST ? nw : ghost_ring_row(nw, cnt, 0, p.budget)) * p.E;
        for (int e = tid; e < p.E; e += GHOST_PROXY_THREADS) out[e] = row[e];
    } else if (p.mode == BUSCA_GHOST_PROXY_MEDIAN) {
        const int k = (w - 1) >> 1;                                       // the lower median, as torch.median returns
        for (int e = tid; e < p.E; e += GHOST_PROXY_THREADS) {
            float res = 0.f;
            bool nan = false;
            for (int x = 0; x < w; ++x) {                                 // a NaN among the samples is the result, as torch.median gives it
                const float vx = base[(size_t)ghost_ring_row(nw, w, x, p.budget) * p.E + e];
                if (vx != vx) { nan = true; res = vx; }
            }
            for (int x = 0; x < w && !nan; ++x) {                         // rank under the strict order (value, chronological index)
                const float vx = base[(size_t)ghost_ring_row(nw, w, x, p.budget) * p.E + e];
                int rank = 0;
                for (int y = 0; y < w; ++y) {
                    const float vy = base[(size_t)ghost_ring_row(nw, w, y, p.budget) * p.E + e];
                    rank += (vy < vx || (vy == vx && y < x)) ? 1 : 0;
                }
                if (rank == k) { res = vx; break; }
            }
            out[e] = res;
        }
    } else {                                                              // MEAN, MEANNORM
        double sq = 0.0;
        for (int e = tid; e < p.E; e += GHOST_PROXY_THREADS) {
            double acc = 0.0;
            for (int x = 0; x < w; ++x) acc = acc + (double)base[(size_t)ghost_ring_row(nw, w, x, p.budget) * p.E + e];     // oldest -> newest
            const float mean = (float)(acc / (double)w);
            if (p.mode == BUSCA_GHOST_PROXY_MEAN) out[e] = mean;
            else sq = sq + (double)mean * (double)mean;                    // this thread's features, ascending
        }
        if (p.mode == BUSCA_GHOST_PROXY_MEANNORM) {
            for (int o = 32; o >= 1; o >>= 1) sq = sq + __shfl_xor(sq, o);
            if ((tid & 63) == 0) part[tid >> 6] = sq;
            __syncthreads();
            double norm = sqrt((part[0] + part[1]) + (part[2] + part[3]));
            if (norm < 1e-12) norm = 1e-12;                               // F.normalize's eps
            for (int e = tid; e < p.E; e += GHOST_PROXY_THREADS) {
                double acc = 0.0;
                for (int x = 0; x < w; ++x) acc = acc + (double)base[(size_t)ghost_ring_row(nw, w, x, p.budget) * p.E + e];
                const float mean = (float)(acc / (double)w);
                out[e] = (float)((double)mean / norm);
            }
        }
    }
}

// ---- thresholds --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GHOST_THR_THREADS) ghost_thresholds_kernel(const double* cost, long long len_act, long long len_inact, double k_act, double k_inact, double* thr) {
    __shared__ double part[GHOST_THR_THREADS / 64];
    ghost_thresholds_groups<false>(cost, len_act, cost + len_act, len_inact, 0, 0, k_act, k_inact, 3, thr, part);
}

// ---- mask, blend, threshold ------------------------------------------------------------------------------------------------------
struct GhostCombineArgs {
    const double* app; const double* motion; const int* tlabel; const int* dlabel; const double* thr; double* out;
    long long total; int m, num_active; double w_app, w_motion;
};

// One entry of busca_ghost_combine in the reference's order: the class mask, the blend with the motion cost, the threshold.  `thr`: where the
// entry's threshold stands, or nullptr.  ghost_combine_kernel and gframe_cost_kernel (gframe_kernel.hip.inc, libbusca_gframe.so) share it.
__device__ __forceinline__ double ghost_combine_entry(double c, bool other_class, bool blend, double motion, double w_app, double w_motion,
                                                      const double* __restrict__ thr) {
    if (other_class) c = __builtin_nan("");
    if (blend) {
        const double x = w_app * c, y = w_motion * motion;
        c = x + y;
    }
    if (thr) {
        const double t = *thr;
        if (!(c <= t)) c = __builtin_nan("");                              // np.where(dist <= thresh, dist, nan): a NaN threshold leaves nothing
    }
    return c;
}

__global__ void __launch_bounds__(256) ghost_combine_kernel(GhostCombineArgs p) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= p.total) return;
    const int i = (int)(k / p.m), j = (int)(k % p.m);
    p.out[k] = ghost_combine_entry(p.app[k], p.tlabel && p.tlabel[i] != p.dlabel[j], p.motion != nullptr, p.motion ? p.motion[k] : 0.0, p.w_app,
                                   p.w_motion, p.thr ? p.thr + (i < p.num_active ? 0 : 1) : nullptr);
}

#pragma clang fp contract(fast)
