// Appearance state resident on the device (include/busca_store.h): GHOST's feature rings and moving-average table, StrongSORT's EMA feature.  Four kernels,
// one launch per call:
//
//   store_ring_add_kernel   one workgroup per (slot, feature) pair: thread 0 does the ring bookkeeping and broadcasts the row, the threads copy the feature
//                           (store_ring_push / store_ring_copy: device functions that gframe_kernel.hip.inc, libbusca_gframe.so, calls on one wave)
//   store_release_kernel    one thread per listed slot
//   store_mv_avg_kernel     one workgroup per listed track: the newest ring row, blended with the slot's moving average where it has one
//   store_ema_fit_kernel    one workgroup per target: its features of this call in call order, the running row in LDS (E <= STORE_EMA_LDS) until the last
//
// Thread = feature element, strided over E (coalesced, as ghost_proxies_kernel).  A slot outside 0 .. S-1 is skipped before anything of it is addressed.
// No multiply-add contraction anywhere: every product and sum is one rounded float32 operation.
#pragma clang fp contract(off)

#define STORE_THREADS 256
#define STORE_EMA_LDS 4096      // floats of running row kept in LDS; a longer row runs in the slot's ring row 0 (each thread re-reads only what it wrote)

// a * b + c * d as two float32 products and one float32 sum, each rounded (__fmul_rn, __fmul_rn, __fadd_rn): written with the plain operators under
// this file's contract(off), which is what keeps the backend from fusing them - the intrinsics' own bodies are compiled under the header's mode.
__device__ __forceinline__ float store_blend(float a, float b, float c, float d) {
    const float x = a * b, y = c * d;
    return x + y;
}

struct StoreRingArgs {
    float* gallery; int* count; int* newest; unsigned char* mv_seen;
    const int* slot; const float* feats; const int* det_index; const unsigned char* is_new;
    int S, budget, E, m;
};

// The ring bookkeeping of busca_store_ring_add for the valid slot s, by one thread -> the ring row the new sample goes to.  `fresh` starts a new
// track in the slot first.  store_ring_add_kernel and gframe_apply_kernel (gframe_kernel.hip.inc, libbusca_gframe.so) share it and store_ring_copy.
__device__ __forceinline__ int store_ring_push(int* count, int* newest, unsigned char* mv_seen, int budget, int s, bool fresh) {
    const int c = fresh ? 0 : count[s];
    int row = 0;
    if (c != 0) {
        row = (int)(((long long)newest[s] + 1) % budget);                  // a row of the ring whatever `newest` holds
        if (row < 0) row += budget;
    }
    if (fresh) mv_seen[s] = 0;
    newest[s] = row;
    count[s] = c >= budget ? budget : c + 1;
    return row;
}

// gallery[s, row, :] = feats[j, :] by `threads` threads of which this is `tid`: the bits, whatever they encode
__device__ __forceinline__ void store_ring_copy(float* gallery, const float* __restrict__ feats, int budget, int E, int s, int row, int j, int tid, int threads) {
    const unsigned* src = (const unsigned*)(feats + (size_t)j * E);
    unsigned* dst = (unsigned*)(gallery + ((size_t)s * budget + row) * E);
    for (int e = tid; e < E; e += threads) dst[e] = src[e];
}

__global__ void __launch_bounds__(STORE_THREADS) store_ring_add_kernel(StoreRingArgs p) {
    __shared__ int ring_row;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int s = p.slot[i];
    const int j = p.det_index ? p.det_index[i] : i;
    if (s < 0 || s >= p.S || j < 0 || j >= p.m) return;                   // the workgroup's: every thread leaves
    if (tid == 0) ring_row = store_ring_push(p.count, p.newest, p.mv_seen, p.budget, s, p.is_new && p.is_new[i] != 0);
    __syncthreads();
    store_ring_copy(p.gallery, p.feats, p.budget, p.E, s, ring_row, j, tid, STORE_THREADS);
}

__global__ void __launch_bounds__(STORE_THREADS) store_release_kernel(int* count, unsigned char* mv_seen, int S, const int* slot, int k) {
    const int i = blockIdx.x * STORE_THREADS + threadIdx.x;
    if (i >= k) return;
    const int s = slot[i];
    if (s < 0 || s >= S) return;
    count[s] = 0;
    mv_seen[s] = 0;
}

struct StoreMvAvgArgs {
    const float* gallery; const int* count; const int* newest; float* mv_avg; unsigned char* mv_seen; const int* slot; float* out;
    int S, budget, E, num_active;
    float wa_act, wb_act, wa_inact, wb_inact;                              // (float)a and (float)(1.0 - a) of the two groups
};

__global__ void __launch_bounds__(STORE_THREADS) store_mv_avg_kernel(StoreMvAvgArgs p) {
    __shared__ int row_seen[2];                                            // the newest ring row (-1: no sample), whether the slot has a moving average
    const int i = blockIdx.x, tid = threadIdx.x;
    const int s = p.slot[i];
    if (tid == 0) {
        int cnt = (s < 0 || s >= p.S) ? 0 : (p.count ? p.count[s] : p.budget);       // the rules of ghost_proxies_kernel
        cnt = cnt < 0 ? 0 : cnt > p.budget ? p.budget : cnt;
        int nw = -1, seen = 0;
        if (cnt > 0) {
            nw = p.newest ? p.newest[s] : cnt - 1;
            if (nw < 0 || nw >= p.budget) nw = cnt - 1;
            seen = p.mv_seen[s] != 0;
            p.mv_seen[s] = 1;
        }
        row_seen[0] = nw;
        row_seen[1] = seen;
    }
    __syncthreads();
    const int nw = row_seen[0];
    float* out = p.out + (size_t)i * p.E;
    if (nw < 0) {                                                          // a skipped slot or a track without samples: NaN, the tables untouched
        for (int e = tid; e < p.E; e += STORE_THREADS) out[e] = __builtin_nanf("");
        return;
    }
    const float* last = p.gallery + ((size_t)s * p.budget + nw) * p.E;
    float* avg = p.mv_avg + (size_t)s * p.E;
    if (row_seen[1]) {
        const float wa = i < p.num_active ? p.wa_act : p.wa_inact, wb = i < p.num_active ? p.wb_act : p.wb_inact;
        for (int e = tid; e < p.E; e += STORE_THREADS) {
            const float f = store_blend(avg[e], wa, last[e], wb);
            avg[e] = f;
            out[e] = f;
        }
    } else {
        for (int e = tid; e < p.E; e += STORE_THREADS) {
            const float f = last[e];
            avg[e] = f;
            out[e] = f;
        }
    }
}

// Correctly rounded float32 square root and quotient whatever the build's float32 division mode: the float64 operation is correctly rounded and its
// 53 bits are more than 2 * 24 + 2, so rounding its result to float32 is the correctly rounded float32 result (no double-rounding case exists).
__device__ __forceinline__ float store_sqrt_rn(float x) { return (float)__builtin_sqrt((double)x); }
__device__ __forceinline__ float store_div_rn(float a, float b) { return (float)((double)a / (double)b); }

// ||v|| of a row whose squares this thread summed (elements tid, tid + 256, .. in ascending order) into `sq`: the 64 lanes of a wave by xor-shuffles
// (offsets 32 .. 1), the four waves as (w0 + w1) + (w2 + w3), all in float64 (a float32 square is exact there), rounded once to float32, then the root.
__device__ __forceinline__ float store_block_norm(double sq, double* part) {
    for (int o = 32; o >= 1; o >>= 1) sq = sq + __shfl_xor(sq, o);
    __syncthreads();                                                       // the previous norm's readers are done with `part`
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
    __syncthreads();
    return store_sqrt_rn((float)((part[0] + part[1]) + (part[2] + part[3])));
}

struct StoreEmaArgs {
    float* gallery; const float* feats; const int* group_slot; const int* group_old_row; const int* group_start; const int* src;
    int S, ring, E, m, k;
    float wa, wb;                                                          // (float)alpha, (float)(1.0 - alpha)
};

__global__ void __launch_bounds__(STORE_THREADS) store_ema_fit_kernel(StoreEmaArgs p) {
    __shared__ double part[STORE_THREADS / 64];
    __shared__ float held[STORE_EMA_LDS];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int s = p.group_slot[i], old_row = p.group_old_row[i];
    if (s < 0 || s >= p.S || old_row >= p.ring) return;
    int lo = p.group_start[i], hi = p.group_start[i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > p.k ? p.k : hi;
    float* row0 = p.gallery + (size_t)s * p.ring * p.E;
    float* cur = p.E <= STORE_EMA_LDS ? held : row0;                       // thread t alone reads and writes cur[t], cur[t + 256], ..: no barrier is owed
    const float* old = old_row >= 0 ? row0 + (size_t)old_row * p.E : nullptr;
    for (int x = lo; x < hi; ++x) {
        const int j = p.src[x];
        if (j < 0 || j >= p.m) continue;                                   // the workgroup's: every thread skips it
        const float* f = p.feats + (size_t)j * p.E;
        double sq = 0.0;
        for (int e = tid; e < p.E; e += STORE_THREADS) sq = sq + (double)f[e] * (double)f[e];
        const float nf = store_block_norm(sq, part);
        if (!old) {
            for (int e = tid; e < p.E; e += STORE_THREADS) cur[e] = store_div_rn(f[e], nf);
        } else {
            sq = 0.0;
            for (int e = tid; e < p.E; e += STORE_THREADS) {
                const float sm = store_blend(p.wa, old[e], p.wb, store_div_rn(f[e], nf));
                sq = sq + (double)sm * (double)sm;
            }
            const float ns = store_block_norm(sq, part);
            for (int e = tid; e < p.E; e += STORE_THREADS) {               // the same operations on the same operands: the same `sm`
                const float sm = store_blend(p.wa, old[e], p.wb, store_div_rn(f[e], nf));
                cur[e] = store_div_rn(sm, ns);
            }
        }
        old = cur;
    }
    if (old == held)
        for (int e = tid; e < p.E; e += STORE_THREADS) row0[e] = held[e];
}

#pragma clang fp contract(fast)
