// The bodies of ghost_distance_kernel<MEDIAN> and ghost_thresholds_kernel (ghost_kernel.hip.inc) as device functions: ghost_kernel.hip.inc includes
// this file inside its contract(off) region, after appear_kernel.hip.inc, and wraps each in its kernel; mgframe_kernel.hip.inc (libbusca_mgframe.so)
// calls the same functions per problem of a batch.  One text behind two addressings: what a workgroup computes for one (track, 64-detection tile)
// and for one problem's two groups of rows does not depend on where the operands were found.

#define GHOST_SEL_CHUNK 8       // rows a lane ranks at a time: one LDS read of row j serves this many comparisons

// One (track, 64-detection tile) of busca_ghost_distance by the whole workgroup of 64 * APPEAR_WAVES lanes -> this lane's reduced distance (lane
// (a, b) of wave w holds column col = 16 w + a; the lanes b = 0 write).  `base`: the track's [budget, E] rows of which the first `cnt` (clamped to
// 0 .. budget by the caller) are valid; `brow`: this lane's detection row, or nullptr past the last detection.  MEDIAN stages in `lds`
// ([budget + 2][64] float64) and passes two workgroup barriers: cnt is the workgroup's, so every wave takes the same path.
template <bool MEDIAN>
__device__ __forceinline__ double ghost_distance_entry(const float* base, int cnt, int budget, const float* brow, int E, int reduce, double* lds, int col,
                                                       int a, int b) {
    const double inf = __builtin_huge_val();
    double mn = inf, mx = -inf, sum = 0.0, nb = 0.0;
    ap_f64x4 dot, ga, gb;
    for (int t0 = 0; t0 < cnt; t0 += 16) {                                // the loop of appear_kernel<true>, rows beyond the count never loaded
        const float* arow = t0 + a < cnt ? base + (size_t)(t0 + a) * E : nullptr;
        if (t0 == 0) {
            appear_tile<true>(arow, brow, E, b, dot, ga, gb);
            nb = __shfl(appear_diag(gb, a), a + 16 * (a & 3));
        } else {
            appear_tile<false>(arow, brow, E, b, dot, ga, gb);
        }
        const double da = appear_diag(ga, a);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = b + 4 * r;
            const double na = __shfl(da, row + 16 * b);
            const double c = appear_dist(dot[r], na, nb, 0);
            if (t0 + row < cnt) {
                mn = appear_fold(mn, c, BUSCA_APPEAR_MIN);
                mx = appear_fold(mx, c, BUSCA_APPEAR_MAX);
                sum = appear_fold(sum, c, BUSCA_APPEAR_MEAN);
                if (MEDIAN) lds[(size_t)(t0 + row) * APPEAR_TILE_M + col] = c;
            }
        }
    }
    mn = appear_fold(mn, __shfl_xor(mn, 16), BUSCA_APPEAR_MIN);
    mn = appear_fold(mn, __shfl_xor(mn, 32), BUSCA_APPEAR_MIN);
    mx = appear_fold(mx, __shfl_xor(mx, 16), BUSCA_APPEAR_MAX);
    mx = appear_fold(mx, __shfl_xor(mx, 32), BUSCA_APPEAR_MAX);
    sum = appear_fold(sum, __shfl_xor(sum, 16), BUSCA_APPEAR_MEAN);
    sum = appear_fold(sum, __shfl_xor(sum, 32), BUSCA_APPEAR_MEAN);
    double res;
    if (cnt == 0) res = inf;
    else if (reduce == BUSCA_GHOST_MIN) res = mn;
    else if (reduce == BUSCA_GHOST_MAX) res = mx;
    else if (reduce == BUSCA_GHOST_MEAN) res = sum / (double)cnt;
    else res = (mx + mn) / 2.0;                                           // MIDRANGE; a NaN among the distances is in both
    if constexpr (MEDIAN) {
        double* sel = lds + (size_t)budget * APPEAR_TILE_M;               // [2][64]: the rows of rank (cnt - 1) / 2 and cnt / 2
        __syncthreads();                                                   // cnt is the workgroup's: every wave takes the same path
        if (cnt > 0 && mn == mn) {                                        // no NaN in this column (mn keeps one): the order is total
            const int klo = (cnt - 1) >> 1, khi = cnt >> 1;
            const double* v = lds + col;
            for (int i0 = b; i0 < cnt; i0 += 4 * GHOST_SEL_CHUNK) {
                double vi[GHOST_SEL_CHUNK];
                int rank[GHOST_SEL_CHUNK];
#pragma unroll
                for (int u = 0; u < GHOST_SEL_CHUNK; ++u) {
                    const int i = i0 + 4 * u;
                    vi[u] = i < cnt ? v[(size_t)i * APPEAR_TILE_M] : inf;
                    rank[u] = 0;
                }
                for (int jr = 0; jr < cnt; ++jr) {
                    const double vj = v[(size_t)jr * APPEAR_TILE_M];
#pragma unroll
                    for (int u = 0; u < GHOST_SEL_CHUNK; ++u)
                        rank[u] += (vj < vi[u] || (vj == vi[u] && jr < i0 + 4 * u)) ? 1 : 0;
                }
#pragma unroll
                for (int u = 0; u < GHOST_SEL_CHUNK; ++u) {
                    if (i0 + 4 * u < cnt) {
                        if (rank[u] == klo) sel[col] = vi[u];
                        if (rank[u] == khi) sel[APPEAR_TILE_M + col] = vi[u];
                    }
                }
            }
        }
        __syncthreads();
        if (cnt > 0) res = mn != mn ? mn : (cnt & 1) ? sel[col] : (sel[col] + sel[APPEAR_TILE_M + col]) / 2.0;
    }
    return res;
}

// ---- thresholds --------------------------------------------------------------------------------------------------------------------
#define GHOST_THR_THREADS 256

// the sum of f(x[k]) over k = 0 .. len-1: thread t adds k = t, t + 256, ... in ascending order, the 64 lanes of a wave are added by xor-shuffles
// (offsets 32, 16, 8, 4, 2, 1), the four waves as (w0 + w1) + (w2 + w3).  Every thread returns the total.  PADDED: entry k is entry k of a
// [len / m, m] block in row-major order whose rows lie `ld` apart - the same entries in the same order, found elsewhere.
template <bool SQDEV, bool PADDED>
__device__ __forceinline__ double ghost_block_sum(const double* x, long long len, int m, int ld, double mean, double* part) {
    double acc = 0.0;
    for (long long k = threadIdx.x; k < len; k += GHOST_THR_THREADS) {
        const double v = PADDED ? x[(k / m) * ld + k % m] : x[k];
        if (SQDEV) { const double d = v - mean; acc = acc + d * d; }
        else acc = acc + v;
    }
    for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
    __syncthreads();                                                       // the previous sum's readers are done with `part`
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// busca_ghost_thresholds by one workgroup of GHOST_THR_THREADS lanes: group 0 (the active rows) starts at x_act and holds len_act entries, group 1
// at x_inact with len_inact.  `which`: bit 0 computes thr[0], bit 1 thr[1]; a group without entries leaves its threshold what it was.  Every
// lane passes the same barriers: the lengths and `which` are the workgroup's.
template <bool PADDED>
__device__ __forceinline__ void ghost_thresholds_groups(const double* x_act, long long len_act, const double* x_inact, long long len_inact, int m, int ld,
                                                        double k_act, double k_inact, int which, double* thr, double* part) {
    for (int g = 0; g < 2; ++g) {
        const double* x = g == 0 ? x_act : x_inact;
        const long long len = g == 0 ? len_act : len_inact;
        if (len == 0 || !(which & (1 << g))) continue;                    // no row of this kind: its threshold stays what it was
        const double mean = ghost_block_sum<false, PADDED>(x, len, m, ld, 0.0, part) / (double)len;
        const double var = ghost_block_sum<true, PADDED>(x, len, m, ld, mean, part) / (double)len;
        const double kstd = (g == 0 ? k_act : k_inact) * sqrt(var);
        if (threadIdx.x == 0) thr[g] = mean - kstd;
    }
}
