// Appearance cost (include/busca_appearance.h): out[i, j] = reduce over the valid gallery rows g of track i of
//   1 - <g, d_j> / sqrt(<g, g> * <d_j, d_j>)
// in float64 on v_mfma_f64_16x16x4_f64, operands converted from f32 in registers.
//
// One wave owns a 16-row x 16-detection tile.  Lane (a = lane & 15, b = lane >> 4) loads four consecutive k of gallery row a and of
// detection a as one 16-byte load each (k = 16 s + 4 b .. + 3) and feeds four matrix instructions with them: instruction t takes element t of
// both loads, so both operands see the same k permutation (A: lane (a, b) = G[row a][k b], B: lane (a, b) = D[k b][col a]).  The squared norms
// are the diagonals of G G^T and D D^T, computed by the same instruction on the same registers (A = B = the row's values): a norm is then the
// very sum a dot product of the vector with itself would be, and identical vectors come out at distance exactly 0.
// C/D map of the f64 instruction: lane (a, b), register r = element [row b + 4 r][col a] (NOT the f32 map).  The diagonal element of row x sits
// in lane (a = x, b = x & 3), register x >> 2.
//
// Two flavours of one kernel, four waves (64 detections) per workgroup, 1-D grid:
//   plain   (GALLERY = false)  workgroup = 16 tracks x 64 detections; row i of the matrix is gallery row i
//   gallery (GALLERY = true)   workgroup = (track, 64 detections); the track's valid rows 16 at a time, rows beyond the count are masked: never
//                              loaded (their operand is 0) and never reduced.  The running min / max / sum lives in registers: over the lane's four
//                              rows of every tile, then across the four row groups b with two xor-shuffles.
// No LDS, no workspace, no atomics; every sum in the order the header states.  No multiply-add contraction: the epilogue is written out.
#pragma clang fp contract(off)

typedef double ap_f64x4 __attribute__((ext_vector_type(4)));

#define APPEAR_WAVES 4
#define APPEAR_TILE_M (16 * APPEAR_WAVES)

struct AppearArgs {
    const float* gallery; const int* slot; const int* count; const float* dets; double* out;
    int n, budget, m, E, reduce, clamp, mt;        // mt = detection tiles per row of workgroups
};

// four consecutive k of this lane's row at step `step` (k = 16 step + 4 b); a masked row (nullptr) reads nothing and gives zeros
__device__ __forceinline__ float4 appear_load(const float* __restrict__ row, int step, int b) {
    return row ? *reinterpret_cast<const float4*>(row + 16 * step + 4 * b) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <bool WITH_B>
__device__ __forceinline__ void appear_step(const float4& av, const float4& bv, ap_f64x4& dot, ap_f64x4& ga, ap_f64x4& gb) {
    const double x[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
    const double y[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dot = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t], y[t], dot, 0, 0, 0);
        ga = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t], x[t], ga, 0, 0, 0);
        if (WITH_B) gb = __builtin_amdgcn_mfma_f64_16x16x4f64(y[t], y[t], gb, 0, 0, 0);
    }
}

// dot = G D^T, ga = G G^T (and with WITH_B gb = D D^T) of one 16 x 16 tile over the whole of E.  `arow` / `brow`: this lane's row, nullptr = a masked row (zeros).
// The steps run in ascending order whatever the chunking: chunks of APPEAR_CHUNK steps whose loads are issued one chunk ahead of the matrix instructions
// that consume them (the last chunk is fetched twice rather than branching), then the E / 16 mod APPEAR_CHUNK steps that are left.
#define APPEAR_CHUNK 4
template <bool WITH_B>
__device__ __forceinline__ void appear_tile(const float* __restrict__ arow, const float* __restrict__ brow, int E, int b, ap_f64x4& dot, ap_f64x4& ga, ap_f64x4& gb) {
    dot = ap_f64x4{0.0, 0.0, 0.0, 0.0};
    ga = dot;
    if (WITH_B) gb = dot;
    const int nsteps = E >> 4, nchunk = nsteps / APPEAR_CHUNK;
    float4 av[APPEAR_CHUNK], bv[APPEAR_CHUNK];
    if (nchunk > 0) {
#pragma unroll
        for (int u = 0; u < APPEAR_CHUNK; ++u) { av[u] = appear_load(arow, u, b); bv[u] = appear_load(brow, u, b); }
    }
    for (int c = 0; c < nchunk; ++c) {
        const int nxt = (c + 1 < nchunk ? c + 1 : c) * APPEAR_CHUNK;
        float4 an[APPEAR_CHUNK], bn[APPEAR_CHUNK];
#pragma unroll
        for (int u = 0; u < APPEAR_CHUNK; ++u) { an[u] = appear_load(arow, nxt + u, b); bn[u] = appear_load(brow, nxt + u, b); }
#pragma unroll
        for (int u = 0; u < APPEAR_CHUNK; ++u) appear_step<WITH_B>(av[u], bv[u], dot, ga, gb);
#pragma unroll
        for (int u = 0; u < APPEAR_CHUNK; ++u) { av[u] = an[u]; bv[u] = bn[u]; }
    }
    for (int s = nchunk * APPEAR_CHUNK; s < nsteps; ++s) appear_step<WITH_B>(appear_load(arow, s, b), appear_load(brow, s, b), dot, ga, gb);
}

// the register of `g` that holds a diagonal element on the lanes that hold one (a >> 2; meaningful where b == (a & 3))
__device__ __forceinline__ double appear_diag(const ap_f64x4& g, int a) {
    const int q = a >> 2;
    return q == 0 ? g[0] : q == 1 ? g[1] : q == 2 ? g[2] : g[3];
}

__device__ __forceinline__ double appear_dist(double dot, double na, double nb, int clamp) {
    double c = 1.0 - dot / sqrt(na * nb);
    if (clamp && c < 0.0) c = 0.0;                  // a NaN stays a NaN, as np.maximum(0, .) leaves it
    return c;
}

// MIN / MAX that keep a NaN once they have seen one (numpy's min / max); MEAN adds
__device__ __forceinline__ double appear_fold(double acc, double c, int reduce) {
    if (reduce == BUSCA_APPEAR_MEAN) return acc + c;
    if (acc != acc) return acc;
    if (c != c) return c;
    if (reduce == BUSCA_APPEAR_MIN) return c < acc ? c : acc;
    return c > acc ? c : acc;
}

template <bool GALLERY>
__global__ void __launch_bounds__(64 * APPEAR_WAVES) appear_kernel(AppearArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, b = lane >> 4;
    const int tm = blockIdx.x % p.mt, ti = blockIdx.x / p.mt;
    const int j = tm * APPEAR_TILE_M + wave * 16 + a;                     // this lane's detection: its B row and its output column
    const float* brow = j < p.m ? p.dets + (size_t)j * p.E : nullptr;
    ap_f64x4 dot, ga, gb;
    if constexpr (!GALLERY) {
        const int i0 = ti * 16;
        const float* arow = i0 + a < p.n ? p.gallery + (size_t)(i0 + a) * p.E : nullptr;
        appear_tile<true>(arow, brow, p.E, b, dot, ga, gb);
        const double da = appear_diag(ga, a), db = appear_diag(gb, a);
        const double nb = __shfl(db, a + 16 * (a & 3));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = b + 4 * r;
            const double na = __shfl(da, row + 16 * b);                     // row & 3 == b
            const double c = appear_dist(dot[r], na, nb, p.clamp);
            if (i0 + row < p.n && j < p.m) p.out[(size_t)(i0 + row) * p.m + j] = c;
        }
    } else {
        const int s = p.slot ? p.slot[ti] : ti;
        int cnt = s < 0 ? 0 : (p.count ? p.count[s] : p.budget);
        cnt = cnt < 0 ? 0 : cnt > p.budget ? p.budget : cnt;
        const double inf = __builtin_huge_val();
        double acc = p.reduce == BUSCA_APPEAR_MIN ? inf : p.reduce == BUSCA_APPEAR_MAX ? -inf : 0.0;
        double nb = 0.0;
        const float* base = p.gallery + (size_t)(s < 0 ? 0 : s) * p.budget * p.E;
        for (int t0 = 0; t0 < cnt; t0 += 16) {
            const float* arow = t0 + a < cnt ? base + (size_t)(t0 + a) * p.E : nullptr;
            if (t0 == 0) {
                appear_tile<true>(arow, brow, p.E, b, dot, ga, gb);
                nb = __shfl(appear_diag(gb, a), a + 16 * (a & 3));
            } else {
                appear_tile<false>(arow, brow, p.E, b, dot, ga, gb);
            }
            const double da = appear_diag(ga, a);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = b + 4 * r;
                const double na = __shfl(da, row + 16 * b);
                const double c = appear_dist(dot[r], na, nb, p.clamp);
                if (t0 + row < cnt) acc = appear_fold(acc, c, p.reduce);
            }
        }
        acc = appear_fold(acc, __shfl_xor(acc, 16), p.reduce);
        acc = appear_fold(acc, __shfl_xor(acc, 32), p.reduce);
        if (cnt == 0) acc = inf;
        else if (p.reduce == BUSCA_APPEAR_MEAN) acc = acc / (double)cnt;
        if (b == 0 && j < p.m) p.out[(size_t)ti * p.m + j] = acc;
    }
}

#pragma clang fp contract(fast)
