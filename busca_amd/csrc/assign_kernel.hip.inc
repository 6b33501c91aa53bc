// Linear assignment of an association round (include/busca_assign.h): matching.linear_assignment, adapters/ByteTrack/yolox/tracker/matching.py:39-50
// (lap.lapjv with cost_limit), and the solver of min_cost_matching, adapters/StrongSORT/deep_sort/linear_assignment.py:59-85.
//
// The reduced problem: row i may take column j at w_ij = c_ij - limit when c_ij < limit (NaN and +inf never pass that test), and any row may go to
// one sink of unbounded capacity at cost 0 (= stay unmatched).  Minimise the sum of w over the matching.
//
// assign_kernel: one workgroup per problem - one wave up to ASSIGN_ONE_WAVE_COLS columns (no exchange, no barrier to wait at), four waves beyond -, shortest augmenting paths with potentials (Hungarian / Jonker-Volgenant), float64.
//   Invariants: u_i + v_j <= w_ij on admissible pairs, equality on matched pairs, u_i <= 0 (the sink's potential is 0), v_j <= 0 and v_j = 0 on a free column.
//   Stage `cur` (one per row, at most n): Dijkstra from row cur over the columns.  u_cur starts at 0, so the first scan may see negative reduced costs -
//   harmless, every later edge is non-negative and the first column taken is the cheapest.  Scanning row i at distance d relaxes shortest[j] over the
//   unscanned columns (every thread its own columns, j = tid, tid + threads, ...) and offers the sink at d - u_i.  The workgroup reduces to the
//   nearest unscanned column (a DPP reduction inside the wave - row shifts, then the two row broadcasts, the result read from lane 63 - then, with four
//   waves, one LDS exchange; ties to the lowest column index; the column's matched row travels with it).  The path ends at the sink when the sink is no
//   farther than that column, or at that column when it is free; otherwise the column joins the tree and its row is scanned next: at most m + 1 scans.
//   Then the potentials move (u_i += D - d_i over the tree's rows, v_j -= D - shortest_j over its columns, D = the path's length), and thread 0 flips
//   the path: at most n links.  A row that the path sends to the sink ends at u = 0 and is never looked at again.
//   Every loop is a counted loop; a problem that runs one out (only non-finite arithmetic can) writes status 1 and -1 everywhere and returns.
//   All the solver's state is in LDS (dynamic): u, v, shortest (f64), path, row4col, col4row, the scan stamps (i32), the exchange slots; with STAGED
//   also the n_k x m_k cost matrix, read once, coalesced.  The two flavours run the same arithmetic in the same order: identical results.

#define ASSIGN_WAVES 4                  // waves of the wide flavour (the exchange slots are sized for it)
#define ASSIGN_ONE_WAVE_COLS 256        // up to here one wave scans the row, at most 4 columns per lane
#define ASSIGN_STAGE_DEPTH 16           // global loads a lane keeps in flight while the matrix is staged

// bytes of LDS besides the staged matrix: 2 f64 per column / 1 per row / 2 x ASSIGN_WAVES exchange slots, 3 + 1 i32 likewise and two sets of slots
__host__ __device__ static inline size_t assign_state_bytes(int n, int m) {
    return (size_t)8 * (2 * (size_t)m + n + 2 * ASSIGN_WAVES) + (((size_t)4 * (3 * (size_t)m + n + 4 * ASSIGN_WAVES) + 7) & ~(size_t)7);
}

struct AssignArgs {
    const double* cost; const int* dims; int n, m; double limit;
    int* row_to_col; int* col_to_row; double* duals; double* objective; int* status;
};

// the smaller of two (distance, column, the column's row) candidates; equal distances: the lower column.  column < 0: no candidate.
__device__ __forceinline__ void assign_min(double& v, int& j, int& r, double v2, int j2, int r2) {
    if (j2 >= 0 && (j < 0 || v2 < v || (v2 == v && j2 < j))) { v = v2; j = j2; r = r2; }
}

// one step of the wave reduction: every lane takes the candidate of the lane DPP control CTRL names (lanes without a source, or outside ROW_MASK, see their own)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void assign_dpp_min(double& v, int& j, int& r) {
    const int hi = __double2hiint(v), lo = __double2loint(v);
    const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int oj = __builtin_amdgcn_update_dpp(j, j, CTRL, ROW_MASK, 0xf, false);
    const int orow = __builtin_amdgcn_update_dpp(r, r, CTRL, ROW_MASK, 0xf, false);
    assign_min(v, j, r, __hiloint2double(ohi, olo), oj, orow);
}

// the wave's best candidate, in every lane: row_shr 1 / 2 / 4 / 8 gather a row of 16 lanes in its last lane, row_bcast 15 and 31 carry that across the
// rows into lane 63
__device__ __forceinline__ void assign_wave_min(double& v, int& j, int& r) {
    assign_dpp_min<0x111, 0xf>(v, j, r);
    assign_dpp_min<0x112, 0xf>(v, j, r);
    assign_dpp_min<0x114, 0xf>(v, j, r);
    assign_dpp_min<0x118, 0xf>(v, j, r);
    assign_dpp_min<0x142, 0xa>(v, j, r);
    assign_dpp_min<0x143, 0xc>(v, j, r);
    v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
    j = __builtin_amdgcn_readlane(j, 63);
    r = __builtin_amdgcn_readlane(r, 63);
}

template <bool STAGED, int NW>
__global__ void __launch_bounds__(NW * 64) assign_kernel(AssignArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double assign_lds[];
    constexpr int ASSIGN_THREADS = NW * 64;
    const int tid = threadIdx.x, k = blockIdx.x, n = a.n, m = a.m;
    int nk = n, mk = m;
    bool bad = false;
    if (a.dims != nullptr) {
        nk = a.dims[2 * k];
        mk = a.dims[2 * k + 1];
        if (nk < 0 || nk > n || mk < 0 || mk > m) { bad = true; nk = 0; mk = 0; }
    }
    const double* gcost = a.cost + (size_t)k * n * m;
    int* r2c = a.row_to_col + (size_t)k * n;
    int* c2r = a.col_to_row != nullptr ? a.col_to_row + (size_t)k * m : nullptr;
    double* du = a.duals != nullptr ? a.duals + (size_t)k * (n + m) : nullptr;

    // LDS carve-up (sized for the padded n x m by the host)
    double* v = assign_lds;                      // [m] column potentials
    double* shortest = v + m;                    // [m] tentative distances of this stage
    double* u = shortest + m;                    // [n] row potentials
    double* red_v = u + n;                       // [2][ASSIGN_WAVES]
    int* path = (int*)(red_v + 2 * ASSIGN_WAVES);    // [m] the row a column was reached from
    int* row4col = path + m;                     // [m]
    int* stamp = row4col + m;                    // [m] stage + 1 in which the column joined the tree
    int* col4row = stamp + m;                    // [n]
    int* red_j = col4row + n;                    // [2][ASSIGN_WAVES]
    int* red_r = red_j + 2 * ASSIGN_WAVES;       // [2][ASSIGN_WAVES]
    const double* lcost = assign_lds + (assign_state_bytes(n, m) >> 3);       // STAGED: [nk][mk]

    for (int j = tid; j < mk; j += ASSIGN_THREADS) { v[j] = 0.0; row4col[j] = -1; stamp[j] = 0; path[j] = -1; }
    for (int i = tid; i < nk; i += ASSIGN_THREADS) { u[i] = 0.0; col4row[i] = -1; }
    if (STAGED) {
        double* w = assign_lds + (assign_state_bytes(n, m) >> 3);
        // ASSIGN_STAGE_DEPTH loads in flight per lane: one load per trip would pay the memory latency n m / threads times over
        const int total = nk * mk;
        for (int e0 = tid; e0 < total; e0 += ASSIGN_STAGE_DEPTH * ASSIGN_THREADS) {
            double t[ASSIGN_STAGE_DEPTH];
#pragma unroll
            for (int q = 0; q < ASSIGN_STAGE_DEPTH; ++q) {
                const int e = e0 + q * ASSIGN_THREADS;
                t[q] = e < total ? gcost[(size_t)(e / mk) * m + e % mk] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < ASSIGN_STAGE_DEPTH; ++q) {
                const int e = e0 + q * ASSIGN_THREADS;
                if (e < total) w[e] = t[q];
            }
        }
    }
    __syncthreads();

    const double limit = a.limit;
    const double INF = __builtin_inf();
    bool failed = bad;
    unsigned parity = 0;
    for (int cur = 0; cur < nk && !failed; ++cur) {
        for (int j = tid; j < mk; j += ASSIGN_THREADS) shortest[j] = INF;      // own columns only: no barrier needed before the scan
        int i = cur;
        double ui = 0.0, dist = 0.0;               // the row being scanned, its potential and its distance
        double sink_dist = 0.0;                    // row cur may stay unmatched at 0 (u_cur = 0 here)
        int sink_row = cur, end_col = -1;
        bool done = false;
        for (int step = 0; step <= mk; ++step) {
            if (step > 0) {
                const double cand = dist - ui;
                if (cand < sink_dist) { sink_dist = cand; sink_row = i; }
            }
            double best = INF;
            int bj = -1, br = -1;
            const double* crow = STAGED ? lcost + i * mk : gcost + (size_t)i * m;
            for (int j = tid; j < mk; j += ASSIGN_THREADS) {
                if (stamp[j] == cur + 1) continue;
                const double c = crow[j];
                const int rj = row4col[j];
                double s = shortest[j];
                if (c < limit) {
                    const double r = (dist + ((c - limit) - ui)) - v[j];
                    if (r < s) { s = r; shortest[j] = r; path[j] = i; }
                }
                if (s < best) { best = s; bj = j; br = rj; }          // ascending j: the lowest column of equal distances stays
            }
            assign_wave_min(best, bj, br);
            double lowest = best;
            int jmin = bj, r4 = br;
            if (NW > 1) {
                if ((tid & 63) == 0) { red_v[parity * ASSIGN_WAVES + (tid >> 6)] = best; red_j[parity * ASSIGN_WAVES + (tid >> 6)] = bj; red_r[parity * ASSIGN_WAVES + (tid >> 6)] = br; }
                __syncthreads();
                lowest = red_v[parity * ASSIGN_WAVES];
                jmin = red_j[parity * ASSIGN_WAVES];
                r4 = red_r[parity * ASSIGN_WAVES];
#pragma unroll
                for (int w = 1; w < NW; ++w)
                    assign_min(lowest, jmin, r4, red_v[parity * ASSIGN_WAVES + w], red_j[parity * ASSIGN_WAVES + w], red_r[parity * ASSIGN_WAVES + w]);
                parity ^= 1u;
            }
            if (jmin < 0 || !(lowest < sink_dist)) { dist = sink_dist; done = true; break; }      // the sink is no farther: the path ends there
            dist = lowest;
            if ((jmin % ASSIGN_THREADS) == tid) stamp[jmin] = cur + 1;
            if (r4 < 0) { end_col = jmin; done = true; break; }                                   // a free column
            i = r4;
            ui = u[i];
        }
        if (!done || !(dist == dist) || dist == INF || dist == -INF) { failed = true; break; }     // the same in every thread
        // potentials: the tree's matched columns and their rows (row4col is still the old matching)
        for (int j = tid; j < mk; j += ASSIGN_THREADS) {
            if (stamp[j] != cur + 1) continue;
            const int r = row4col[j];
            if (r < 0) continue;                   // the free column the path ends at: shortest == dist, nothing moves
            const double d = dist - shortest[j];
            u[r] = u[r] + d;
            v[j] = v[j] - d;
        }
        __syncthreads();
        if (tid == 0) {
            u[cur] = dist;
            int j = end_col;
            bool flip = true;
            if (end_col < 0) {                     // row sink_row leaves its column and stays unmatched at potential 0
                u[sink_row] = 0.0;
                if (sink_row == cur) flip = false;
                else { j = col4row[sink_row]; col4row[sink_row] = -1; }
            }
            for (int links = 0; flip && links <= nk; ++links) {
                const int r = path[j];
                row4col[j] = r;
                const int jn = col4row[r];
                col4row[r] = j;
                if (r == cur) break;
                j = jn;
            }
        }
        __syncthreads();
    }

    // ---- results ----
    double part = 0.0;
    for (int i = tid; i < n; i += ASSIGN_THREADS) {
        const int j = (i < nk && !failed) ? col4row[i] : -1;
        r2c[i] = j;
        if (j >= 0) part = part + (STAGED ? lcost[i * mk + j] : gcost[(size_t)i * m + j]);
        if (du != nullptr) du[i] = (i < nk && !failed) ? u[i] : 0.0;
    }
    for (int j = tid; j < m; j += ASSIGN_THREADS) {
        if (c2r != nullptr) c2r[j] = (j < mk && !failed) ? row4col[j] : -1;
        if (du != nullptr) du[n + j] = (j < mk && !failed) ? v[j] : 0.0;
    }
    if (a.objective != nullptr) {                  // a fixed summation order: rows tid, tid + threads, ... per thread, then the butterfly, then the waves in order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part = part + __shfl_xor(part, off, 64);
        __syncthreads();
        if ((tid & 63) == 0) red_v[tid >> 6] = part;
        __syncthreads();
        if (tid == 0) {
            double s = red_v[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) s = s + red_v[w];
            a.objective[k] = failed ? __builtin_nan("") : s;
        }
    }
    if (tid == 0 && a.status != nullptr) a.status[k] = failed ? 1 : 0;
}
