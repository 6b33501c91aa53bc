// Staged linear assignment (include/busca_assign_stages.h): a chain of assignment problems over one set of rows and columns in ONE launch - the levels
// of matching_cascade (adapters/StrongSORT/deep_sort/linear_assignment.py:88-162) followed by the IoU stage of Tracker._match (deep_sort/tracker.py:
// 238-248).  Included after assign_kernel.hip.inc, whose candidate reduction (assign_min / assign_wave_min) and LDS state it shares.
//
// assign_stages_kernel: one workgroup per problem, the flavours of assign_kernel (one wave up to ASSIGN_ONE_WAVE_COLS columns, four beyond; costs
// staged in LDS or read from global memory).  Stage s solves, with that stage's limit on that stage's plane, the problem of its member
// rows (first == s, or again == s and still unmatched) against the columns no earlier stage matched - by the very augmentation of assign_kernel run
// on the FULL index space with a mask:
//   - only member rows are started from, in ascending order - the row order of the compacted matrix;
//   - a column matched in an earlier stage carries a negative scan stamp, -(stage + 1), and is skipped by every scan, so neither it nor its row (which
//     could only be reached through it) is ever touched again; a column's stamp is otherwise the number of the augmentation in which it joined the
//     tree, counted over the whole launch, so the stamps need no clearing between stages;
//   - u and v are cleared when a populated stage begins; col4row / row4col of earlier matches persist.
// Every number the augmentation computes is a function of admissible entries of member rows and free columns and of potentials that start at 0: the
// same operands in the same order as the compacted solve.  Every choice between candidates is "smallest distance, then lowest column", which does not
// depend on how the columns are dealt to lanes, and dropping columns keeps their order.  So each stage chooses the very pairs busca_linear_assignment
// chooses on the compacted matrix - the same matching, not merely one of equal cost (DESIGN K-STAGES).
// A histogram of first / again over the stages (one pass over the rows) tells an empty stage before anything is cleared or scanned: a cascade of 30
// levels of which 3 hold tracks costs 3 solves.  The stage loop also ends once every column is matched.
// Staging (STAGED): what a stage reads is the rows of its members only, so that is what is copied into LDS when the stage begins - members x m_k
// doubles, member q (in ascending row order: slotrow / rowslot, listed by the first wave with a ballot per 64 rows) at row q - if it fits what the
// workgroup has left of its 160 KiB (stage_cap); a stage whose member rows do not fit reads global memory.  A cascade level of a 150 x 150 frame
// holds a handful of rows and is staged although the plane itself would not fit.  Both ways run the same arithmetic in the same order.

#define ASSIGN_STAGES_MAX 128           // BUSCA_ASSIGN_STAGES_MAX

struct AssignStageRec { int plane; int reserved; double limit; };      // one record of the stage table, 16 bytes

// bytes of LDS besides the staged rows: the solver's state and, per row, the two stage words and the two slot maps, the histogram, two member counters
__host__ __device__ static inline size_t assign_stages_state_bytes(int n, int m) {
    return assign_state_bytes(n, m) + (((size_t)4 * (4 * (size_t)n + ASSIGN_STAGES_MAX + 2) + 7) & ~(size_t)7);
}

struct AssignStagesArgs {
    const double* cost; const int* dims; int planes, n, m;
    unsigned stage_cap;                            // doubles of LDS behind the state for the member rows of a stage (STAGED)
    const AssignStageRec* stages; int n_stages; const int* first; const int* again;
    int* row_to_col; int* col_to_row; int* row_stage; int* status;
};

template <bool STAGED, int NW>
__global__ void __launch_bounds__(NW * 64) assign_stages_kernel(AssignStagesArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double assign_lds[];
    constexpr int ASSIGN_THREADS = NW * 64;
    const int tid = threadIdx.x, k = blockIdx.x, n = a.n, m = a.m, S = a.n_stages;
    int nk = n, mk = m;
    int fault = 0;                                 // the status word: 1 = sizes outside the slab or a loop bound, 2 = a plane outside the slab
    if (a.dims != nullptr) {
        nk = a.dims[2 * k];
        mk = a.dims[2 * k + 1];
        if (nk < 0 || nk > n || mk < 0 || mk > m) { fault = 1; nk = 0; mk = 0; }
    }
    for (int s = 0; s < S; ++s) {                  // the same in every thread; checked before anything is read through a plane index
        const int p = a.stages[s].plane;
        if (p < 0 || p >= a.planes) fault = 2;
    }
    const double* gcost = a.cost + (size_t)k * a.planes * n * m;
    int* r2c = a.row_to_col + (size_t)k * n;
    int* c2r = a.col_to_row != nullptr ? a.col_to_row + (size_t)k * m : nullptr;
    int* rst = a.row_stage != nullptr ? a.row_stage + (size_t)k * n : nullptr;

    // LDS carve-up (sized for the padded n x m by the host): assign_kernel's, then the stage words
    double* v = assign_lds;                      // [m] column potentials
    double* shortest = v + m;                    // [m] tentative distances of this augmentation
    double* u = shortest + m;                    // [n] row potentials
    double* red_v = u + n;                       // [2][ASSIGN_WAVES]
    int* path = (int*)(red_v + 2 * ASSIGN_WAVES);    // [m] the row a column was reached from
    int* row4col = path + m;                     // [m]
    int* stamp = row4col + m;                    // [m] > 0: the augmentation in which the column joined the tree; < 0: taken in stage -stamp - 1
    int* col4row = stamp + m;                    // [n]
    int* red_j = col4row + n;                    // [2][ASSIGN_WAVES]
    int* red_r = red_j + 2 * ASSIGN_WAVES;       // [2][ASSIGN_WAVES]
    int* first = (int*)(assign_lds + (assign_state_bytes(n, m) >> 3));      // [n] the stage a row takes part in, or -1
    int* again = first + n;                      // [n] the stage it takes part in once more if still unmatched, or -1
    int* count = again + n;                      // [ASSIGN_STAGES_MAX] rows that name the stage
    int* rowslot = count + ASSIGN_STAGES_MAX;    // [n] this stage: the member's slot among the members, -1 for the other rows
    int* slotrow = rowslot + n;                  // [n] this stage: the member at a slot
    int* nmem = slotrow + n;                     // [2] members of this stage (one counter per stage parity)
    double* lcost = assign_lds + (assign_stages_state_bytes(n, m) >> 3);    // STAGED: [members][mk] of this stage's plane

    for (int j = tid; j < mk; j += ASSIGN_THREADS) { v[j] = 0.0; row4col[j] = -1; stamp[j] = 0; path[j] = -1; }
    for (int i = tid; i < nk; i += ASSIGN_THREADS) { u[i] = 0.0; col4row[i] = -1; }
    for (int s = tid; s < S; s += ASSIGN_THREADS) count[s] = 0;
    __syncthreads();
    if (fault == 0) {
        const int* gfirst = a.first + (size_t)k * n;
        const int* gagain = a.again != nullptr ? a.again + (size_t)k * n : nullptr;
        for (int i = tid; i < nk; i += ASSIGN_THREADS) {
            const int f = gfirst[i], g = gagain != nullptr ? gagain[i] : -1;
            const int fs = (f >= 0 && f < S) ? f : -1;
            const int gs = (g >= 0 && g < S && g > f) ? g : -1;
            first[i] = fs;
            again[i] = gs;
            if (fs >= 0) atomicAdd(&count[fs], 1);
            if (gs >= 0) atomicAdd(&count[gs], 1);
        }
    }
    __syncthreads();

    const double INF = __builtin_inf();
    bool failed = fault != 0;
    unsigned parity = 0;
    int tick = 0, matched = 0;
    for (int s = 0; s < S && !failed && matched < mk; ++s) {
        if (count[s] == 0) continue;               // nobody names this stage: nothing is cleared, staged or scanned
        const int plane = a.stages[s].plane;
        const double limit = a.stages[s].limit;
        const double* gplane = gcost + (size_t)plane * n * m;
        for (int j = tid; j < mk; j += ASSIGN_THREADS) v[j] = 0.0;
        for (int i = tid; i < nk; i += ASSIGN_THREADS) u[i] = 0.0;
        if (tid < 64) {                            // the first wave lists the members in ascending order, 64 rows a trip (every augmentation ended at
            int base = 0;                          // a barrier: col4row is what the earlier stages left)
            for (int i0 = 0; i0 < nk; i0 += 64) {
                const int i = i0 + tid;
                const bool member = i < nk && (first[i] == s || (again[i] == s && col4row[i] < 0));
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(member);
                const int slot = base + __popcll(mask & ((1ull << tid) - 1ull));
                if (i < nk) rowslot[i] = member ? slot : -1;
                if (member) slotrow[slot] = i;
                base += __popcll(mask);
            }
            if (tid == 0) nmem[s & 1] = base;
        }
        __syncthreads();
        const int members = nmem[s & 1];           // the same in every thread
        if (members == 0) continue;                // every row that named the stage for a second try was matched meanwhile
        const bool in_lds = STAGED && (size_t)members * mk <= (size_t)a.stage_cap;
        if (in_lds) {                              // nobody reads the rows of the stage before: they are overwritten
            const int total = members * mk;
            for (int e0 = tid; e0 < total; e0 += ASSIGN_STAGE_DEPTH * ASSIGN_THREADS) {
                double t[ASSIGN_STAGE_DEPTH];
#pragma unroll
                for (int q = 0; q < ASSIGN_STAGE_DEPTH; ++q) {
                    const int e = e0 + q * ASSIGN_THREADS;
                    t[q] = e < total ? gplane[(size_t)slotrow[e / mk] * m + e % mk] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < ASSIGN_STAGE_DEPTH; ++q) {
                    const int e = e0 + q * ASSIGN_THREADS;
                    if (e < total) lcost[e] = t[q];
                }
            }
            __syncthreads();
        }
        for (int q = 0; q < members && !failed; ++q) {
            const int cur = slotrow[q];                // ascending: the row order of the compacted matrix (an LDS word behind a barrier: the same in every thread)
            ++tick;
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
                const double* grow = gplane + (size_t)i * m;
                const double* lrow = lcost + (in_lds ? rowslot[i] * mk : 0);   // a row of the tree is a member: its column was matched in this stage
                for (int j = tid; j < mk; j += ASSIGN_THREADS) {
                    const int st = stamp[j];
                    if (st < 0 || st == tick) continue;                    // taken by an earlier stage, or in the tree already
                    double c;
                    if (in_lds) c = lrow[j];
                    else c = grow[j];
                    const int rj = row4col[j];
                    double sh = shortest[j];
                    if (c < limit) {
                        const double r = (dist + ((c - limit) - ui)) - v[j];
                        if (r < sh) { sh = r; shortest[j] = r; path[j] = i; }
                    }
                    if (sh < best) { best = sh; bj = j; br = rj; }        // ascending j: the lowest column of equal distances stays
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
                if ((jmin % ASSIGN_THREADS) == tid) stamp[jmin] = tick;
                if (r4 < 0) { end_col = jmin; done = true; break; }                                   // a free column
                i = r4;
                ui = u[i];
            }
            if (!done || !(dist == dist) || dist == INF || dist == -INF) { failed = true; fault = 1; break; }     // the same in every thread
            // potentials: the tree's matched columns and their rows (row4col is still the old matching)
            for (int j = tid; j < mk; j += ASSIGN_THREADS) {
                if (stamp[j] != tick) continue;
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
            if (end_col >= 0) ++matched;               // a path to the sink moves a column from one row to another: the count stays
            __syncthreads();
        }
        // the stage's matches are final: its columns are withdrawn (own columns only, as the scans read them)
        for (int j = tid; j < mk; j += ASSIGN_THREADS)
            if (stamp[j] >= 0 && row4col[j] >= 0) stamp[j] = -(s + 1);
    }
    __syncthreads();

    // ---- results ----
    for (int i = tid; i < n; i += ASSIGN_THREADS) {
        const int j = (i < nk && !failed) ? col4row[i] : -1;
        r2c[i] = j;
        if (rst != nullptr) rst[i] = j >= 0 ? -stamp[j] - 1 : -1;
    }
    if (c2r != nullptr)
        for (int j = tid; j < m; j += ASSIGN_THREADS) c2r[j] = (j < mk && !failed) ? row4col[j] : -1;
    if (tid == 0 && a.status != nullptr) a.status[k] = fault;
}
