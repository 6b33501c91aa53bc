// The cost matrices of the association rounds of many sequences in one launch (include/busca_rounds.h; float64, no contraction).  The arithmetic is
// kstore_round_cost_tile of kalman_store_kernel.hip.inc, included by the unit before this file - the tile body busca_track_round_cost runs; only
// the addressing is new here: a table of problems over one slot list and one detection table, and a padded [batch, N, M] slab for the solver.
//
//  rounds_cost_kernel : grid (ceil(M / PW_TB), ceil(N / PW_TA), batch), 256 lanes.  Workgroup (x, y, k) reads row k of the table and serves tile
//      (y, x) of problem k, if that tile lies inside (n_k, m_k); what lies outside is not written.  A row the table should not hold - a negative entry,
//      a range that leaves the slot list or the detections, n_k > N, m_k > M - skips its problem.  Both exits are taken by the whole workgroup, before
//      the tile's barrier.

struct RoundsCost {
    const double* mean;         // [S,8]
    const double* cov;          // [S,8,8]
    const int* slot;            // [n_total]
    const double* det_tlbr;     // [m_total,4]
    const double* det_xyah;     // [m_total,4] or NULL (no motion flag)
    const double* det_score;    // [m_total] or NULL
    const int* problems;        // [batch,4]: slot_begin, n_k, det_begin, m_k
    double* out;                // [batch,N,M]
    int* status;                // [n_total] or NULL
    double lambda;
    int S, n_total, m_total, N, M, flags;
};

__global__ void __launch_bounds__(256) rounds_cost_kernel(RoundsCost r) {
    const int* p = r.problems + (size_t)blockIdx.z * 4;
    const int slot_begin = p[0], n_k = p[1], det_begin = p[2], m_k = p[3];
    if (slot_begin < 0 || n_k < 0 || det_begin < 0 || m_k < 0 || n_k > r.N || m_k > r.M || (long long)slot_begin + n_k > r.n_total ||
        (long long)det_begin + m_k > r.m_total)
        return;                                                    // uniform over the workgroup: the table row is the block's
    const long long a0 = (long long)blockIdx.y * PW_TA, b0 = (long long)blockIdx.x * PW_TB;
    if (a0 >= n_k || b0 >= m_k) return;                            // padding of the slab (uniform too)
    const KStore k{(double*)r.mean, (double*)r.cov, r.slot + slot_begin, r.S, n_k};
    kstore_round_cost_tile(k, r.det_tlbr + (size_t)det_begin * 4, r.det_xyah != nullptr ? r.det_xyah + (size_t)det_begin * 4 : nullptr,
                           r.det_score != nullptr ? r.det_score + det_begin : nullptr, m_k, r.flags, r.lambda,
                           r.out + (size_t)blockIdx.z * (size_t)r.N * (size_t)r.M, (size_t)r.M, r.status != nullptr ? r.status + slot_begin : nullptr,
                           (int)a0, (int)b0);
}
