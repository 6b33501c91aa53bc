// The four kernels of a GHOST frame on resident track state (include/busca_gframe.h), around the linear assignment.  The arithmetic is included
// text: ghost_motion_warp_corner, ghost_motion_step_coord and ghost_motion_append_one of ghost_motion_kernel.hip.inc, pairwise_iou and
// pairwise_iou_cost of pairwise_kernel.hip.inc, ghost_combine_entry of ghost_kernel.hip.inc, store_ring_push and store_ring_copy of
// store_kernel.hip.inc - all included by the unit before this file, and the very functions the kernels of libbusca_hip.so and libbusca_store.so call.
// The body of each kernel is a device function of gframe_body.hip.inc, which mgframe_kernel.hip.inc (libbusca_mgframe.so) calls per problem of a
// batch; the kernels here give it the single frame's addressing (a row of the matrix is that row of the slot list).
//
//  gframe_advance_kernel : one 64-lane workgroup per listed slot: (with a warp) every valid ring row of the slot through the warp, one (row, corner)
//      per lane and round, a barrier, then - for the first n_step slots - the motion step, one coordinate per lane 0 .. 3, which reads the rows
//      the workgroup has just warped.
//  gframe_cost_kernel    : the final [n, m] cost.  A PW_TA x PW_TB (16 x 64) tile per 256-lane workgroup, as pairwise_kernel and frame_cost_kernel:
//      the 16 positions and 64 detection boxes staged once in LDS, every lane the four rows of one column: the appearance entry, the class mask,
//      the blend with 1 - IoU, the threshold.  A lane reads and writes its own entries only, so `out` may be `app`.
//  gframe_keep_kernel    : one thread per row of the range and per column: the strict threshold test of the matched pair, read from both match
//      vectors of the solver - the row's thread writes track_det, the column's thread det_track and, with a mask, the NaN of that column in the
//      rows from mask_from on.  Both threads evaluate the same comparison on the same entry; no atomics.
//  gframe_apply_kernel   : n + m workgroups of 64 lanes (one wave).  Workgroup i < n: Track.add_detection of slot[i] with the detection it was
//      assigned.  Workgroup n + j: Track.__init__ of detection j into a free slot, when j was not assigned and may start a track; its rank among
//      such columns is counted by the workgroup itself over the columns below j.  Lane 0 does the bookkeeping of both rings and broadcasts the
//      feature row by a shuffle; the 64 lanes copy the feature.  Both decisions are uniform over the workgroup.
//
// No multiply-add contraction anywhere in this file (the files included before it leave the file-scope mode at `fast`).
#pragma clang fp contract(off)

#include "gframe_body.hip.inc"

struct GFrameAdvance {
    GhostMotionRings r;
    const int* slot;            // [n]
    const float* warp;          // dev [6] or nullptr
    double* out;                // [n_step, 4]
    int n, n_step, num_active, last_n, diff32;
};

__global__ void __launch_bounds__(64) gframe_advance_kernel(GFrameAdvance p) {
    const int i = blockIdx.x;
    if (i >= p.n) return;
    gframe_advance_slot(p.r, p.slot[i], p.warp, i < p.n_step, i < p.num_active, p.last_n, p.diff32, p.out + (size_t)i * 4, threadIdx.x);
}

__global__ void __launch_bounds__(256) gframe_cost_kernel(GFrameCost p) {
    __shared__ double sa[PW_TA][4];
    __shared__ double sb[PW_TB][4];
    gframe_cost_tile(p, blockIdx.y * PW_TA, blockIdx.x * PW_TB, sa, sb, threadIdx.x);
}

__global__ void __launch_bounds__(256) gframe_keep_kernel(GFrameKeep p) {
    gframe_keep_thread(p, (long long)blockIdx.x * 256 + threadIdx.x);
}

// `n`: the rows of the matrix (f.rows maps row i < n to list row i)
__global__ void __launch_bounds__(64) gframe_apply_kernel(GFrameApply f, int n) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < n) {                                                   // a row: the track's own detection
        gframe_apply_row(f, b, tid);
        return;
    }
    const int j = b - n;
    if (j >= f.m) return;
    gframe_apply_col(f, j, tid);
}

#pragma clang fp contract(fast)
