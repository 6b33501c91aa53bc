// GHOST's linear motion model (include/busca_ghost_motion.h): per-track rings of past boxes in HBM, the velocity step, the camera warp.  Three kernels:
//
//   ghost_motion_append_kernel  one thread per (slot, detection) pair: pos = box, box and frame pushed onto the ring (one 32-byte row)
//   ghost_motion_warp_kernel    one thread per (listed slot, ring row, corner): W . (x, y, 1) in float64, rounded once to float32
//   ghost_motion_step_kernel    one thread per (track, coordinate): the pair velocities of the window summed sequentially, oldest pair first
//
// A few hundred tracks of four coordinates each: every launch is a handful of waves whose time is the launch and one dependent chain of loads per thread
// (latency-bound; there is no byte or FLOP rate to approach).  The four coordinates of a track are four adjacent lanes, so a ring row is one 32-byte read.
// No multiply-add contraction: every sum, product and quotient is the IEEE operation numpy performs.
// The body of each kernel is a device function (ghost_motion_append_one, ghost_motion_warp_corner, ghost_motion_step_coord) that gframe_kernel.hip.inc
// (libbusca_gframe.so) calls under its own lane mapping: one text behind two addressings.
#pragma clang fp contract(off)

#define GHOST_MOTION_THREADS 256

struct GhostMotionRings {
    double* hist; int* frames; int* count; int* newest; double* pos; double* vel;
    int S, H;
};

// (count, newest) of slot s as the kernels read them: the count clamped to 0 .. H, a newest outside 0 .. H-1 taken as count - 1 (the ring that has not wrapped)
__device__ __forceinline__ void ghost_motion_ring(const GhostMotionRings& r, int s, int& cnt, int& nw) {
    cnt = r.count[s];
    cnt = cnt < 0 ? 0 : cnt > r.H ? r.H : cnt;
    nw = r.newest[s];
    if (nw < 0 || nw >= r.H) nw = cnt - 1;
}

// the ring row of the oldest of the w newest samples: w - 1 rows back from `nw`, modulo H
__device__ __forceinline__ int ghost_motion_oldest(int nw, int w, int H) {
    const int r = (nw - (w - 1)) % H;
    return r < 0 ? r + H : r;
}

struct GhostMotionAppendArgs {
    GhostMotionRings r;
    const int* slot; const int* det; const unsigned char* reset; const double* boxes;
    int k, m, frame;
};

// One (slot, box) pair of busca_ghost_motion_append, by one thread: pos = box, the box and `frame` pushed onto the ring of the valid slot s; `fresh`
// empties the ring and zeroes the velocity first.  ghost_motion_append_kernel and gframe_apply_kernel (gframe_kernel.hip.inc, libbusca_gframe.so) are
// this function behind two addressings.
__device__ __forceinline__ void ghost_motion_append_one(const GhostMotionRings& r, int s, const double* __restrict__ box, int frame, bool fresh) {
    int cnt, nw;
    ghost_motion_ring(r, s, cnt, nw);
    if (fresh) cnt = 0;
    const int row = cnt == 0 ? 0 : (nw + 1) % r.H;
    double* hist = r.hist + ((size_t)s * r.H + row) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = box[c];
        r.pos[(size_t)s * 4 + c] = v;
        hist[c] = v;
        if (fresh) r.vel[(size_t)s * 4 + c] = 0.0;
    }
    r.frames[(size_t)s * r.H + row] = frame;
    r.count[s] = cnt < r.H ? cnt + 1 : r.H;
    r.newest[s] = row;
}

__global__ void __launch_bounds__(GHOST_MOTION_THREADS) ghost_motion_append_kernel(GhostMotionAppendArgs p) {
    const long long i = (long long)blockIdx.x * GHOST_MOTION_THREADS + threadIdx.x;
    if (i >= p.k) return;
    const int s = p.slot[i];
    const int j = p.det ? p.det[i] : (int)i;
    if (s < 0 || s >= p.r.S || j < 0 || j >= p.m) return;
    ghost_motion_append_one(p.r, s, p.boxes + (size_t)j * 4, p.frame, p.reset && p.reset[i]);
}

struct GhostMotionWarpArgs {
    GhostMotionRings r;
    const int* slot;
    int n;
    double w[6];
};

// One corner (0: x1 y1, 1: x2 y2) of ring row `row` of the valid slot s through the warp w[6], when the row holds a sample: the body of
// busca_ghost_motion_warp.  ghost_motion_warp_kernel and gframe_advance_kernel (gframe_kernel.hip.inc) are this function behind two addressings.
__device__ __forceinline__ void ghost_motion_warp_corner(const GhostMotionRings& r, int s, int row, int corner, const double* w) {
    int cnt, nw;
    ghost_motion_ring(r, s, cnt, nw);
    int back = (nw - row) % r.H;                                           // rows back from the newest one
    if (back < 0) back += r.H;
    if (back >= cnt) return;
    double* xy = r.hist + ((size_t)s * r.H + row) * 4 + 2 * corner;
    const double x = xy[0], y = xy[1];
    const double xn = (w[0] * x + w[1] * y) + w[2];
    const double yn = (w[3] * x + w[4] * y) + w[5];
    xy[0] = (double)(float)xn;
    xy[1] = (double)(float)yn;
}

__global__ void __launch_bounds__(GHOST_MOTION_THREADS) ghost_motion_warp_kernel(GhostMotionWarpArgs p) {
    const long long t = (long long)blockIdx.x * GHOST_MOTION_THREADS + threadIdx.x;
    const int corner = (int)(t & 1);
    const long long q = t >> 1;
    const int row = (int)(q % p.r.H);
    const long long i = q / p.r.H;
    if (i >= p.n) return;
    const int s = p.slot ? p.slot[i] : (int)i;
    if (s < 0 || s >= p.r.S) return;
    ghost_motion_warp_corner(p.r, s, row, corner, p.w);
}

struct GhostMotionStepArgs {
    GhostMotionRings r;
    const int* slot; double* out;
    int n, num_active, last_n, diff32;
};

// Coordinate c of one motion() step of the valid slot s -> its pos afterwards: the body of busca_ghost_motion_step.  `active`: the velocity is
// taken from the window first (and stored); otherwise the stored one is used.  ghost_motion_step_kernel and gframe_advance_kernel
// (gframe_kernel.hip.inc) are this function behind two addressings.
__device__ __forceinline__ double ghost_motion_step_coord(const GhostMotionRings& r, int s, int c, bool active, int last_n, int diff32) {
    int cnt, nw;
    ghost_motion_ring(r, s, cnt, nw);
    double pos = r.pos[(size_t)s * 4 + c];
    if (cnt > 1) {
        double v;
        if (active) {
            const int w = cnt < last_n ? cnt : last_n;
            const double* hist = r.hist + (size_t)s * r.H * 4 + c;
            const int* frames = r.frames + (size_t)s * r.H;
            int row = ghost_motion_oldest(nw, w, r.H);
            double p0 = hist[(size_t)row * 4];
            int f0 = frames[row];
            double sum = 0.0;
            for (int k = 1; k < w; ++k) {                                  // oldest pair first, as np.mean(axis=0) adds the rows
                row = row + 1 == r.H ? 0 : row + 1;
                const double p1 = hist[(size_t)row * 4];
                const int f1 = frames[row];
                const double d = diff32 ? (double)((float)p1 - (float)p0) : p1 - p0;
                const double q = d / (double)((long long)f1 - (long long)f0);
                sum = k == 1 ? q : sum + q;                                // the first row starts the sum (a lone -0.0 stays -0.0)
                p0 = p1;
                f0 = f1;
            }
            v = sum / (double)(w - 1);
            r.vel[(size_t)s * 4 + c] = v;
        } else {
            v = r.vel[(size_t)s * 4 + c];
        }
        pos = pos + v;
        r.pos[(size_t)s * 4 + c] = pos;
    }
    return pos;
}

__global__ void __launch_bounds__(GHOST_MOTION_THREADS) ghost_motion_step_kernel(GhostMotionStepArgs p) {
    const long long t = (long long)blockIdx.x * GHOST_MOTION_THREADS + threadIdx.x;
    const long long i = t >> 2;
    const int c = (int)(t & 3);
    if (i >= p.n) return;
    const int s = p.slot[i];
    if (s < 0 || s >= p.r.S) {
        p.out[(size_t)i * 4 + c] = __builtin_nan("");
        return;
    }
    p.out[(size_t)i * 4 + c] = ghost_motion_step_coord(p.r, s, c, i < p.num_active, p.last_n, p.diff32);
}

#pragma clang fp contract(fast)
