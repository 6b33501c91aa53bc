// GHOST's linear motion model (include/busca_ghost_motion.h): per-track rings of past boxes in HBM, the velocity step, the camera warp.  Three kernels:
//
//   ghost_motion_append_kernel  one thread per (slot, detection) pair: pos = box, box and frame pushed onto the ring (one 32-byte row)
//   ghost_motion_warp_kernel    one thread per (listed slot, ring row, corner): W . (x, y, 1) in float64, rounded once to float32
//   ghost_motion_step_kernel    one thread per (track, coordinate): the pair velocities of the window summed sequentially, oldest pair first
//
// A few hundred tracks of four coordinates each: every launch is a handful of waves whose time is the launch and one dependent chain of loads per thread
// (latency-bound; there is no byte or FLOP rate to approach).  The four coordinates of a track are four adjacent lanes, so a ring row is one 32-byte read.
// No multiply-add contraction: every sum, product and quotient is the IEEE operation numpy performs.
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

__global__ void __launch_bounds__(GHOST_MOTION_THREADS) ghost_motion_append_kernel(GhostMotionAppendArgs p) {
    const long long i = (long long)blockIdx.x * GHOST_MOTION_THREADS + threadIdx.x;
    if (i >= p.k) return;
    const int s = p.slot[i];
    const int j = p.det ? p.det[i] : (int)i;
    if (s < 0 || s >= p.r.S || j < 0 || j >= p.m) return;
    int cnt, nw;
    ghost_motion_ring(p.r, s, cnt, nw);
    const bool fresh = p.reset && p.reset[i];
    if (fresh) cnt = 0;
    const int row = cnt == 0 ? 0 : (nw + 1) % p.r.H;
    const double* box = p.boxes + (size_t)j * 4;
    double* hist = p.r.hist + ((size_t)s * p.r.H + row) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = box[c];
        p.r.pos[(size_t)s * 4 + c] = v;
        hist[c] = v;
        if (fresh) p.r.vel[(size_t)s * 4 + c] = 0.0;
    }
    p.r.frames[(size_t)s * p.r.H + row] = p.frame;
    p.r.count[s] = cnt < p.r.H ? cnt + 1 : p.r.H;
    p.r.newest[s] = row;
}

struct GhostMotionWarpArgs {
    GhostMotionRings r;
    const int* slot;
    int n;
    double w[6];
};

__global__ void __launch_bounds__(GHOST_MOTION_THREADS) ghost_motion_warp_kernel(GhostMotionWarpArgs p) {
    const long long t = (long long)blockIdx.x * GHOST_MOTION_THREADS + threadIdx.x;
    const int corner = (int)(t & 1);
    const long long q = t >> 1;
    const int row = (int)(q % p.r.H);
    const long long i = q / p.r.H;
    if (i >= p.n) return;
    const int s = p.slot ? p.slot[i] : (int)i;
    if (s < 0 || s >= p.r.S) return;
    int cnt, nw;
    ghost_motion_ring(p.r, s, cnt, nw);
    int back = (nw - row) % p.r.H;                                         // rows back from the newest one
    if (back < 0) back += p.r.H;
    if (back >= cnt) return;
    double* xy = p.r.hist + ((size_t)s * p.r.H + row) * 4 + 2 * corner;
    const double x = xy[0], y = xy[1];
    const double xn = (p.w[0] * x + p.w[1] * y) + p.w[2];
    const double yn = (p.w[3] * x + p.w[4] * y) + p.w[5];
    xy[0] = (double)(float)xn;
    xy[1] = (double)(float)yn;
}

struct GhostMotionStepArgs {
    GhostMotionRings r;
    const int* slot; double* out;
    int n, num_active, last_n, diff32;
};

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
    int cnt, nw;
    ghost_motion_ring(p.r, s, cnt, nw);
    double pos = p.r.pos[(size_t)s * 4 + c];
    if (cnt > 1) {
        double v;
        if (i < p.num_active) {
            const int w = cnt < p.last_n ? cnt : p.last_n;
            const double* hist = p.r.hist + (size_t)s * p.r.H * 4 + c;
            const int* frames = p.r.frames + (size_t)s * p.r.H;
            int row = ghost_motion_oldest(nw, w, p.r.H);
            double p0 = hist[(size_t)row * 4];
            int f0 = frames[row];
            double sum = 0.0;
            for (int k = 1; k < w; ++k) {                                  // oldest pair first, as np.mean(axis=0) adds the rows
                row = row + 1 == p.r.H ? 0 : row + 1;
                const double p1 = hist[(size_t)row * 4];
                const int f1 = frames[row];
                const double d = p.diff32 ? (double)((float)p1 - (float)p0) : p1 - p0;
                const double q = d / (double)((long long)f1 - (long long)f0);
                sum = k == 1 ? q : sum + q;                                // the first row starts the sum (a lone -0.0 stays -0.0)
                p0 = p1;
                f0 = f1;
            }
            v = sum / (double)(w - 1);
            p.r.vel[(size_t)s * 4 + c] = v;
        } else {
            v = p.r.vel[(size_t)s * 4 + c];
        }
        pos = pos + v;
        p.r.pos[(size_t)s * 4 + c] = pos;
    }
    p.out[(size_t)i * 4 + c] = pos;
}

#pragma clang fp contract(fast)
