// Camera-motion compensation: adapters/ByteTrack/yolox/tracker/byte_tracker.py:626-650 (cv2.cvtColor BGR2GRAY on the previous
// and the current frame + cv2.findTransformECC, opencv_python 4.7.0.72 - third-party arithmetic, absent from the reference
// tree; restated from the published algorithm (Evangelidis & Psarakis, PAMI 2008) in the evaluation order of OpenCV's
// video/src/ecc.cpp, see oracle/ecc.py.  PARITY UNPINNED against the real cv2).
//
// All kernels are HBM-bound streaming passes over H x W float images:
//   ecc_gray_kernel    u8 BGR -> gray (8-bit fixed point) -> f32
//   ecc_blur_h/v       separable [1 4 6 4 1]/16, BORDER_REFLECT_101
//   ecc_grad_kernel    [-0.5 0 0.5] central differences of the blurred input image
//   ecc_iter_kernel<P> ONE pass per ECC iteration: warps image + gradients with OpenCV's fixed-point coordinates, builds the
//                      Jacobian row of the pixel and accumulates every sum the update needs (n, I, T, II, TT, IT, J, J.I, J.T,
//                      J J^T) in float64; per-block partials, fixed-order second stage (ecc_reduce_kernel) -> NS doubles.
//   Algorithmic bytes per iteration: 4 (template) + 3 x 4 (image, gx, gy, bilinear taps hit L1/L2) = 16 B per pixel.
// The P x P solve and the warp update run on the host between iterations (a few hundred FLOPs).

static __device__ __forceinline__ int ecc_reflect101(int i, int n) { i = i < 0 ? -i : i; return i >= n ? 2 * (n - 1) - i : i; }

__global__ void __launch_bounds__(256) ecc_gray_kernel(const uint8_t* __restrict__ frame, int H, int W, int stride, float* __restrict__ out) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint8_t* p = frame + (size_t)y * stride + (size_t)x * 3;
    const int g = (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14;      // cv::cvtColor BGR2GRAY, 8-bit path
    out[(size_t)y * W + x] = (float)g;
}

__global__ void __launch_bounds__(256) ecc_blur_h_kernel(const float* __restrict__ in, int H, int W, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float* r = in + (size_t)y * W;
    const float k0 = 0.0625f, k1 = 0.25f, k2 = 0.375f;
    float s = k0 * r[ecc_reflect101(x - 2, W)];
    s = s + k1 * r[ecc_reflect101(x - 1, W)];
    s = s + k2 * r[x];
    s = s + k1 * r[ecc_reflect101(x + 1, W)];
    s = s + k0 * r[ecc_reflect101(x + 2, W)];
    out[(size_t)y * W + x] = s;
}

__global__ void __launch_bounds__(256) ecc_blur_v_kernel(const float* __restrict__ in, int H, int W, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float k0 = 0.0625f, k1 = 0.25f, k2 = 0.375f;
    float s = k0 * in[(size_t)ecc_reflect101(y - 2, H) * W + x];
    s = s + k1 * in[(size_t)ecc_reflect101(y - 1, H) * W + x];
    s = s + k2 * in[(size_t)y * W + x];
    s = s + k1 * in[(size_t)ecc_reflect101(y + 1, H) * W + x];
    s = s + k0 * in[(size_t)ecc_reflect101(y + 2, H) * W + x];
    out[(size_t)y * W + x] = s;
}

__global__ void __launch_bounds__(256) ecc_grad_kernel(const float* __restrict__ I, int H, int W, float* __restrict__ gx, float* __restrict__ gy) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t o = (size_t)y * W + x;
    gx[o] = 0.5f * I[(size_t)y * W + ecc_reflect101(x + 1, W)] - 0.5f * I[(size_t)y * W + ecc_reflect101(x - 1, W)];
    gy[o] = 0.5f * I[(size_t)ecc_reflect101(y + 1, H) * W + x] - 0.5f * I[(size_t)ecc_reflect101(y - 1, H) * W + x];
}

#define ECC_NS(P) (6 + 3 * (P) + (P) * ((P) + 1) / 2)
#define ECC_MAX_BLOCKS 1024

struct EccIterArgs {
    const float *T, *I, *gx, *gy;
    int H, W;
    double m[6];             // the float32 warp matrix, widened (row-major 2x3)
    float h0, h1;            // m[0], m[3] (cos, sin) for the Euclidean Jacobian
    double* partials;        // [gridDim.x][NS]
};

// P = 2: translation (tx, ty); P = 3: Euclidean (theta, tx, ty); P = 6: affine.
template <int P>
__global__ void __launch_bounds__(256) ecc_iter_kernel(const EccIterArgs g) {
#pragma clang fp contract(off)
    constexpr int NS = ECC_NS(P);
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    const int H = g.H, W = g.W;
    const long npix = (long)H * W;
    for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (long)gridDim.x * 256) {
        const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
        // cv::warpAffine with WARP_INVERSE_MAP: source = M [x y 1]^T in 1/1024-pixel fixed point, 5 fractional bits used
        const long adelta = (long)rint(g.m[0] * (double)x * 1024.0), bdelta = (long)rint(g.m[3] * (double)x * 1024.0);
        const long X0 = (long)rint((g.m[1] * (double)y + g.m[2]) * 1024.0) + 16, Y0 = (long)rint((g.m[4] * (double)y + g.m[5]) * 1024.0) + 16;
        const long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
        const long sx = X >> 5, sy = Y >> 5;
        const int ax = (int)(X & 31), ay = (int)(Y & 31);
        const long nx = sx + (ax >= 16), ny = sy + (ay >= 16);           // INTER_NEAREST of the all-ones mask
        const bool in_mask = nx >= 0 && nx < W && ny >= 0 && ny < H;
        if (sx + 1 < 0 || sx >= W || sy + 1 < 0 || sy >= H) continue;      // no bilinear tap inside: every warped value is 0
        // ecc.cpp warps the image and its gradients WITHOUT the mask: a fringe pixel outside the (nearest-neighbour) mask whose
        // bilinear taps are partly inside still enters the Hessian and the image projection; only the mean / norm / template
        // terms are masked.
        const float fx = (float)ax / 32.0f, fy = (float)ay / 32.0f;
        const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
        const bool x0ok = sx >= 0 && sx < W, x1ok = sx + 1 >= 0 && sx + 1 < W, y0ok = sy >= 0 && sy < H, y1ok = sy + 1 >= 0 && sy + 1 < H;
        const size_t o00 = (size_t)(y0ok ? sy : 0) * W + (x0ok ? sx : 0), o01 = (size_t)(y0ok ? sy : 0) * W + (x1ok ? sx + 1 : 0);
        const size_t o10 = (size_t)(y1ok ? sy + 1 : 0) * W + (x0ok ? sx : 0), o11 = (size_t)(y1ok ? sy + 1 : 0) * W + (x1ok ? sx + 1 : 0);
        const bool k00 = y0ok && x0ok, k01 = y0ok && x1ok, k10 = y1ok && x0ok, k11 = y1ok && x1ok;
        auto samp = [&](const float* im) -> float {
            const float v00 = k00 ? im[o00] : 0.f, v01 = k01 ? im[o01] : 0.f, v10 = k10 ? im[o10] : 0.f, v11 = k11 ? im[o11] : 0.f;
            float s = v00 * w00;
            s = s + v01 * w01;
            s = s + v10 * w10;
            s = s + v11 * w11;
            return s;
        };
        const float Iw = samp(g.I), gxw = samp(g.gx), gyw = samp(g.gy);
        const float Tv = g.T[pix];
        float J[P];
        const float Xf = (float)x, Yf = (float)y;
        if constexpr (P == 2) {
            J[0] = gxw; J[1] = gyw;
        } else if constexpr (P == 3) {
            const float hatX = -(Xf * g.h1) - (Yf * g.h0), hatY = (Xf * g.h0) - (Yf * g.h1);
            J[0] = gxw * hatX + gyw * hatY; J[1] = gxw; J[2] = gyw;
        } else {
            J[0] = gxw * Xf; J[1] = gyw * Xf; J[2] = gxw * Yf; J[3] = gyw * Yf; J[4] = gxw; J[5] = gyw;
        }
        const double Id = (double)Iw, Td = in_mask ? (double)Tv : 0.0, mk = in_mask ? 1.0 : 0.0;
        acc[0] += mk; acc[1] += mk * Id; acc[2] += Td; acc[3] += mk * Id * Id; acc[4] += Td * Td; acc[5] += mk * Id * Td;
        int k = 6 + 3 * P;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const double Ji = (double)J[i];
            acc[6 + i] += mk * Ji;                  // masked: multiplies the means
            acc[6 + P + i] += Ji * Id;              // all pixels (raw warped image outside the mask)
            acc[6 + 2 * P + i] += mk * Ji * Td;     // masked (the zero-mean template is 0 outside)
#pragma unroll
            for (int j = i; j < P; ++j) acc[k++] += Ji * (double)J[j];     // all pixels
        }
    }
    // block reduction in a fixed order: lanes (xor tree), then the four waves
    __shared__ double sh[4][NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) sh[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NS) g.partials[(size_t)blockIdx.x * NS + threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

__global__ void __launch_bounds__(64) ecc_reduce_kernel(const double* __restrict__ partials, int nblocks, int NS, double* __restrict__ out) {
    const int s = threadIdx.x;
    if (s >= NS) return;
    double v = 0.0;
    for (int b = 0; b < nblocks; ++b) v += partials[(size_t)b * NS + s];
    out[s] = v;
}
