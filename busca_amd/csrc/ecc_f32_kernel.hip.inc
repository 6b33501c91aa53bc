// GHOST's camera-motion estimate: adapters/GHOST/src/base_tracker.py:600-633 (cv2.cvtColor RGB2GRAY on two float32 frames in [0, 1] +
// cv2.findTransformECC(template = current, input = previous, ..., gaussFiltSize = 15)).  Same third-party arithmetic as ecc_kernel.hip.inc,
// restated in tests/ghost_ecc_ref.py; PARITY UNPINNED against the real cv2.  The frame is prepared ONCE (busca_ecc_prepare): its blurred grey
// is the template of this frame's call and the input of the next one's.
//   ecc_prep_h_kernel  planar float32 RGB (any element strides) -> float grey into an LDS row tile -> horizontal K-tap Gaussian: the grey
//                      image is never written.  One block = 256 output pixels of one row + a halo of K / 2 on either side.
//   ecc_blur_vk_kernel vertical K-tap Gaussian.
// Both accumulate the taps in the order of ecc_blur_h/v_kernel (left to right, top to bottom; s = k0 * v0, s = s + k1 * v1, ...), so K = 5
// reproduces them bit for bit.  Borders: BORDER_REFLECT_101; the C ABI refuses H or W < K / 2 + 1, so one reflection lands inside the image.
// Algorithmic bytes per pixel: 12 (RGB) + 4 (row-blurred out) in the first pass; 4 in (K row taps, L2 hits after the first) + 4 out in the second.

#define ECC_KMAX 31
#define ECC_TILE 256

struct EccTaps { float k[ECC_KMAX]; };

__global__ void __launch_bounds__(ECC_TILE) ecc_prep_h_kernel(const float* __restrict__ img, int channels, int H, int W, long stride_c, long stride_row,
                                                              long stride_col, const EccTaps taps, int K, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float tile[ECC_TILE + ECC_KMAX - 1];
    const int R = K >> 1, x0 = blockIdx.x * ECC_TILE, y = blockIdx.y;
    const float* row = img + (long)y * stride_row;
    const int last = min(x0 + ECC_TILE, W) - 1 + R;                          // the rightmost (unreflected) column a live thread of this block reads
    for (int t = threadIdx.x; t < ECC_TILE + 2 * R; t += ECC_TILE) {
        const int gx = x0 - R + t;
        if (gx > last) break;
        const float* p = row + (long)ecc_reflect101(gx, W) * stride_col;
        float g = p[0];
        if (channels == 3) g = (p[0] * 0.299f + p[stride_c] * 0.587f) + p[2 * stride_c] * 0.114f;      // float RGB2GRAY, left to right
        tile[t] = g;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    float s = taps.k[0] * tile[threadIdx.x];
    for (int i = 1; i < K; ++i) s = s + taps.k[i] * tile[threadIdx.x + i];
    out[(size_t)y * W + x] = s;
}

__global__ void __launch_bounds__(256) ecc_blur_vk_kernel(const float* __restrict__ in, int H, int W, const EccTaps taps, int K, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int R = K >> 1;
    float s = taps.k[0] * in[(size_t)ecc_reflect101(y - R, H) * W + x];
    for (int i = 1; i < K; ++i) s = s + taps.k[i] * in[(size_t)ecc_reflect101(y - R + i, H) * W + x];
    out[(size_t)y * W + x] = s;
}
