/*
 * busca_ecc.h - GHOST's camera-motion estimate as device calls of libbusca_hip.so: adapters/GHOST/src/base_tracker.py:600-633
 * (motion_compensation: two float32 [3, H, W] frames in [0, 1] -> cv2.cvtColor RGB2GRAY -> cv2.findTransformECC(templateImage = CURRENT
 * frame, inputImage = PREVIOUS frame, eye(2, 3), Translation | Euclidean | Affine, (EPS | COUNT, num_iter_mc, termination_eps_mc), None,
 * gaussFiltSize = 15)).  busca_ecc_align (busca_hip.h) is ByteTrack's call - u8 BGR, 8-bit grey, 5-tap blur, previous as template - and
 * keeps its behaviour; this header splits the work so that a frame is prepared ONCE: its blurred grey plane is the template of this
 * frame's alignment and the input of the next frame's.
 *
 * PARITY UNPINNED: OpenCV is third-party arithmetic that is neither in the reference tree nor installable where this is built.  The
 * algorithm is restated (oracle/ecc.py, tests/ghost_ecc_ref.py) in the order OpenCV's ecc.cpp evaluates it.  Two orders of evaluation
 * are a guess: the float grey, here (R * 0.299f + G * 0.587f) + B * 0.114f in float32, and the Gaussian, here tap by tap from the
 * left / the top where OpenCV's column filter adds symmetric pairs.
 *
 * Same conventions as busca_hip.h (return codes, dev / host pointers, `stream`, one ctx per GPU/process).  Scratch lives in the context
 * (the workspace of busca_ecc_align, grown when a larger frame arrives: growth synchronises `stream` and allocates).
 */
#ifndef BUSCA_ECC_H
#define BUSCA_ECC_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_ECC_KSIZE_MAX 31
#define BUSCA_ECC_EUCLIDEAN 0      /* motion codes: 0 and 1 are busca_ecc_align's */
#define BUSCA_ECC_AFFINE 1
#define BUSCA_ECC_TRANSLATION 2

/* cv::getGaussianKernel(ksize, sigma <= 0, CV_32F), host only (ctx-free, no GPU): the fixed tables for ksize 1, 3, 5, 7
 * ([1], [1 2 1] / 4, [1 4 6 4 1] / 16, [1 3.5 7 9 7 3.5 1] / 32); otherwise sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8 and
 * exp(-x^2 / (2 sigma^2)) for x = i - (ksize - 1) / 2 in double, divided by the sum, then rounded to float.
 *   taps  HOST f32 [ksize]
 * BUSCA_EINVAL: ksize even, < 1 or > BUSCA_ECC_KSIZE_MAX; taps NULL. */
int busca_ecc_gauss_taps(int32_t ksize, float* taps);

/* One frame -> its blurred grey plane: RGB2GRAY in float32, then the separable ksize x ksize Gaussian of busca_ecc_gauss_taps (rows, then
 * columns; BORDER_REFLECT_101; float32 accumulation from the first tap to the last - ksize = 5 on a one-channel plane has the bits of
 * busca_ecc_align's blur).  Two launches: grey + rows (the grey image stays in LDS), columns.
 *   img       dev f32, planar: element (c, y, x) at img[c * stride_c + y * stride_row + x * stride_col] - strides in ELEMENTS, so a
 *             contiguous [3, H, W] tensor is (H * W, W, 1), an [H, W, 3] frame viewed as [3, H, W] is (1, 3 * W, 3), and a crop keeps
 *             its parent's strides.  Values are taken as they are (the reference's are in [0, 1]).
 *   channels  3: R, G, B; 1: the plane is the grey (stride_c is ignored)
 *   out       dev f32 [H, W], contiguous, caller-owned; must not overlap img
 * Asynchronous on `stream` unless the workspace grows.
 * BUSCA_EINVAL: ksize as above; H or W < max(8, ksize / 2 + 1) (a single reflection must stay inside the image); channels not 1 or 3;
 * a negative row or column stride, stride_col = 0; img or out NULL. */
int busca_ecc_prepare(busca_ctx* ctx, const float* img, int32_t channels, int32_t H, int32_t W, int64_t stride_c, int64_t stride_row,
                      int64_t stride_col, int32_t ksize, float* out, void* stream);

/* cv2.findTransformECC on two prepared planes: the gradients of `input`, then exactly the loop of busca_ecc_align - one pass over the
 * pixels per iteration, the P x P solve on the host (P = 2, 3, 6), one synchronisation of `stream` per iteration, the same termination
 * rule (stop when |rho - last_rho| < eps or after max_iters iterations) and the same refusals (singular Hessian, no overlap, NaN,
 * correlation about to be minimised: BUSCA_EINVAL with a message, warp / cc / iters untouched).
 *   templ, input  dev f32 [H, W], contiguous (busca_ecc_prepare's `out`); neither is written
 *   motion        BUSCA_ECC_EUCLIDEAN, _AFFINE or _TRANSLATION (the translation update is warp[2] += dp[0], warp[5] += dp[1])
 *   warp          HOST f32 [6], row-major 2x3: the initial warp in, the estimate out (it maps template coordinates to input coordinates)
 *   cc, iters     HOST, may be NULL: the correlation coefficient and the iterations run
 * GHOST: templ = the current frame's plane, input = the previous frame's, warp = identity.
 * BUSCA_EINVAL: H or W < 8, max_iters < 1, an unknown motion, templ / input / warp NULL. */
int busca_ecc_align_planes(busca_ctx* ctx, const float* templ, const float* input, int32_t H, int32_t W, int32_t motion, int32_t max_iters,
                           double eps, float* warp, double* cc, int32_t* iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
