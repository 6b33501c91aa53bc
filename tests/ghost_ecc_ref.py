"""Checker (CPU, test infrastructure only) of GHOST's camera-motion estimate, adapters/GHOST/src/base_tracker.py:600-633:
`cv2.cvtColor(RGB2GRAY)` on two float32 frames in [0, 1] + `cv2.findTransformECC(template=current, input=previous, eye(2,3),
TRANSLATION|EUCLIDEAN|AFFINE, (EPS|COUNT, num_iter_mc, termination_eps_mc), None, gaussFiltSize=15)`.

PARITY UNPINNED: like oracle/ecc.py this restates OpenCV, which is neither in the reference tree nor installable here, so no recorded
output exists.  Beyond what oracle/ecc.py already says about itself, OpenCV's own order of evaluation is a GUESS in two places:
  * the float grey.  cvtColor's CV_32F path computes 0.299 R + 0.587 G + 0.114 B; whether its vector code adds left to right, fuses a
    multiply-add or orders the channels otherwise is not known here.  Stated: (R * 0.299f + G * 0.587f) + B * 0.114f, float32.
  * the symmetric-pair column filter.  OpenCV's separable Gaussian runs a symmetric column filter that adds the two rows of a pair first,
    (row[-i] + row[+i]) * k[i], around the centre tap.  Stated: tap by tap from the first to the last, s = k[0] v[0]; s = s + k[i] v[i],
    for rows and columns alike - the order of oracle.ecc.blur5, which this reproduces bit for bit at K = 5.
What is stated here: the float grey, the K-tap blur, the Gaussian taps and the translation Jacobian.  gradients, warp_coords, warp_linear,
warp_mask_nearest and the Euclidean / affine loop are oracle.ecc's own: the loop is find_transform_ecc itself, run on planes that are
already blurred (its blur5 rebound to the identity).  Translation is not a branch of that loop, so `_loop` below repeats its iteration
with the Jacobian as an argument; tests/test_ghost_ecc.py holds `_loop` with the Euclidean Jacobian to the oracle's trace bit for bit."""
import types

import numpy as np

from oracle import ecc

SMALL_TAPS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
              7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
MOTIONS = ("translation", "euclidean", "affine")


def gauss_taps(K):
    """cv::getGaussianKernel(K, sigma <= 0, CV_32F): the closed form in float64, rounded to float32 (fixed tables up to 7)."""
    if K in SMALL_TAPS:
        return np.array(SMALL_TAPS[K], np.float32)
    sigma = 0.3 * ((K - 1) * 0.5 - 1) + 0.8
    x = np.arange(K, dtype=np.float64) - (K - 1) * 0.5
    v = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (v / v.sum()).astype(np.float32)


def gray_f32(img):
    """[3,H,W] float32 RGB -> float32 grey, (R * 0.299f + G * 0.587f) + B * 0.114f; an [H,W] plane is the grey."""
    img = np.asarray(img, np.float32)
    if img.ndim == 2:
        return img.copy()
    return ((img[0] * np.float32(0.299) + img[1] * np.float32(0.587)) + img[2] * np.float32(0.114)).astype(np.float32)


def blur(x, taps):
    """float32 separable K-tap filter, reflect-101 borders, rows then columns, taps accumulated from the first to the last."""
    k = np.asarray(taps, np.float32)
    K, R = len(k), len(k) // 2
    H, W = x.shape
    assert H > R and W > R, "a single reflection must stay inside the image"
    xp = x[:, ecc._reflect101(np.arange(-R, W + R), W)]
    t = k[0] * xp[:, 0:W]
    for i in range(1, K):
        t = t + k[i] * xp[:, i:i + W]
    tp = t[ecc._reflect101(np.arange(-R, H + R), H), :]
    b = k[0] * tp[0:H, :]
    for i in range(1, K):
        b = b + k[i] * tp[i:i + H, :]
    assert b.dtype == np.float32
    return b


def prepare(img, taps):
    """busca_ecc_prepare: one frame -> its blurred grey plane."""
    return blur(gray_f32(img), taps)


# oracle.ecc.find_transform_ecc on planes that are blurred already: the same code object, its `blur5` bound to the identity
_oracle_loop = types.FunctionType(ecc.find_transform_ecc.__code__, {**vars(ecc), "blur5": lambda x: x}, "find_transform_ecc_planes",
                                  ecc.find_transform_ecc.__defaults__)


def jacobian(motion, gxw, gyw, M, Xg, Yg):
    if motion == "translation":
        return [gxw, gyw]
    if motion == "euclidean":
        h0, h1 = M[0, 0], M[1, 0]
        return [gxw * (-(Xg * h1) - (Yg * h0)) + gyw * ((Xg * h0) - (Yg * h1)), gxw, gyw]
    return [gxw * Xg, gyw * Xg, gxw * Yg, gyw * Yg, gxw, gyw]


def _loop(T, I, M, motion, iters, eps):
    """The iteration of oracle.ecc.find_transform_ecc with the Jacobian and the update of `motion` -> (rho, M, trace)."""
    gx, gy = ecc.gradients(I)
    H, W = T.shape
    Xg, Yg = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    dot = lambda a, b: float(np.dot(a.astype(np.float64).ravel(), b.astype(np.float64).ravel()))
    rho, last_rho, trace, it = -1.0, -eps, [], 1
    while it <= iters and abs(rho - last_rho) >= eps:
        co = ecc.warp_coords(M, H, W)
        mask = ecc.warp_mask_nearest(co, H, W)
        Iw, gxw, gyw = ecc.warp_linear(I, co), ecc.warp_linear(gx, co), ecc.warp_linear(gy, co)
        n = int(mask.sum())
        mI, mT = Iw[mask].astype(np.float64).mean(), T[mask].astype(np.float64).mean()
        Izm = np.where(mask, Iw - np.float32(mI), Iw).astype(np.float32)
        Tzm = np.where(mask, T - np.float32(mT), np.float32(0)).astype(np.float32)
        img_norm, tmp_norm = np.sqrt(n * Iw[mask].astype(np.float64).var()), np.sqrt(n * T[mask].astype(np.float64).var())
        J = [j.astype(np.float32) for j in jacobian(motion, gxw, gyw, M, Xg, Yg)]
        P = len(J)
        hess = np.array([[dot(J[i], J[j]) for j in range(P)] for i in range(P)], np.float32)
        hinv = np.linalg.inv(hess.astype(np.float64)).astype(np.float32)
        corr = dot(Tzm, Izm)
        last_rho, rho = rho, corr / (img_norm * tmp_norm)
        if np.isnan(rho):
            raise RuntimeError("NaN encountered.")
        ip, tp = np.array([dot(j, Izm) for j in J], np.float32), np.array([dot(j, Tzm) for j in J], np.float32)
        iph = hinv @ ip
        lam_n = img_norm * img_norm - float(np.dot(ip.astype(np.float64), iph.astype(np.float64)))
        lam_d = corr - float(np.dot(tp.astype(np.float64), iph.astype(np.float64)))
        if lam_d <= 0.0:
            raise RuntimeError("The algorithm stopped before its convergence. The correlation is going to be minimized.")
        err = (np.float32(lam_n / lam_d) * Tzm - Izm).astype(np.float32)
        dp = hinv @ np.array([dot(j, err) for j in J], np.float32)
        if motion == "translation":
            M[0, 2] += dp[0]; M[1, 2] += dp[1]
        elif motion == "euclidean":
            th = np.float32(np.arcsin(M[1, 0])) + dp[0]
            M[0, 2] += dp[1]; M[1, 2] += dp[2]
            M[0, 0] = M[1, 1] = np.float32(np.cos(th)); M[1, 0] = np.float32(np.sin(th)); M[0, 1] = -M[1, 0]
        else:
            M[0, 0] += dp[0]; M[1, 0] += dp[1]; M[0, 1] += dp[2]; M[1, 1] += dp[3]; M[0, 2] += dp[4]; M[1, 2] += dp[5]
        trace.append((rho, M.copy()))
        it += 1
    return rho, M, trace


def align_planes(templ, inp, warp=None, motion="euclidean", iters=100, eps=1e-5, return_trace=False, own_loop=False):
    """busca_ecc_align_planes: two blurred planes -> (rho, warp float32 [2,3][, trace]).  Raises where OpenCV raises.  Euclidean and affine
    run oracle.ecc's loop; translation (and own_loop=True, for the test that pins it) runs `_loop`."""
    assert motion in MOTIONS
    T, I = np.asarray(templ, np.float32), np.asarray(inp, np.float32)
    if motion == "translation" or own_loop:
        M = np.eye(2, 3, dtype=np.float32) if warp is None else np.array(warp, np.float32).reshape(2, 3)
        r = _loop(T, I, M, motion, iters, eps)
    else:
        r = _oracle_loop(T, I, warp=warp, motion=motion, iters=iters, eps=eps, return_trace=True)
    return r if return_trace else r[:2]


def find_transform_ecc(template, inp, warp=None, motion="euclidean", K=15, iters=100, eps=1e-5, return_trace=False, taps=None):
    """cv2.findTransformECC(gray(template), gray(inp), warp, motion, (EPS|COUNT, iters, eps), None, K) on float frames."""
    taps = gauss_taps(K) if taps is None else taps
    return align_planes(prepare(template, taps), prepare(inp, taps), warp, motion, iters, eps, return_trace)
