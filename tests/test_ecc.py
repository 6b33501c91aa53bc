"""Camera-motion compensation: busca_ecc_align against the oracle restatement of cv2.findTransformECC and
against known transforms.  (cv2 itself is third-party and absent: parity unpinned, see oracle/ecc.py.)

Step form (test_ecc_step_matches_oracle and its CPU twin): every call takes ONE iteration from the oracle's own previous
iterate, so two correct implementations cannot drift apart (free-running affine iterates separate by 4e-4 in six iterations
on a 25 px shift; one step holds 2e-6).  The kernel forms ip / tp / ep by linearity from unrounded float64 sums, the oracle
from element-wise float32 zero-mean images; `_step_f64` below restates the kernel's formulation in numpy so that the gap
between the two formulations - and what two deliberate errors would do to it - is measured without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

RHO_BAR, WARP_BAR = 1e-5, 2e-5            # the bars of test_ecc_matches_oracle; the step tests use the same two
MOTIONS = ["MOTION_EUCLIDEAN", "MOTION_AFFINE"]


def _pair(H=120, W=160, th=0.01, tx=2.3, ty=-1.4, seed=0, cell=8):
    """Smooth random image and a copy moved by a known Euclidean transform: im1(x) ~ im2(M x).  BGR frames.  `cell` is the
    feature size in pixels (small frames need a finer one, or they come out flat)."""
    from scipy.ndimage import affine_transform, zoom
    rng = np.random.default_rng(seed)
    chans1, chans2 = [], []
    c, s = np.cos(th), np.sin(th)
    A = np.array([[c, -s], [s, c]])
    Ainv = np.linalg.inv(A)
    R = np.array([[Ainv[1, 1], Ainv[1, 0]], [Ainv[0, 1], Ainv[0, 0]]])
    off = -(R @ np.array([ty, tx]))
    for _ in range(3):
        big = zoom(rng.uniform(0, 255, (H // cell + 4, W // cell + 4)), cell, order=3)[2 * cell:2 * cell + H, 2 * cell:2 * cell + W]
        chans1.append(np.clip(big, 0, 255))
        chans2.append(np.clip(affine_transform(big, R, offset=off, order=3, mode="nearest"), 0, 255))
    im1, im2 = np.stack(chans1, -1).astype(np.uint8), np.stack(chans2, -1).astype(np.uint8)
    return im1, im2, np.array([[c, -s, tx], [s, c, ty]])


def _rot(th, tx, ty):
    return [[np.cos(th), -np.sin(th), tx], [np.sin(th), np.cos(th), ty]]


# name -> H, W, theta, tx, ty, seed, cell, init (None = the identity default), steps, motions.
# What each reaches: the reductions use one block up to 1024 pixels and two from 1025; the 2-D grids of the grey / blur /
# gradient kernels get a second x-block at W = 257; the block cap of the iteration kernel is passed at 1024 * 1024 pixels.
BOTH = ("euclidean", "affine")
CASES = {
    "8x8": (8, 8, 0.0, 0.3, 0.2, 2, 2, None, 6, ("euclidean",)),            # smallest the ABI takes; affine Hessian singular
    "9x13": (9, 13, 0.0, 0.3, 0.2, 5, 2, None, 6, BOTH),                    # one block, border-dominated
    "16x16": (16, 16, 0.0, 0.3, 0.2, 5, 2, None, 6, BOTH),                  # one block
    "32x32": (32, 32, 0.004, 0.7, -0.6, 11, 4, None, 6, BOTH),              # exactly 1024 pixels
    "25x41": (25, 41, -0.004, -0.6, 0.7, 12, 4, None, 6, BOTH),             # 1025 pixels, two blocks
    "24x40": (24, 40, 0.005, 0.6, -0.4, 6, 4, None, 6, BOTH),
    "24x256": (24, 256, 0.002, 0.8, -0.6, 13, 8, None, 6, BOTH),            # x-block boundary of the 2-D grids
    "24x257": (24, 257, 0.002, 0.8, -0.6, 13, 8, None, 6, BOTH),
    "67x301": (67, 301, 0.01, 1.3, -0.7, 1, 8, None, 6, BOTH),              # ragged second x-block
    "40x517": (40, 517, -0.005, 1.1, 0.6, 2, 4, None, 6, BOTH),             # third x-block
    "259x33": (259, 33, 0.004, -0.8, 1.2, 3, 4, None, 6, BOTH),             # tall and narrow
    "shift27": (120, 160, 0.01, 24.6, -17.3, 8, 8, [[1, 0, 24], [0, 1, -17]], 6, BOTH),      # 27 % of the frame uncovered
    "shift38": (96, 200, 0.0, -40.4, 21.7, 9, 8, [[1, 0, -40], [0, 1, 22]], 6, BOTH),        # 38 %, negative source coordinates
    "rot0.2": (120, 160, 0.2, 3.0, -2.0, 7, 8, _rot(0.19, 2.5, -1.6), 6, BOTH),              # h1 terms of the Jacobian
    "120x160": (120, 160, 0.01, 2.3, -1.4, 0, 8, None, 6, BOTH),            # the pair of test_ecc_matches_oracle
    "1025x1031": (1025, 1031, 0.001, 1.6, -0.9, 4, 8, None, 2, BOTH),       # just above the block cap; two steps only
}
SHIFTED = ("shift27", "shift38")
CASE_MOTIONS = [(name, m) for name, c in CASES.items() for m in c[9]]
# the oracle's final warp of the free-running call (eps 1e-5, <= 100 iterations), as the largest displacement in pixels of
# the frame's corners and centre from the true transform; measured on the CPU by test_ecc_cases_are_well_posed, which
# also checks that these figures still hold.  {case: (euclidean, affine)}
FREE_RUN = {"67x301": (0.0021, 0.0164), "259x33": (0.0201, 0.0253), "shift27": (0.0074, 0.0111), "shift38": (0.0355, 0.0503)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (im1, im2, true transform, init or None); computed once, shared, never written to."""
    H, W, th, tx, ty, seed, cell, init = CASES[name][:8]
    im1, im2, M = _pair(H, W, th, tx, ty, seed, cell)
    for a in (im1, im2, M):
        a.setflags(write=False)
    return im1, im2, M, None if init is None else np.array(init, np.float32)


@functools.lru_cache(maxsize=None)
def _trace(name, motion):
    """The oracle's iterates with the termination test off: [(rho_k, W_k)], k = 1..steps."""
    from oracle import ecc
    im1, im2, _, init = _case(name)
    return ecc.find_transform_ecc(ecc.bgr2gray(im1), ecc.bgr2gray(im2), warp=init, motion=motion, iters=CASES[name][8],
                                  eps=-1.0, return_trace=True)[2]


def _start(name, motion, k):
    """The warp step k starts from: the oracle's iterate k - 1, or the case's initial warp."""
    init = _case(name)[3]
    return _trace(name, motion)[k - 2][1] if k > 1 else (np.eye(2, 3, dtype=np.float32) if init is None else init)


def _corner_dist(W, M, shape):
    """Largest displacement (pixels, either axis) of the frame's corners and centre under W from where M sends them."""
    h, w = shape[0] - 1, shape[1] - 1
    pts = np.array([[0, 0, 1.0], [w, 0, 1], [0, h, 1], [w, h, 1], [w / 2, h / 2, 1]]).T
    return float(np.abs(np.asarray(W, np.float64) @ pts - M @ pts).max())


# ---- the kernel's formulation in numpy -----------------------------------------------------------------------------------
def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _clamp(i, n):
    return np.clip(i, 0, n - 1)


def _prefilter(gray, border):
    """ecc_blur_h/v + ecc_grad_kernel: [1 4 6 4 1]/16 rows then columns, central differences; `border` maps an index into range."""
    x = gray.astype(np.float32)
    H, W = x.shape
    k = [np.float32(v) for v in (0.0625, 0.25, 0.375, 0.25, 0.0625)]
    cols, rows = [border(np.arange(W) + d, W) for d in range(-2, 3)], [border(np.arange(H) + d, H) for d in range(-2, 3)]
    t = k[0] * x[:, cols[0]]
    for i in range(1, 5):
        t = t + k[i] * x[:, cols[i]]
    b = k[0] * t[rows[0], :]
    for i in range(1, 5):
        b = b + k[i] * t[rows[i], :]
    gx = np.float32(0.5) * b[:, cols[3]] - np.float32(0.5) * b[:, cols[1]]
    gy = np.float32(0.5) * b[rows[3], :] - np.float32(0.5) * b[rows[1], :]
    return b, gx, gy


def _step_f64(T, I, gx, gy, M, motion, drop_fringe=False):
    """One iteration as ecc_iter_kernel + the host loop of busca_ecc_align do it: per-pixel float32 warp and Jacobian, every
    sum over pixels in float64, then ip / tp / ep by linearity from the unrounded sums.  -> (rho, new warp, masked pixels).
    drop_fringe is a deliberate error: pixels outside the nearest-neighbour mask whose bilinear taps are partly inside are
    left out of the Hessian and the image projection (ecc.cpp and the kernel keep them)."""
    from oracle import ecc
    H, W = T.shape
    M = np.array(M, np.float32).reshape(2, 3)
    co = ecc.warp_coords(M, H, W)
    mask = ecc.warp_mask_nearest(co, H, W)
    Iw, gxw, gyw = (ecc.warp_linear(a, co) for a in (I, gx, gy))
    if drop_fringe:
        Iw, gxw, gyw = (np.where(mask, a, np.float32(0)) for a in (Iw, gxw, gyw))
    Xg, Yg = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    if motion == "euclidean":
        h0, h1 = M[0, 0], M[1, 0]
        J = [gxw * (-(Xg * h1) - (Yg * h0)) + gyw * ((Xg * h0) - (Yg * h1)), gxw, gyw]
    else:
        J = [gxw * Xg, gyw * Xg, gxw * Yg, gyw * Yg, gxw, gyw]
    J = [j.astype(np.float32).astype(np.float64) for j in J]
    P, mk, Id = len(J), mask.astype(np.float64), Iw.astype(np.float64)
    Td = np.where(mask, T, np.float32(0)).astype(np.float64)
    n, sI, sT, sII, sTT, sIT = mk.sum(), (mk * Id).sum(), Td.sum(), (mk * Id * Id).sum(), (Td * Td).sum(), (mk * Id * Td).sum()
    sJ, sJI, sJT = (np.array([(j * w).sum() for j in J]) for w in (mk, Id, mk * Td))
    hess = np.array([[(J[i] * J[j]).sum() for j in range(P)] for i in range(P)]).astype(np.float32)
    mI, mT = sI / n, sT / n
    img2, tmp2, corr = sII - n * mI * mI, sTT - n * mT * mT, sIT - n * mI * mT
    hinv = np.linalg.inv(hess.astype(np.float64)).astype(np.float32)
    ip, tp = (sJI - mI * sJ).astype(np.float32), (sJT - mT * sJ).astype(np.float32)
    rho = corr / (np.sqrt(img2) * np.sqrt(tmp2))
    iph = (hinv @ ip).astype(np.float64)
    lam = (img2 - ip.astype(np.float64) @ iph) / (corr - tp.astype(np.float64) @ iph)
    dp = hinv @ (lam * (sJT - mT * sJ) - (sJI - mI * sJ)).astype(np.float32)
    if motion == "euclidean":
        th = np.float32(np.arcsin(M[1, 0])) + dp[0]
        M[0, 2] += dp[1]; M[1, 2] += dp[2]
        M[0, 0] = M[1, 1] = np.float32(np.cos(th)); M[1, 0] = np.float32(np.sin(th)); M[0, 1] = -M[1, 0]
    else:
        M[0, 0] += dp[0]; M[1, 0] += dp[1]; M[0, 1] += dp[2]; M[1, 1] += dp[3]; M[0, 2] += dp[4]; M[1, 2] += dp[5]
    return float(rho), M, int(n)


def _restatement_gaps(name, motion, border=_reflect101, drop_fringe=False):
    """Largest |rho - rho_k|, max|W - W_k| over the steps, each step started from the oracle's previous iterate; and the
    masked share of the frame at every step."""
    from oracle import ecc
    im1, im2 = _case(name)[:2]
    T = _prefilter(ecc.bgr2gray(im1), border)[0]
    I, gx, gy = _prefilter(ecc.bgr2gray(im2), border)
    drho, dwarp, shares = 0.0, 0.0, []
    for k, (rho_k, W_k) in enumerate(_trace(name, motion), 1):
        rho, Wn, n = _step_f64(T, I, gx, gy, _start(name, motion, k), motion, drop_fringe)
        drho, dwarp = max(drho, abs(rho - rho_k)), max(dwarp, float(np.abs(Wn - W_k).max()))
        shares.append(n / T.size)
    return drho, dwarp, shares


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_oracle_recovers_known_transform():
    from oracle import ecc
    im1, im2, M = _pair()
    rho, W = ecc.find_transform_ecc(ecc.bgr2gray(im1), ecc.bgr2gray(im2), motion="euclidean")
    assert rho > 0.99 and np.abs(W - M).max() < 0.02
    rho6, W6 = ecc.find_transform_ecc(ecc.bgr2gray(im1), ecc.bgr2gray(im2), motion="affine")
    assert rho6 > 0.99 and np.abs(W6 - M).max() < 0.03
    g = ecc.bgr2gray(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8))
    assert g.tolist() == [[29, 150, 76, 22]]                   # cv2 BGR2GRAY known answers (0.114 B + 0.587 G + 0.299 R)
    assert np.allclose(ecc.warp_pos([10.0, 20.0], np.array([[1, 0, 2.5], [0, 1, -1.5]])), [12.5, 18.5])


@functools.lru_cache(maxsize=None)
def _free_run_oracle(name, motion):
    """The oracle with the reference's settings from the case's initial warp -> (rho, warp, corner distance to the truth)."""
    from oracle import ecc
    im1, im2, M, init = _case(name)
    rho, W = ecc.find_transform_ecc(ecc.bgr2gray(im1), ecc.bgr2gray(im2), warp=init, motion=motion)
    return rho, W, _corner_dist(W, M, im1.shape)


def _refused_inputs():
    """(frames, initial warp, what busca_ecc_align says) of the two refusals: no gradient anywhere; a warp that throws the
    whole frame out of the template."""
    im1, im2 = _case("120x160")[:2]
    flat = np.full((120, 160, 3), 100, np.uint8)
    return [(flat, flat, None, "singular Hessian"), (im1, im2, np.array([[1, 0, 10 * 160], [0, 1, 0]], np.float32), "overlap")]


def test_pair_default_cell_is_unchanged():
    """cell=8 is the generator the existing tests were written with: same bytes as its former fixed-cell form."""
    from scipy.ndimage import zoom
    im1 = _pair(H=24, W=40, seed=3)[0]
    rng = np.random.default_rng(3)
    for ch in range(3):
        big = zoom(rng.uniform(0, 255, (24 // 8 + 4, 40 // 8 + 4)), 8, order=3)[16:16 + 24, 16:16 + 40]
        assert np.array_equal(im1[..., ch], np.clip(big, 0, 255).astype(np.uint8))
    assert _pair(seed=1)[1].tobytes() == _pair(seed=1, cell=8)[1].tobytes()


def test_ecc_cases_are_well_posed():
    """Every case of the table, both motions, on the CPU: the oracle runs, ends above rho 0.8 and keeps more than 40 % of the
    frame under the mask (the two shifted cases less than 80 %, so their fringe is real).  One step of the kernel's
    formulation (_step_f64) from the oracle's previous iterate stays within a tenth of each bar of the oracle, so nine tenths
    of the bars are left to the kernel.  The same step with either deliberate error - fringe pixels dropped, clamped instead of
    reflected borders - leaves the bars, which is what makes test_ecc_step_matches_oracle able to fail.  (The clamped border
    moves rho by more than its bar everywhere but on the above-cap frame, where the border is 0.8 % of the pixels; it moves
    the warp by more than its bar there too.)"""
    from oracle import ecc
    g = ecc.bgr2gray(_case("9x13")[1])
    b, gx, gy = _prefilter(g, _reflect101)                     # the restatement's own pre-filter is the oracle's, bit for bit
    assert np.array_equal(b, ecc.blur5(g.astype(np.float32)))
    assert all(np.array_equal(x, y) for x, y in zip((gx, gy), ecc.gradients(b)))
    for name, motion in CASE_MOTIONS:
        trace = _trace(name, motion)                           # raises where the oracle does
        drho, dwarp, shares = _restatement_gaps(name, motion)
        _, fringe_warp, _ = _restatement_gaps(name, motion, drop_fringe=True)
        clamp_rho, clamp_warp, _ = _restatement_gaps(name, motion, border=_clamp)
        line = ("%-10s %-9s rho %.4f share %.3f..%.3f  formulations: rho %.2e warp %.2e  fringe dropped: warp %.2e  clamped: rho %.2e warp %.2e"
                % (name, motion, trace[-1][0], min(shares), max(shares), drho, dwarp, fringe_warp, clamp_rho, clamp_warp))
        print(line)
        assert len(trace) == CASES[name][8] and trace[-1][0] > 0.8, line
        assert min(shares) > 0.4 and (name not in SHIFTED or max(shares) < 0.8), line
        assert drho < RHO_BAR / 10 and dwarp < WARP_BAR / 10, line
        assert fringe_warp > WARP_BAR, line
        assert clamp_warp > WARP_BAR and (clamp_rho > RHO_BAR or name == "1025x1031"), line
    for name, rec in FREE_RUN.items():
        for motion, r in zip(BOTH, rec):
            rho, _, d = _free_run_oracle(name, motion)
            line = "%-10s %-9s free-running oracle: rho %.4f, corners and centre %.4f px from the truth (recorded %.4f)" % (name, motion, rho, d, r)
            print(line)
            assert rho > 0.8 and 0.5 * r <= d <= r, line             # FREE_RUN still says what the oracle does


def test_oracle_refuses_what_the_kernel_refuses():
    """Constant frames and a warp without overlap: the oracle raises on both (test_ecc_refusals is the GPU side)."""
    import warnings
    from oracle import ecc
    for prev, cur, init, _ in _refused_inputs():
        for motion in BOTH:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")                # mean of an empty slice, on the way to the exception
                with pytest.raises((RuntimeError, np.linalg.LinAlgError)):
                    ecc.find_transform_ecc(ecc.bgr2gray(prev), ecc.bgr2gray(cur), warp=init, motion=motion)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _bits(cc, W, iters=None):
    return np.float64(cc).tobytes() + np.asarray(W, np.float32).tobytes() + (b"" if iters is None else bytes([iters]))


def _gpu_steps(name, motion, ctx=None, steps=None):
    """One kernel iteration from each of the oracle's iterates; prints the gaps, then holds them to the bars."""
    from busca_amd import tracking
    im1, im2 = (_dev(a) for a in _case(name)[:2])
    gaps = []
    for k, (rho_k, W_k) in enumerate(_trace(name, motion)[:steps], 1):
        cc, W = tracking.find_transform_ecc(im1, im2, warp_matrix=_start(name, motion, k), motion="MOTION_" + motion.upper(),
                                            number_of_iterations=1, termination_eps=-1.0, ctx=ctx)
        gaps.append((abs(cc - rho_k), float(np.abs(W - W_k).max()), tracking.find_transform_ecc.last_iterations))
    print("ECC step gaps %-10s %-9s rho %.2e warp %.2e" % (name, motion, max(g[0] for g in gaps), max(g[1] for g in gaps)))
    for k, (drho, dwarp, its) in enumerate(gaps, 1):
        assert drho < RHO_BAR and dwarp < WARP_BAR and its == 1, (name, motion, k, drho, dwarp, its)


@pytest.mark.gpu
@pytest.mark.parametrize("name,motion", CASE_MOTIONS, ids=["%s-%s" % nm for nm in CASE_MOTIONS])
def test_ecc_step_matches_oracle(name, motion):
    """Step by step from the oracle's own iterates (module docstring), at the shapes of CASES: rho within 1e-5, every warp entry
    within 2e-5, one iteration run."""
    _gpu_steps(name, motion)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", MOTIONS)
def test_ecc_matches_oracle(motion):
    """Iterate by iterate: after k = 1..6 iterations (termination test off) the kernel's warp and correlation coefficient equal
    the oracle's to float32 round-off.  The free-running call (eps 1e-5, <= 100 iterations, the reference's settings) is then
    compared on what matters - where the warp sends points - because near the optimum the rho increments hover around the
    termination threshold and round-off decides at which iteration the loop stops (and, for the affine model on a
    near-identity pair, the iterates themselves separate after ~20 iterations)."""
    from busca_amd import tracking
    from oracle import ecc
    pts = np.array([[x, y, 1.0] for x in (0, 80, 159) for y in (0, 60, 119)]).T
    for seed, (th, tx, ty) in enumerate([(0.01, 2.3, -1.4), (-0.02, -3.1, 0.8), (0.0, 0.4, 0.2)]):
        im1, im2, M = _pair(th=th, tx=tx, ty=ty, seed=seed)
        g1, g2 = ecc.bgr2gray(im1), ecc.bgr2gray(im2)
        _, _, trace = ecc.find_transform_ecc(g1, g2, motion=motion[7:].lower(), iters=6, eps=-1.0, return_trace=True)
        for k in (1, 2, 4, 6):
            cc, W = tracking.find_transform_ecc(im1, im2, motion=motion, number_of_iterations=k, termination_eps=-1.0)
            rho_k, W_k = trace[k - 1]
            assert tracking.find_transform_ecc.last_iterations == k
            assert abs(cc - rho_k) < 1e-5, (seed, k, cc, rho_k)
            assert np.abs(W - W_k).max() < 2e-5, (seed, k, np.abs(W - W_k).max())
        cc, W = tracking.find_transform_ecc(im1, im2, motion=motion)                  # the reference's settings
        rho, Wo = ecc.find_transform_ecc(g1, g2, motion=motion[7:].lower())
        assert cc > 0.99 and rho > 0.99
        lim = 0.1 if motion == "MOTION_EUCLIDEAN" else 0.25
        assert np.abs(W.astype(np.float64) @ pts - M @ pts).max() < lim               # both sit on the true transform
        assert np.abs(Wo.astype(np.float64) @ pts - M @ pts).max() < lim


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FREE_RUN))
def test_ecc_free_running_on_edge_shapes(name):
    """The reference's settings (eps 1e-5, <= 100 iterations) from the case's initial warp.  Kernel and oracle are compared on
    where their final warp sends the frame's corners and centre, against the true transform.  The limit is twice the oracle's
    own distance to the truth as measured on the CPU (FREE_RUN, checked by test_ecc_cases_are_well_posed), 0.1 px at least:
                 euclidean   affine      limits
      67x301     0.0021 px   0.0164 px   0.1 / 0.1 px
      259x33     0.0201 px   0.0253 px   0.1 / 0.1 px
      shift27    0.0074 px   0.0111 px   0.1 / 0.1 px
      shift38    0.0355 px   0.0503 px   0.1 / 0.1006 px
    (figures rounded up in the fourth decimal.)"""
    from busca_amd import tracking
    im1, im2, M, init = _case(name)
    for motion, rec in zip(BOTH, FREE_RUN[name]):
        lim = max(2 * rec, 0.1)
        cc, W = tracking.find_transform_ecc(_dev(im1), _dev(im2), warp_matrix=init, motion="MOTION_" + motion.upper())
        rho, _, d_oracle = _free_run_oracle(name, motion)
        d = _corner_dist(W, M, im1.shape)
        print("ECC free-running %-8s %-9s kernel %.4f px (cc %.5f, %d iterations), oracle %.4f px (rho %.5f), limit %.3f px"
              % (name, motion, d, cc, tracking.find_transform_ecc.last_iterations, d_oracle, rho, lim))
        assert cc > 0.8 and rho > 0.8                          # the bar of test_ecc_cases_are_well_posed
        assert d < lim and d_oracle < lim, (name, motion, d, d_oracle, lim)


def _align_abi(ctx, prev, cur, H, W, stride_prev, stride_cur, motion, iters=6, eps=-1.0, warp=None):
    """busca_ecc_align itself on device buffers -> (rc, cc, warp, iterations)."""
    import torch
    warp = np.eye(2, 3, dtype=np.float32) if warp is None else warp
    cc, its = C.c_double(-7.0), C.c_int32(-7)
    torch.cuda.synchronize()
    rc = ctx.lib.busca_ecc_align(ctx.h, None if prev is None else prev.data_ptr(), None if cur is None else cur.data_ptr(), H, W,
                                 stride_prev, stride_cur, motion, iters, eps, None if warp is False else warp.ctypes.data,
                                 C.byref(cc), C.byref(its), None)
    return rc, cc.value, warp, its.value


@pytest.mark.gpu
def test_ecc_row_strides():
    """Frames inside wider byte buffers (row strides 3 W + 5 and 3 W + 64, padding 255) give the bits of the contiguous call:
    through the C ABI, which takes the two strides, and through the Python mirror, which makes its own contiguous copy of a
    column slice."""
    import torch
    from busca_amd import _lib, tracking
    im1, im2 = _case("67x301")[:2]
    H, W = im1.shape[:2]
    ctx = _lib.Context(0)
    padded = []
    for im, stride in ((im1, 3 * W + 5), (im2, 3 * W + 64)):
        buf = torch.full((H, stride), 255, dtype=torch.uint8, device="cuda")
        buf[:, :3 * W] = _dev(im.reshape(H, 3 * W))
        padded.append((buf, stride))
    wide = [torch.full((H, W + 7, 3), 255, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for w, im in zip(wide, (im1, im2)):
        w[:, 3:3 + W] = _dev(im)
    views = [w[:, 3:3 + W] for w in wide]
    assert not views[0].is_contiguous() and views[0].stride(0) == 3 * (W + 7)
    for motion in (0, 1):
        rc, cc, warp, its = _align_abi(ctx, _dev(im1), _dev(im2), H, W, 3 * W, 3 * W, motion)
        assert rc == 0 and its == 6 and cc > 0.9
        rc2, cc2, warp2, its2 = _align_abi(ctx, padded[0][0], padded[1][0], H, W, padded[0][1], padded[1][1], motion)
        assert rc2 == 0 and _bits(cc2, warp2, its2) == _bits(cc, warp, its), (motion, cc, cc2, warp, warp2)
        cc3, warp3 = tracking.find_transform_ecc(views[0], views[1], motion=MOTIONS[motion], number_of_iterations=6, termination_eps=-1.0, ctx=ctx)
        assert _bits(cc3, warp3, tracking.find_transform_ecc.last_iterations) == _bits(cc, warp, its), (motion, cc, cc3, warp, warp3)
    ctx.close()


@pytest.mark.gpu
def test_ecc_deterministic_across_workspace_reuse():
    """One context, sizes small - taller - above the block cap - small - taller (the cached workspace grows twice, then is reused
    by smaller frames), each call twice in a row: every repeat of a size returns the bits of its first run, and a second
    fresh context returns them too."""
    from busca_amd import _lib, tracking
    order = ["24x40", "259x33", "1025x1031", "24x40", "259x33"]
    frames = {n: [_dev(a) for a in _case(n)[:2]] for n in set(order)}

    def run(ctx, name, motion):
        cc, W = tracking.find_transform_ecc(*frames[name], motion=motion, number_of_iterations=6, termination_eps=-1.0, ctx=ctx)
        assert tracking.find_transform_ecc.last_iterations == 6 and cc > 0.9
        return _bits(cc, W)
    ctx, first = _lib.Context(0), {}
    for name in order:
        for _ in range(2):
            for motion in MOTIONS:
                assert first.setdefault((name, motion), run(ctx, name, motion)) == run(ctx, name, motion), (name, motion)
    ctx.close()
    ctx2 = _lib.Context(0)
    for name in order[:3]:
        for motion in MOTIONS:
            assert run(ctx2, name, motion) == first[name, motion], (name, motion)
    ctx2.close()


@pytest.mark.gpu
def test_ecc_refusals():
    """The exits of the host loop and the argument checks.  Constant frames have no gradient (singular Hessian); a warp that
    sends every pixel outside leaves nothing under the mask (no overlap) - OpenCV raises on both, the oracle does
    (test_oracle_refuses_what_the_kernel_refuses), the library returns EINVAL with a message and the context goes on working.
    A bad argument returns EINVAL before any launch and leaves the caller's warp alone."""
    import torch
    from busca_amd import _lib, tracking
    ctx = _lib.Context(0)
    for prev, cur, init, says in _refused_inputs():
        for motion in BOTH:
            with pytest.raises(_lib.BuscaError, match=says):
                tracking.find_transform_ecc(_dev(prev), _dev(cur), warp_matrix=init, motion="MOTION_" + motion.upper(), ctx=ctx)
            _gpu_steps("120x160", motion, ctx=ctx)
    frame = torch.full((16, 16, 3), 100, dtype=torch.uint8, device="cuda")
    ok = dict(prev=frame, cur=frame, H=16, W=16, stride_prev=48, stride_cur=48, motion=0, iters=5)
    bad = [dict(H=7), dict(W=7), dict(stride_prev=3 * 16 - 1), dict(iters=0), dict(motion=2), dict(prev=None), dict(cur=None), dict(warp=False)]
    for kw in bad:
        sentinel = np.array([[9, 8, 7], [6, 5, 4]], np.float32)
        rc, cc, warp, its = _align_abi(ctx, **{**ok, "warp": sentinel, **kw})
        assert rc == -1 and (cc, its) == (-7.0, -7), kw
        assert ctx.lib.busca_last_error(ctx.h).decode().startswith("busca_ecc_align"), kw
        assert np.array_equal(sentinel, np.array([[9, 8, 7], [6, 5, 4]], np.float32)), kw
    _gpu_steps("120x160", "euclidean", ctx=ctx, steps=1)
    ctx.close()


@pytest.mark.gpu
def test_ecc_full_hd_and_track_update():
    """1080p frames; tracks are moved like STrack.apply_camera_motion does (byte_tracker.py:123-137)."""
    import types
    from busca_amd import tracking
    im1, im2, M = _pair(H=1080, W=1920, th=0.004, tx=5.5, ty=-2.25, seed=3)
    trk = [types.SimpleNamespace(mean=np.array([400.0, 300.0, 0.4, 200.0, 0, 0, 0, 0]), _tlwh=np.zeros(4), scale=1.0),
           types.SimpleNamespace(mean=None, _tlwh=np.array([100.0, 50.0, 40.0, 90.0]), scale=2.0)]
    cc = tracking.camera_motion_compensation(trk, im1, im2, frame_id=5)
    assert cc > 0.98
    want0 = M @ np.array([400.0, 300.0, 1.0])
    want1 = (M @ np.array([200.0, 100.0, 1.0])) / 2.0
    assert np.abs(trk[0].mean[:2] - want0).max() < 0.2 and np.abs(trk[1]._tlwh[:2] - want1).max() < 0.2
    assert tracking.camera_motion_compensation(trk, None, im2, frame_id=1) == 1.0            # first frame: nothing to align
    with pytest.raises(ValueError):
        tracking.find_transform_ecc(im1, im2, motion="MOTION_HOMOGRAPHY")
