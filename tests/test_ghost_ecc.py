"""GHOST's camera-motion estimate on the device: busca_ecc_gauss_taps / busca_ecc_prepare / busca_ecc_align_planes (include/busca_ecc.h) and
their mirrors in busca_amd.tracking (find_transform_ecc_f32, GhostCameraMotion, ghost_motion_compensation, ghost_ecc_check_config).

The checker is tests/ghost_ecc_ref.py, a numpy restatement on top of oracle/ecc.py (parity with the real cv2 is unpinned: see its header).  No
golden file: there is no reference output to record.
  * planes: bit for bit against the restatement's blurred grey (the restatement uses the library's own taps, which the CPU test holds to the
    closed form).
  * anchor: on K = 5 one-channel planes of oracle.ecc.bgr2gray values busca_ecc_align_planes returns the bits of busca_ecc_align on the BGR frames -
    same kernels, same host loop -, which ties the new host code to what tests/test_ecc.py holds to the oracle.
  * steps: the design of tests/test_ecc.py::test_ecc_step_matches_oracle and its two bars, |rho| 1e-5 and |dW| 2e-5: ONE iteration from each of the
    restatement's own iterates.  `_step_f64` restates the kernel's formulation (float64 sums, ip / tp / ep by linearity) in numpy; the CPU test
    holds its gap to the restatement below a quarter of each bar for every case, so three quarters are left to the kernel's summation order.
  * free-running: only cases whose outcome is insensitive - on the CPU the restatement fed planes scaled by 1 and by 255 stops after the same
    number of iterations with warps within 1e-5 of each other (FREE_RUN; test_cases_are_well_posed checks that this still holds).
Frames are smooth random float RGB in [0, 1] moved by a known transform, feature cells of 8 - 16 pixels: a 15-pixel blur flattens anything finer.
At 8x8 and 9x13 the blurred plane is close to a ramp and most images are ill posed (the Hessian of the 6-parameter model is singular, or the
iteration leaves the frame); the seeds of those two rows were searched for on the CPU (80 seeds x 2 shifts at 8x8) until all three motions ran."""
import ctypes as C
import functools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from tests import ghost_ecc_ref as ref
from tests.test_streams_gpu import behind, busy, ctx  # noqa: F401  (busy, ctx: fixtures)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO_BAR, WARP_BAR = 1e-5, 2e-5            # tests/test_ecc.py's
NAMES = {"busca_ecc_gauss_taps": 2, "busca_ecc_prepare": 11, "busca_ecc_align_planes": 12}
GHOST_NAME = {"euclidean": "Euclidean", "affine": "Affine", "translation": "Translation"}

# name -> H, W, theta, tx, ty, seed, cell, steps.  What each reaches: K / 2 = 7 reflected pixels touch the far edge at 8 (the smallest the ABI takes
# at K = 15); the reductions use one block up to 1024 pixels and two from 1025; the 2-D grids and the LDS row tile get a second x-block at W = 257,
# whose halo crosses the tile edge; 259x33 is tall and narrow; 1080x1920 is the frame of the reference, two iterations only.
CASES = {
    "8x8": (8, 8, 0.0, 0.05, 0.04, 54, 8, 6),
    "9x13": (9, 13, 0.0, 0.1, -0.08, 10, 8, 6),
    "32x32": (32, 32, 0.004, 0.7, -0.6, 11, 8, 6),
    "25x41": (25, 41, -0.004, -0.6, 0.7, 12, 8, 6),
    "24x256": (24, 256, 0.002, 0.8, -0.6, 13, 12, 6),
    "24x257": (24, 257, 0.002, 0.8, -0.6, 13, 12, 6),
    "259x33": (259, 33, 0.004, -0.8, 1.2, 3, 12, 6),
    "120x160": (120, 160, 0.01, 2.3, -1.4, 0, 16, 6),
}
FULL_HD = ("1080x1920", (1080, 1920, 0.004, 5.5, -2.25, 3, 16, 2))
CASE_MOTIONS = [(n, m) for n in CASES for m in ref.MOTIONS]
# (case, motion) -> iterations the restatement runs with the reference's settings (eps 1e-5, <= 100 iterations), the same at input scales 1 and 255
FREE_RUN = {("32x32", "euclidean"): 5, ("259x33", "euclidean"): 5, ("25x41", "euclidean"): 7, ("120x160", "translation"): 3, ("32x32", "translation"): 9}


def _pair(H, W, th, tx, ty, seed, cell):
    """Smooth random float32 RGB [3,H,W] in [0, 1] and a copy moved by a known Euclidean transform: a(x) ~ b(M x)."""
    from scipy.ndimage import affine_transform, zoom
    rng = np.random.default_rng(seed)
    c, s = np.cos(th), np.sin(th)
    Ainv = np.linalg.inv(np.array([[c, -s], [s, c]]))
    R = np.array([[Ainv[1, 1], Ainv[1, 0]], [Ainv[0, 1], Ainv[0, 0]]])
    off = -(R @ np.array([ty, tx]))
    a, b = [], []
    for _ in range(3):
        big = zoom(rng.uniform(0, 1, (H // cell + 4, W // cell + 4)), cell, order=3)[2 * cell:2 * cell + H, 2 * cell:2 * cell + W]
        a.append(np.clip(big, 0, 1))
        b.append(np.clip(affine_transform(big, R, offset=off, order=3, mode="nearest"), 0, 1))
    return np.stack(a).astype(np.float32), np.stack(b).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (current frame = template, previous frame = input), float32 [3,H,W]; computed once, shared, never written to."""
    cur, prev = _pair(*(dict(CASES, **dict([FULL_HD]))[name][:7]))
    cur.setflags(write=False)
    prev.setflags(write=False)
    return cur, prev


@functools.lru_cache(maxsize=None)
def _taps(K):
    """busca_ecc_gauss_taps (host only)."""
    from busca_amd import _lib
    t = np.full(K, np.nan, np.float32)
    assert _lib.load().busca_ecc_gauss_taps(K, t.ctypes.data) == 0
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _planes(name, K=15):
    """The restatement's blurred grey planes of the case's two frames, with the library's taps."""
    out = tuple(ref.prepare(f, _taps(K)) for f in _case(name))
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _trace(name, motion):
    """The restatement's iterates at K = 15 with the termination test off: [(rho_k, W_k)], k = 1..steps.  Warnings are errors: a mean over an empty
    mask is a case that is not well posed."""
    T, I = _planes(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return ref.align_planes(T, I, motion=motion, iters=dict(CASES, **dict([FULL_HD]))[name][7], eps=-1.0, return_trace=True)[2]


def _start(name, motion, k):
    return _trace(name, motion)[k - 2][1] if k > 1 else np.eye(2, 3, dtype=np.float32)


def _step_f64(T, I, gx, gy, M, motion):
    """One iteration as ecc_iter_kernel<P> + the host loop do it (tests/test_ecc.py::_step_f64, with the Jacobian of `motion`) -> (rho, new warp)."""
    from oracle import ecc
    H, W = T.shape
    M = np.array(M, np.float32).reshape(2, 3)
    co = ecc.warp_coords(M, H, W)
    mask = ecc.warp_mask_nearest(co, H, W)
    Iw, gxw, gyw = (ecc.warp_linear(a, co) for a in (I, gx, gy))
    Xg, Yg = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    J = [j.astype(np.float32).astype(np.float64) for j in ref.jacobian(motion, gxw, gyw, M, Xg, Yg)]
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
    if motion == "translation":
        M[0, 2] += dp[0]; M[1, 2] += dp[1]
    elif motion == "euclidean":
        th = np.float32(np.arcsin(M[1, 0])) + dp[0]
        M[0, 2] += dp[1]; M[1, 2] += dp[2]
        M[0, 0] = M[1, 1] = np.float32(np.cos(th)); M[1, 0] = np.float32(np.sin(th)); M[0, 1] = -M[1, 0]
    else:
        M[0, 0] += dp[0]; M[1, 0] += dp[1]; M[0, 1] += dp[2]; M[1, 1] += dp[3]; M[0, 2] += dp[4]; M[1, 2] += dp[5]
    return float(rho), M


def _u8_planes(name):
    """One-channel float planes holding oracle.ecc.bgr2gray values of a BGR pair of tests/test_ecc.py -> (frames, prev plane, cur plane)."""
    from oracle import ecc
    from tests import test_ecc as u8
    im1, im2 = u8._case(name)[:2]
    return (im1, im2), ecc.bgr2gray(im1).astype(np.float32), ecc.bgr2gray(im2).astype(np.float32)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_gauss_taps():
    """busca_ecc_gauss_taps is cv::getGaussianKernel(K, sigma <= 0, CV_32F): the fixed tables up to 7, the closed form beyond."""
    from busca_amd import _lib
    assert np.array_equal(_taps(5), np.array([1, 4, 6, 4, 1], np.float32) / np.float32(16))
    for K, tab in ref.SMALL_TAPS.items():
        assert np.array_equal(_taps(K), np.array(tab, np.float32)), K
    for K in (9, 15, 31):
        t, want = _taps(K), ref.gauss_taps(K)
        assert np.array_equal(t, t[::-1]), K
        assert abs(t.astype(np.float64).sum() - 1.0) <= np.spacing(np.float32(1)), K
        assert np.all(np.abs(t.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)), (K, t, want)
    lib, buf = _lib.load(), np.zeros(40, np.float32)
    for K in (0, -1, 2, 4, 16, 33):
        assert lib.busca_ecc_gauss_taps(K, buf.ctypes.data) == -1, K
    assert lib.busca_ecc_gauss_taps(5, None) == -1 and not buf.any()


def test_restatement_at_k5_is_the_oracle():
    """One-channel planes of bgr2gray values, K = 5, the first argument as template: the restatement returns the trace of oracle.ecc.find_transform_ecc bit
    for bit - through the oracle's loop (Euclidean, affine) and through the restatement's own loop, which translation needs."""
    from oracle import ecc
    assert np.array_equal(ref.gauss_taps(5), _taps(5))
    for name in ("24x40", "9x13"):
        _, g1, g2 = _u8_planes(name)
        assert np.array_equal(ref.blur(g1, _taps(5)), ecc.blur5(g1))
        for motion in ("euclidean", "affine"):
            want = ecc.find_transform_ecc(g1.astype(np.uint8), g2.astype(np.uint8), motion=motion, iters=6, eps=-1.0, return_trace=True)
            got = ref.find_transform_ecc(g1, g2, motion=motion, K=5, iters=6, eps=-1.0, return_trace=True, taps=_taps(5))
            own = ref.align_planes(ref.prepare(g1, _taps(5)), ref.prepare(g2, _taps(5)), motion=motion, iters=6, eps=-1.0, return_trace=True, own_loop=True)
            for r in (got, own):
                assert len(r[2]) == 6 and r[0] == want[0] and np.array_equal(r[1], want[1])
                assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(r[2], want[2])), (name, motion)
    rgb = _case("9x13")[0]
    assert np.array_equal(ref.gray_f32(rgb[0]), rgb[0])                       # one channel: the plane is the grey
    r, g, b = (np.float32(v) for v in (0.25, 0.5, 0.75))
    assert ref.gray_f32(np.array([r, g, b], np.float32).reshape(3, 1, 1))[0, 0] == (r * np.float32(0.299) + g * np.float32(0.587)) + b * np.float32(0.114)


def test_cases_are_well_posed():
    """Every case x motion on the CPU: the restatement runs its steps without raising (and without a warning), every rho is finite, so the start
    iterates of the step tests exist; one step of the kernel's formulation (_step_f64) from each of them stays within a quarter of each bar.  The
    free-running cases stop after the recorded number of iterations at input scales 1 and 255, within 1e-5 of each other."""
    from oracle import ecc
    for name, motion in CASE_MOTIONS + [(FULL_HD[0], "euclidean")]:
        T, I = _planes(name)
        gx, gy = ecc.gradients(I)
        trace = _trace(name, motion)
        steps = dict(CASES, **dict([FULL_HD]))[name][7]
        drho = dwarp = 0.0
        for k, (rho_k, W_k) in enumerate(trace, 1):
            rho, Wn = _step_f64(T, I, gx, gy, _start(name, motion, k), motion)
            drho, dwarp = max(drho, abs(rho - rho_k)), max(dwarp, float(np.abs(Wn - W_k).max()))
        line = "%-9s %-11s rho %.4f .. %.4f  formulations: rho %.2e warp %.2e" % (name, motion, trace[0][0], trace[-1][0], drho, dwarp)
        print(line)
        assert len(trace) == steps and all(np.isfinite(r) and np.isfinite(W).all() for r, W in trace), line
        assert drho < RHO_BAR / 4 and dwarp < WARP_BAR / 4, line
    for (name, motion), its in FREE_RUN.items():
        T, I = _planes(name)
        runs = [ref.align_planes(T * np.float32(sc), I * np.float32(sc), motion=motion, return_trace=True) for sc in (1.0, 255.0)]
        line = "%-9s %-11s free-running: %d / %d iterations, warps %.2e apart, rho %.2e" % (
            name, motion, len(runs[0][2]), len(runs[1][2]), np.abs(runs[0][1] - runs[1][1]).max(), abs(runs[0][0] - runs[1][0]))
        print(line)
        assert len(runs[0][2]) == len(runs[1][2]) == its, line
        assert np.abs(runs[0][1] - runs[1][1]).max() < 1e-5 and abs(runs[0][0] - runs[1][0]) < 1e-5, line


def test_config_refusals():
    from busca_amd import tracking
    cfg = {"num_iter_mc": 100, "termination_eps_mc": 1e-5}
    assert [tracking.ghost_ecc_check_config(dict(cfg, warp_mode=m)) for m in ("Euclidean", "Affine", "Translation")] == [0, 1, 2]
    with pytest.raises(ValueError, match="3-row"):
        tracking.ghost_ecc_check_config(dict(cfg, warp_mode="Homography"))
    with pytest.raises(KeyError):
        tracking.ghost_ecc_check_config(dict(cfg, warp_mode="Similarity"))
    with pytest.raises(KeyError):
        tracking.ghost_ecc_check_config(cfg)
    for bad in (dict(cfg, warp_mode="Homography"), dict(cfg, warp_mode="euclidean")):           # refused before a context is made
        with pytest.raises((ValueError, KeyError)):
            tracking.GhostCameraMotion(bad)
    for size in (0, 4, 33):
        with pytest.raises(ValueError, match="gauss_size"):
            tracking.GhostCameraMotion(dict(cfg, warp_mode="Euclidean"), gauss_size=size)
    with pytest.raises(ValueError):
        tracking.find_transform_ecc_f32(None, None, motion="MOTION_HOMOGRAPHY")


def test_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_ecc.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr)) == set(NAMES) == set(_lib.ECC_SIGNATURES)
    for header, table in _lib.HEADERS.items():
        if header == "busca_ecc.h":
            continue
        assert not set(NAMES) & set(table)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert set(NAMES) <= exported
    lib = _lib.load()
    for name, nargs in NAMES.items():
        fn = getattr(lib, name)
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert fn.restype is not None and len(fn.argtypes) == nargs == len(_lib.ECC_SIGNATURES[name][1]) == decl.count(",") + 1, name
    assert lib.busca_version() == 2006
    assert (_lib.ECC_KSIZE_MAX, _lib.ECC_EUCLIDEAN, _lib.ECC_AFFINE, _lib.ECC_TRANSLATION) == tuple(
        int(re.search(r"#define %s (\d+)" % n, hdr).group(1)) for n in ("BUSCA_ECC_KSIZE_MAX", "BUSCA_ECC_EUCLIDEAN", "BUSCA_ECC_AFFINE", "BUSCA_ECC_TRANSLATION"))


def test_mirrors_reachable_from_the_alias_package():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.tracking as bt
        from busca_amd import tracking
        for n in ("ghost_ecc_check_config", "GhostCameraMotion", "ghost_motion_compensation", "find_transform_ecc_f32"):
            assert getattr(bt, n) is getattr(tracking, n)
    finally:
        sys.path.pop(0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _bits(cc, W, iters):
    return np.float64(cc).tobytes() + np.asarray(W, np.float32).tobytes() + int(iters).to_bytes(4, "little")


def _prepare_abi(ctx, t, channels, H, W, strides, K, out=None):
    """busca_ecc_prepare itself -> (rc, plane as numpy)."""
    import torch
    out = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda") if out is None else out
    rc = ctx.lib.busca_ecc_prepare(ctx.h, None if t is None else t.data_ptr(), channels, H, W, strides[0], strides[1], strides[2], K,
                                   None if out is False else out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, (None if out is False else out.cpu().numpy())


@gpu
@pytest.mark.parametrize("name", list(CASES) + [FULL_HD[0]])
def test_prepare_matches_restatement_bit_for_bit(ctx, name):
    """busca_ecc_prepare against the restatement's blurred grey at K = 5 and K = 15: a contiguous [3,H,W] frame, an [H,W,3] frame viewed as [3,H,W], a crop
    out of a larger frame (padding NaN: a read outside the view would show), and the first channel alone as a one-channel plane."""
    import torch
    cur = _case(name)[0]
    H, W = cur.shape[1:]
    hwc = _dev(np.ascontiguousarray(cur.transpose(1, 2, 0))).permute(2, 0, 1)
    assert not hwc.is_contiguous() and hwc.stride() == (1, 3 * W, 3)
    wide = torch.full((3, H + 5, W + 9), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, 2:2 + H, 4:4 + W] = _dev(cur)
    crop = wide[:, 2:2 + H, 4:4 + W]
    for K in (5, 15):
        want3, want1 = ref.prepare(cur, _taps(K)), ref.prepare(cur[0], _taps(K))
        for what, t in (("contiguous", _dev(cur)), ("permuted", hwc), ("cropped", crop)):
            rc, got = _prepare_abi(ctx, t, 3, H, W, t.stride(), K)
            assert rc == 0 and np.array_equal(got, want3), (name, K, what, np.abs(got - want3).max())
        for what, t in (("plane", _dev(cur[0])), ("cropped plane", crop[0])):
            rc, got = _prepare_abi(ctx, t, 1, H, W, (0,) + tuple(t.stride()), K)
            assert rc == 0 and np.array_equal(got, want1), (name, K, what, np.abs(got - want1).max())


@gpu
@pytest.mark.parametrize("name", ["24x40", "120x160"])
def test_align_planes_has_the_bits_of_busca_ecc_align(ctx, name):
    """K = 5 one-channel planes of bgr2gray values, the previous frame as template (the roles of busca_ecc_align), free-running with the reference's
    settings: warp, cc and iteration count of busca_ecc_align on the BGR frames, bit for bit."""
    from busca_amd import tracking
    (im1, im2), g1, g2 = _u8_planes(name)
    for m, motion in enumerate(("MOTION_EUCLIDEAN", "MOTION_AFFINE")):
        cc, W = tracking.find_transform_ecc(_dev(im1), _dev(im2), motion=motion, ctx=ctx)
        its = tracking.find_transform_ecc.last_iterations
        cc2, W2 = tracking.find_transform_ecc_f32(_dev(g1), _dev(g2), motion=motion, gauss_size=5, ctx=ctx)
        assert its > 1 and _bits(cc2, W2, tracking.find_transform_ecc_f32.last_iterations) == _bits(cc, W, its), (name, motion, cc, cc2, W, W2)


def _gpu_steps(ctx, name, motion, steps=None):
    """One kernel iteration from each of the restatement's iterates; prints the gaps, then holds them to the bars."""
    from busca_amd import tracking
    cur, prev = (_dev(f) for f in _case(name))
    gaps = []
    for k, (rho_k, W_k) in enumerate(_trace(name, motion)[:steps], 1):
        cc, W = tracking.find_transform_ecc_f32(cur, prev, warp_matrix=_start(name, motion, k), motion=GHOST_NAME[motion], number_of_iterations=1,
                                                termination_eps=-1.0, ctx=ctx)
        gaps.append((abs(cc - rho_k), float(np.abs(W - W_k).max()), tracking.find_transform_ecc_f32.last_iterations))
    print("GHOST ECC step gaps %-9s %-11s rho %.2e warp %.2e" % (name, motion, max(g[0] for g in gaps), max(g[1] for g in gaps)))
    for k, (drho, dwarp, its) in enumerate(gaps, 1):
        assert drho < RHO_BAR and dwarp < WARP_BAR and its == 1, (name, motion, k, drho, dwarp, its)


@gpu
@pytest.mark.parametrize("name,motion", CASE_MOTIONS, ids=["%s-%s" % nm for nm in CASE_MOTIONS])
def test_step_matches_restatement(ctx, name, motion):
    """Step by step from the restatement's own iterates at K = 15: rho within 1e-5, every warp entry within 2e-5, one iteration run."""
    _gpu_steps(ctx, name, motion)


@gpu
def test_full_hd_two_iterations(ctx):
    """One 1080x1920 call of two iterations (Euclidean, identity start) against the restatement's second iterate, same bars."""
    from busca_amd import tracking
    name = FULL_HD[0]
    cur, prev = (_dev(f) for f in _case(name))
    cc, W = tracking.find_transform_ecc_f32(cur, prev, motion="Euclidean", number_of_iterations=2, termination_eps=-1.0, ctx=ctx)
    rho, W2 = _trace(name, "euclidean")[1]
    print("GHOST ECC 1080p: rho gap %.2e warp gap %.2e" % (abs(cc - rho), np.abs(W - W2).max()))
    assert tracking.find_transform_ecc_f32.last_iterations == 2
    assert abs(cc - rho) < RHO_BAR and np.abs(W - W2).max() < WARP_BAR


@gpu
@pytest.mark.parametrize("name,motion", list(FREE_RUN), ids=["%s-%s" % nm for nm in FREE_RUN])
def test_free_running(ctx, name, motion):
    """The reference's settings (eps 1e-5, <= 100 iterations) on the cases whose outcome is insensitive (FREE_RUN): the same iteration count as the
    restatement, rho within 1e-5, warp within 2e-5."""
    from busca_amd import tracking
    cur, prev = (_dev(f) for f in _case(name))
    cc, W = tracking.find_transform_ecc_f32(cur, prev, motion=GHOST_NAME[motion], ctx=ctx)
    T, I = _planes(name)
    rho, Wr, trace = ref.align_planes(T, I, motion=motion, return_trace=True)
    its = tracking.find_transform_ecc_f32.last_iterations
    print("GHOST ECC free-running %-9s %-11s %d iterations (restatement %d), rho gap %.2e warp gap %.2e" % (name, motion, its, len(trace), abs(cc - rho), np.abs(W - Wr).max()))
    assert its == len(trace) == FREE_RUN[name, motion]
    assert abs(cc - rho) < RHO_BAR and np.abs(W - Wr).max() < WARP_BAR


@functools.lru_cache(maxsize=None)
def _sequence(n=6, H=48, W=64, cell=12, seed=21):
    """n frames [3,H,W] of one smooth scene under a camera that drifts by (0.7, -0.4) pixels a frame."""
    from scipy.ndimage import shift, zoom
    rng = np.random.default_rng(seed)
    big = [zoom(rng.uniform(0, 1, (H // cell + 6, W // cell + 6)), cell, order=3) for _ in range(3)]
    frames = [np.stack([np.clip(shift(b, (-0.4 * i, 0.7 * i), order=3, mode="nearest")[2 * cell:2 * cell + H, 2 * cell:2 * cell + W], 0, 1) for b in big]).astype(np.float32)
              for i in range(n)]
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


CFG = {"warp_mode": "Euclidean", "num_iter_mc": 100, "termination_eps_mc": 1e-5}


def _stateless(ctx, cur, prev, cfg=CFG):
    from busca_amd import tracking
    cc, W = tracking.find_transform_ecc_f32(cur, prev, motion=cfg["warp_mode"], number_of_iterations=cfg["num_iter_mc"], termination_eps=cfg["termination_eps_mc"], ctx=ctx)
    return cc, W, tracking.find_transform_ecc_f32.last_iterations


@gpu
def test_camera_motion_reuses_the_prepared_plane(ctx):
    """GhostCameraMotion over five frames = the stateless call on the same pairs, bit for bit, with five prepares; device and host frames alike.  A
    constant frame (a template without variance: rho is NaN, BuscaError where OpenCV raises) leaves the stored plane and the context usable: the next good frame pairs
    with the frame before the bad one.  reset() makes the next frame a first frame; a frame of another size is refused."""
    import torch
    from busca_amd import _lib, tracking
    frames = _sequence()
    cam = tracking.GhostCameraMotion(CFG, ctx=ctx)
    assert cam.estimate(_dev(frames[0])) is None and cam.norm is None and cam.prepared == 1
    for i in range(1, 5):
        W = cam.estimate(_dev(frames[i]) if i % 2 else frames[i].copy())       # a host array goes through pinned staging
        cc, Ws, its = _stateless(ctx, _dev(frames[i]), _dev(frames[i - 1]))
        assert W.dtype == np.float32 and W.shape == (2, 3) and its > 1
        assert _bits(cam.cc, W, cam.iterations) == _bits(cc, Ws, its), (i, W, Ws)
        assert cam.norm.dtype == np.float32 and cam.norm == np.linalg.norm(W[:, -1])
        assert abs(W[0, 2] + 0.7) < 0.1 and abs(W[1, 2] - 0.4) < 0.1, W       # the template is the current frame: the warp leads back to the previous one
    assert cam.prepared == 5
    with pytest.raises(_lib.BuscaError, match="NaN encountered"):                # the constant frame is the template: zero variance, rho = 0 / 0
        cam.estimate(torch.full((3, 48, 64), 0.5, dtype=torch.float32, device="cuda"))
    assert cam.prepared == 6 and cam.norm is None
    W = cam.estimate(_dev(frames[5]))
    cc, Ws, its = _stateless(ctx, _dev(frames[5]), _dev(frames[4]))
    assert _bits(cam.cc, W, cam.iterations) == _bits(cc, Ws, its)
    with pytest.raises(ValueError, match="48 x 64"):
        cam.estimate(_dev(frames[0][:, :40]))
    with pytest.raises(ValueError, match="float32"):
        cam.estimate(_dev(frames[0]).double())
    cam.reset()
    assert cam.estimate(_dev(frames[2])) is None and cam.norm is None and cam.cc is None
    W = cam.estimate(_dev(frames[3]))
    assert _bits(cam.cc, W, cam.iterations) == _bits(*_stateless(ctx, _dev(frames[3]), _dev(frames[2])))


@gpu
def test_ghost_motion_compensation(ctx):
    """base_tracker.py:600-633 as one call: the GhostMotion state after it equals compensate(returned warp) applied by hand, and stays untouched when
    the sequence does not move or motion compensation is off; the norm is the float32 norm of the warp's last column."""
    from busca_amd import tracking
    frames = _sequence()
    boxes = np.array([[10.0, 12.0, 30.0, 50.0], [100.5, 40.25, 160.0, 200.0], [3.0, 4.0, 5.0, 6.0]])

    def state():
        st = tracking.GhostMotion(4, 3, ctx=ctx)
        st.add([0, 2, 3], boxes, 1, new=[1, 1, 1])
        st.add([0, 3], boxes[:2] + 1.5, 2)
        return st
    cam, moved, by_hand, still = tracking.GhostCameraMotion(CFG, ctx=ctx), state(), state(), state()
    before = still.hist.cpu().numpy().copy()
    assert tracking.ghost_motion_compensation(cam, moved, _dev(frames[0]), True) is None
    assert np.array_equal(moved.hist.cpu().numpy(), before)                   # first frame: nothing to warp with
    W = tracking.ghost_motion_compensation(cam, moved, _dev(frames[1]), True)
    by_hand.compensate(W)
    assert np.array_equal(moved.hist.cpu().numpy(), by_hand.hist.cpu().numpy()) and not np.array_equal(moved.hist.cpu().numpy(), before)
    assert moved.all_warped and cam.norm.dtype == np.float32 and cam.norm == np.linalg.norm(W[:, -1]) and cam.norm > 0.5
    for kw in (dict(is_moving=False), dict(is_moving=True, enabled=False)):
        W2 = tracking.ghost_motion_compensation(cam, still, _dev(frames[cam.prepared]), **kw)
        assert W2 is not None and cam.norm == np.linalg.norm(W2[:, -1])
        assert np.array_equal(still.hist.cpu().numpy(), before) and not still.all_warped, kw


def _align_abi(ctx, T, I, H, W, motion, iters=5, warp=None):
    warp = np.eye(2, 3, dtype=np.float32) if warp is None else warp
    cc, its = C.c_double(-7.0), C.c_int32(-7)
    rc = ctx.lib.busca_ecc_align_planes(ctx.h, None if T is None else T.data_ptr(), None if I is None else I.data_ptr(), H, W, motion, iters, -1.0,
                                        None if warp is False else warp.ctypes.data, C.byref(cc), C.byref(its), None)
    return rc, cc.value, its.value


@gpu
def test_refusals(ctx):
    """BUSCA_EINVAL, with a message that names the entry point, before any launch: the output plane and the caller's warp are left alone, and the
    context goes on working."""
    import torch
    frame = _dev(_case("32x32")[0])
    ok = dict(t=frame, channels=3, H=32, W=32, strides=frame.stride(), K=15)
    bad = [dict(K=0), dict(K=-3), dict(K=4), dict(K=14), dict(K=33), dict(H=7), dict(W=7), dict(K=31, H=15), dict(K=31, W=15), dict(channels=2), dict(channels=0),
           dict(channels=4), dict(t=None), dict(out=False), dict(strides=(1024, 32, 0)), dict(strides=(1024, -32, 1))]
    for kw in bad:
        out = torch.full((32, 32), 7.0, dtype=torch.float32, device="cuda")
        rc, got = _prepare_abi(ctx, **{**ok, "out": out, **kw})
        assert rc == -1 and (got is None or np.all(got == 7.0)), kw
        assert ctx.lib.busca_last_error(ctx.h).decode().startswith("busca_ecc_prepare"), kw
    assert _prepare_abi(ctx, **dict(ok, K=31, H=16, W=16))[0] == 0               # 31 / 2 + 1 = 16 is taken
    assert ctx.lib.busca_ecc_prepare(None, frame.data_ptr(), 3, 32, 32, 1024, 32, 1, 15, frame.data_ptr(), None) == -1
    T, I = (_dev(p) for p in _planes("32x32"))
    for kw in (dict(T=None), dict(I=None), dict(warp=False), dict(H=7), dict(W=7), dict(motion=3), dict(motion=-1), dict(iters=0)):
        sentinel = np.array([[9, 8, 7], [6, 5, 4]], np.float32)
        rc, cc, its = _align_abi(ctx, **{**dict(T=T, I=I, H=32, W=32, motion=0, warp=sentinel), **kw})
        assert rc == -1 and (cc, its) == (-7.0, -7), kw
        assert ctx.lib.busca_last_error(ctx.h).decode().startswith("busca_ecc_align_planes"), kw
        assert np.array_equal(sentinel, np.array([[9, 8, 7], [6, 5, 4]], np.float32)), kw
    _gpu_steps(ctx, "32x32", "translation", steps=1)


@gpu
def test_estimate_behind_a_busy_stream(ctx, busy):
    """GhostCameraMotion.estimate on a side stream that is still busy (tests/test_streams_gpu.py): the prepare kernels, the gradient pass and every
    iteration are ordered on torch's current stream.  Poison: the two frames swapped, which estimates the opposite motion."""
    from busca_amd import tracking
    cur, prev = (_dev(f) for f in _case("120x160"))
    cfg = {"warp_mode": "Affine", "num_iter_mc": 6, "termination_eps_mc": -1.0}

    def call(x, outs, st):
        cam = tracking.GhostCameraMotion(cfg, ctx=ctx)
        assert cam.estimate(x[0]) is None
        warp = cam.estimate(x[1])
        return [warp, cam.cc, cam.iterations, cam.norm]
    want, _ = behind(busy, "GhostCameraMotion.estimate", call, [prev, cur], [cur, prev], form="current", host=True)
    swapped = call([cur, prev], None, None)
    assert not np.array_equal(want[2], swapped[0])                             # the poison does give another answer
