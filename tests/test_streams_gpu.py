"""Stream order: every entry point behind a busy non-default stream ("Streams").

The rest of the suite runs on the legacy default stream, where work is ordered against everything else whether or not the library orders its own work.
Here each call is made on a side stream `s` that is still busy with a prefix of 4096 x 4096 float32 matmuls.  The library is handed tensors that hold
POISON (valid inputs that give another answer); the true values are copied in on `s`, behind the prefix, and every preallocated output is poisoned.  A
kernel, memset or copy on another stream, a host read behind another stream's synchronisation or a staging upload ordered on the wrong stream then
works on poison (or leaves poison in the output) and the result differs from the idle default-stream run, which it must equal bit for bit.

Every case runs once and is deterministic by construction: the prefix makes the wrong order the one that happens.  Asynchronous calls assert that the
prefix was still running when the call had been enqueued (otherwise the case FAILS as inconclusive); calls that return host values assert that the
prefix, measured with events, was at least 4 x the call's own default-stream wall time.  Two forms: "explicit" = default stream current and `stream=s`
passed (raw C-ABI calls, the handles' `stream` arguments), "current" = `s` is torch's current stream (wrappers without a `stream` argument).

This file: the helper, geometry / crops, Kalman, assignment, appearance, GHOST, ECC.  tests/test_streams_model_gpu.py: Decision Transformer, ReID, the
model level and the stream crossings the library owns."""
import ctypes as C
import math
import os
import time
import types

import numpy as np
import pytest

from busca_amd import synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX_FLOOR = 4          # matmuls: what tests/test_dt_gpu.py::test_host_inputs_are_staged_on_the_stream_given enqueues
PREFIX_FACTOR = 4         # prefix >= 4 x the call's default-stream wall time (absorbs host jitter)
PREFIX_SLACK = 1.25       # the prefix is SIZED for 5 x t_call: behind one another the matmuls run up to 10 % faster than when they were timed
PREFIX_CAP = 2000         # a call that would need more is refused, not run behind a token prefix
CROP = 384 * 128 * 3


# ---- the helper ---------------------------------------------------------------------------------------------------------
class Busy:
    """The busy prefix: `a @ a` of 4096 x 4096 float32 into one buffer, timed once with events."""

    def __init__(self):
        import torch
        self.dev = torch.device("cuda", 0)
        self.a = torch.randn(4096, 4096, device=self.dev)
        self.buf = torch.empty_like(self.a)
        for _ in range(2):
            torch.mm(self.a, self.a, out=self.buf)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            torch.mm(self.a, self.a, out=self.buf)
        e1.record()
        e1.synchronize()
        self.t_mm = e0.elapsed_time(e1) / 4e3          # seconds per matmul
        self.s = torch.cuda.Stream(self.dev)
        self.log = []                                   # (what, t_call s, matmuls, prefix s)

    def enqueue(self, s, t_call):
        """Enqueue the prefix for a call of wall time `t_call` on `s` -> (start event, end event `e_busy`, matmuls)."""
        import torch
        n = max(PREFIX_FLOOR, int(math.ceil(PREFIX_SLACK * PREFIX_FACTOR * t_call / self.t_mm)) + 1)
        assert n <= PREFIX_CAP, "a %.1f ms call would need %d matmuls of prefix" % (1e3 * t_call, n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(n):
                torch.mm(self.a, self.a, out=self.buf)
            e1.record(s)
        return e0, e1, n

    def report(self):
        if not self.log:
            return
        worst = max(self.log, key=lambda r: r[1])
        print("\n[streams] one 4096^3 f32 matmul %.3f ms; %d calls; longest t_call %.3f ms (%s) behind %d matmuls = %.1f ms; prefixes %d .. %d matmuls, "
              "%.1f .. %.1f ms" % (1e3 * self.t_mm, len(self.log), 1e3 * worst[1], worst[0], worst[2], 1e3 * worst[3], min(r[2] for r in self.log),
                                   max(r[2] for r in self.log), 1e3 * min(r[3] for r in self.log), 1e3 * max(r[3] for r in self.log)))


@pytest.fixture(scope="module")
def busy():
    b = Busy()
    yield b
    b.report()


@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _flat(r):
    """Every tensor / array / number of a (nested) result, in order."""
    import torch
    if r is None:
        return []
    if isinstance(r, dict):
        return [x for k in sorted(r) for x in _flat(r[k])]
    if isinstance(r, (list, tuple)):
        return [x for v in r for x in _flat(v)]
    if torch.is_tensor(r):
        return [r]
    return [np.asarray(r)]


def _host(items):
    import torch
    return [x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in items]


def same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind in "fc"), "%s: output %d differs from the default-stream run" % (what, k)


def behind(busy, what, call, true=(), poison=(), outs=None, form="explicit", host=False, prepare=None, stream=None, need_busy=True, x=None):
    """The default-stream result of `call`, then the same call on `s` behind a busy prefix with poisoned inputs and outputs; both must have the same bits.
      call(x, outs, stream)  x: the tensors the library reads (`true` values in the reference run; poison, overwritten on `s` behind the prefix, in the
                             run under test); outs: what `outs()` returned (persistent tensors, poisoned anew by every call of `outs`); stream: the raw
                             stream for the "explicit" form (None = default stream in the reference run), always None in the "current" form, where `s`
                             is torch's current stream instead.  Returns None or (nested) tensors / host values.
      host                   the call returns host values (it synchronises `s` itself): read as returned; the prefix is checked against 4 x t_call
      prepare()              host-side work before the prefix is enqueued (a case's own poisoning of what it cannot reach through `x` / `outs`)
      x                      the tensors handed to the library, where a case needs their addresses beforehand (default: fresh ones like `true`)
      need_busy              False: the call is documented to synchronise the device (workspace growth); the query assertion is dropped
    -> (want, got): lists of host arrays, x first, then outs, then what the call returned."""
    import torch
    s = busy.s if stream is None else stream
    x = [torch.empty_like(t) for t in true] if x is None else x
    mk = outs if outs is not None else (lambda: [])

    def reference():
        for xi, ti in zip(x, true):
            xi.copy_(ti)
        o = mk()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = call(x, o, None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, _host(list(x) + list(o) + _flat(r))
    reference()                                          # warm: weights loaded, workspaces and kernels there
    t_call, want = reference()
    for xi, pi in zip(x, poison):
        xi.copy_(pi)
    o = mk()
    if prepare is not None:
        prepare()
    torch.cuda.synchronize()
    e0, e_busy, n = busy.enqueue(s, t_call)
    with torch.cuda.stream(s):
        for xi, ti in zip(x, true):
            xi.copy_(ti, non_blocking=True)
    if form == "current":
        with torch.cuda.stream(s):
            r = call(x, o, None)
    else:
        assert form == "explicit"
        r = call(x, o, s.cuda_stream)
    still_busy = not e_busy.query()
    r = _flat(r)
    if not host and need_busy:
        assert still_busy, "%s: inconclusive - the %d-matmul prefix had drained before the call was enqueued" % (what, n)
    s.synchronize()                                      # (never the device: a read behind the wrong stream must stay wrong)
    got = _host(list(x) + list(o) + r)
    prefix = e0.elapsed_time(e_busy) / 1e3
    busy.log.append((what, t_call, n, prefix))
    if host:
        assert prefix >= PREFIX_FACTOR * t_call, "%s: inconclusive - prefix %.2f ms < %d x t_call %.2f ms" % (what, 1e3 * prefix, PREFIX_FACTOR, 1e3 * t_call)
    same_bits(got, want, what)
    return want, got


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _nan(t):
    import torch
    return torch.full_like(t, float("nan"))


def _full(shape, value, dtype):
    import torch
    return torch.full(tuple(shape), value, dtype=dtype, device=torch.device("cuda", 0))


def _scrub_pinned(nbytes):
    """Fill the pinned block the caching host allocator will hand to the next table of this size (the reference run's own table, answer included) with
    0xFF: NaN as float64, -1 as int32."""
    import torch
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    t.fill_(255)
    del t


# ---- inputs and their poison (shared with the CPU test below) -------------------------------------------------------------
def _boxes(seed, n):
    cx = synth.uniform(seed, "cx", (n,), 0, 1920).astype(np.float64)
    cy = synth.uniform(seed, "cy", (n,), 0, 1080).astype(np.float64)
    h = synth.uniform(seed, "h", (n,), 10, 400).astype(np.float64)
    w = h * synth.uniform(seed, "ar", (n,), 0.2, 0.6).astype(np.float64)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


PAIR_MODES = ["center", "center_w", "iou", "iou_cost", "fuse"]
TOPK_SHAPES = [(5, 257, 7), (4, 1100, 33)]          # the rank kernel; the round-by-round kernel beyond 1 024 columns
FRAME_HW = (270, 480)
CROP_BOXES = np.array([[100.3, 50.2, 180.9, 200.7],        # interior
                       [-20.5, -30.0, 60.2, 120.0],        # clipped top-left: mean padding
                       [430.0, 200.0, 520.0, 300.0],       # clipped bottom-right
                       [2000.0, 2000.0, 2100.0, 2200.0],   # outside
                       [10.0, -60.0, 138.0, 324.0],        # extent 128 x 384: the copy path (clipped, the frame is 270 rows)
                       [300.0, 100.0, 340.0, 180.0]], dtype=np.float64)
SIZED_BOXES = np.concatenate([CROP_BOXES[:4], [[10.0, 10.0, 74.0, 202.0], [300.0, 100.0, 340.0, 180.0]]])      # (64, 192): its own copy-sized box


def _pair_inputs():
    return _boxes(18, 17), _boxes(67, 65), synth.uniform(9, "scores", (65,), 0.1, 1.0).astype(np.float64)


def _pair_oracle(mode, a, b, sc):
    from oracle import geometry as og
    with np.errstate(all="ignore"):
        if mode == "center":
            return og.center_distance(a, b)
        if mode == "center_w":
            return og.center_distance(a, b, weight_size=True)
        if mode == "iou":
            return og.iou_matrix(a, b)
        return og.fuse_score(og.iou_distance(a, b), sc) if mode == "fuse" else og.iou_distance(a, b)


def _topk_inputs(B, N, P):
    return synth.uniform(B + N + P, "d", (B, N), 0, 500).astype(np.float64)


def _frame():
    return synth.randint_u8(3, "frame", FRAME_HW + (3,))


def _cover_rects():
    H, W = FRAME_HW
    x = np.sort(synth.uniform(5, "x", (40, 2), 0, W - 1).astype(np.int32), 1)
    y = np.sort(synth.uniform(5, "y", (40, 2), 0, H - 1).astype(np.int32), 1)
    return np.ascontiguousarray(np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1))


def _ecc_frames():
    from tests.test_ecc import _pair
    im1, im2, _ = _pair()
    return np.ascontiguousarray(im1), np.ascontiguousarray(im2)


def test_poison_is_distinguishable():
    """Every poison of a case with a CPU oracle is a valid input whose oracle answer differs from the true one (no GPU needed)."""
    from busca_amd.tracking import box_extents
    from oracle import ecc as oecc, geometry as og
    a, b, sc = _pair_inputs()
    nan = lambda v: np.full_like(v, np.nan)
    for mode in PAIR_MODES:
        assert not np.array_equal(_pair_oracle(mode, a, b, sc), _pair_oracle(mode, nan(a), nan(b), nan(sc)), equal_nan=True), mode
    for B, N, P in TOPK_SHAPES:
        d = _topk_inputs(B, N, P)
        assert not np.array_equal(og.topk_rows(d, P), og.topk_rows(d[:, ::-1].copy(), P))
    fr = _frame()
    assert not np.array_equal(fr, 255 - fr)
    rects = box_extents(CROP_BOXES)
    assert len({tuple(r) for r in rects}) == len(rects)                      # rolled rects: another rect in every row
    for boxes, size in ((CROP_BOXES, (128, 384)), (SIZED_BOXES, (64, 192))):
        hit = 0
        for i, bx in enumerate(boxes):
            t, p = og.get_bbox_crop(fr, bx, output_size=size), og.get_bbox_crop(255 - fr, bx, output_size=size)
            r = og.get_bbox_crop(fr, boxes[i - 1], output_size=size)
            hit += int(not np.array_equal(t, p)) + int(not np.array_equal(t, r))
            assert not np.array_equal(t, r), i
        assert hit >= 2 * len(boxes) - 1                                     # (the box outside the frame is all padding for any pixels)
    H, W = FRAME_HW
    tracks = lambda rr: [types.SimpleNamespace(tlbr=np.asarray(r, dtype=np.float64), scale=1.0) for r in rr]
    cov = lambda rr: og.detection_coverage((H, W, 3), [np.array(t.tlbr) * t.scale for t in tracks(rr)])["area_covered"]
    assert cov(_cover_rects()) != cov(np.zeros((40, 4), np.int32))
    im1, im2 = _ecc_frames()
    g1, g2 = oecc.bgr2gray(im1), oecc.bgr2gray(im2)
    fwd = oecc.find_transform_ecc(g1, g2, motion="euclidean", iters=6, eps=-1.0)
    rev = oecc.find_transform_ecc(g2, g1, motion="euclidean", iters=6, eps=-1.0)
    assert not np.array_equal(np.asarray(fwd[1]), np.asarray(rev[1]))       # frames swapped: the inverse motion


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def _pair_mode(mode):
    from busca_amd import _lib
    return {"center": _lib.PAIR_CENTER, "center_w": _lib.PAIR_CENTER_WEIGHTED, "iou": _lib.PAIR_IOU}.get(mode, _lib.PAIR_IOU_COST)


@gpu
@pytest.mark.parametrize("mode", PAIR_MODES)
def test_pairwise_abi(ctx, busy, mode):
    import torch
    a, b, sc = (_dev(v) for v in _pair_inputs())
    out = torch.empty(17, 65, dtype=torch.float64, device=a.device)

    def call(x, o, st):
        ctx.check(ctx.lib.busca_pairwise(ctx.h, x[0].data_ptr(), 17, x[1].data_ptr(), 65, _pair_mode(mode), x[2].data_ptr() if mode == "fuse" else None,
                                         o[0].data_ptr(), st))
    want, _ = behind(busy, "busca_pairwise " + mode, call, [a, b, sc], [_nan(a), _nan(b), _nan(sc)], lambda: [out.fill_(float("nan"))])
    assert np.array_equal(want[3], _pair_oracle(mode, *_pair_inputs()), equal_nan=True)


@gpu
@pytest.mark.parametrize("mode", PAIR_MODES[:4])
def test_pairwise_wrapper(ctx, busy, mode):
    from busca_amd import geometry as G
    a, b, _ = (_dev(v) for v in _pair_inputs())
    behind(busy, "geometry.pairwise " + mode, lambda x, o, st: G.pairwise(ctx, x[0], x[1], _pair_mode(mode)), [a, b], [_nan(a), _nan(b)], form="current")


@gpu
@pytest.mark.parametrize("mode", ["center_w", "fuse"])
def test_pairwise_host(ctx, busy, mode):
    """One launch on the current stream, that stream synchronised, the matrix read from the pinned table."""
    from busca_amd import geometry as G
    a, b, sc = _pair_inputs()
    nbytes = 8 * (4 * (17 + 65) + (65 if mode == "fuse" else 0) + 17 * 65)
    want, _ = behind(busy, "geometry.pairwise_host " + mode, lambda x, o, st: G.pairwise_host(ctx, a, b, _pair_mode(mode), scores_b=sc if mode == "fuse" else None),
                     form="current", host=True, prepare=lambda: _scrub_pinned(nbytes))
    assert np.array_equal(want[0], _pair_oracle(mode, a, b, sc), equal_nan=True)


@gpu
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=["rank", "rounds"])
@pytest.mark.parametrize("form", ["explicit", "current", "host"])
def test_topk_rows(ctx, busy, shape, form):
    import torch
    from busca_amd import geometry as G
    from oracle import geometry as og
    B, N, P = shape
    d = _topk_inputs(B, N, P)
    if form == "host":
        want, _ = behind(busy, "geometry.topk_rows_host", lambda x, o, st: G.topk_rows_host(ctx, d, P), form="current", host=True,
                         prepare=lambda: _scrub_pinned(8 * (B * N + (B * P + 1) // 2)))
        assert np.array_equal(want[0], og.topk_rows(d, P))
        return
    dd = _dev(d)
    if form == "current":
        want, _ = behind(busy, "geometry.topk_rows", lambda x, o, st: G.topk_rows(ctx, x[0], P), [dd], [dd.flip(1).contiguous()], form="current")
    else:
        idx = _full((B, P), -7, torch.int32)
        want, _ = behind(busy, "busca_topk_rows", lambda x, o, st: ctx.check(ctx.lib.busca_topk_rows(ctx.h, x[0].data_ptr(), B, N, P, o[0].data_ptr(), st)),
                         [dd], [dd.flip(1).contiguous()], lambda: [idx.fill_(-7)])
    assert np.array_equal(want[1], og.topk_rows(d, P))


@gpu
def test_coverage(ctx, busy):
    import torch
    H, W = FRAME_HW
    r = _dev(_cover_rects())
    cnt = torch.empty(1, dtype=torch.int64, device=r.device)
    want, _ = behind(busy, "busca_coverage", lambda x, o, st: ctx.check(ctx.lib.busca_coverage(ctx.h, x[0].data_ptr(), 40, H, W, o[0].data_ptr(), st)),
                     [r], [torch.zeros_like(r)], lambda: [cnt.fill_(-7)])
    canvas = np.zeros((H, W), bool)
    for x1, y1, x2, y2 in _cover_rects():
        canvas[y1:y2 + 1, x1:x2 + 1] = True
    assert int(want[1][0]) == int(canvas.sum())


@gpu
def test_duplicate_masks(ctx, busy):
    import torch
    nA, nB = 23, 40
    cost = synth.uniform(4, "dup", (nA, nB), 0.2, 1.0).astype(np.float64)
    pairs = ((0, 3), (5, 5), (22, 39), (7, 0), (11, 20))
    for i, j in pairs:
        cost[i, j] = 0.05 + 0.004 * i
    age_a = np.arange(nA, dtype=np.int32) * 3 % 17
    age_b = np.arange(nB, dtype=np.int32) * 5 % 13
    c, aa, ab = _dev(cost), _dev(age_a), _dev(age_b)
    ka, kb = torch.empty(nA, dtype=torch.uint8, device=c.device), torch.empty(nB, dtype=torch.uint8, device=c.device)

    def call(x, o, st):
        ctx.check(ctx.lib.busca_duplicate_masks(ctx.h, x[0].data_ptr(), nA, nB, x[1].data_ptr(), x[2].data_ptr(), 0.15, o[0].data_ptr(), o[1].data_ptr(), st))
    want, _ = behind(busy, "busca_duplicate_masks", call, [c, aa, ab], [_nan(c), torch.zeros_like(aa), torch.zeros_like(ab)], lambda: [ka.fill_(0xA5), kb.fill_(0xA5)])
    keep_a, keep_b = np.ones(nA, np.uint8), np.ones(nB, np.uint8)
    for i, j in pairs:                                   # the younger track goes, ties drop the A track
        if age_a[i] > age_b[j]:
            keep_b[j] = 0
        else:
            keep_a[i] = 0
    assert np.array_equal(want[3], keep_a) and np.array_equal(want[4], keep_b) and keep_a.sum() + keep_b.sum() == nA + nB - 5


def _crop_oracle(boxes, size=(128, 384)):
    from oracle import geometry as og
    fr = _frame()
    return np.stack([og.get_bbox_crop(fr, bx, output_size=size) for bx in boxes])


@gpu
@pytest.mark.parametrize("band", [1, 0], ids=["band", "pixel"])
@pytest.mark.parametrize("target", ["dst_u8", "out_u8", "out_f16"])
@pytest.mark.parametrize("tables", ["device", "pinned"])
def test_crop_gather_ex(ctx, busy, tables, target, band):
    """Frame pixels (and, in device memory, the extents and the destination table) arrive on `s` behind the prefix; with pinned tables the kernel reads
    them from host memory that is final before the call."""
    import torch
    from busca_amd.tracking import box_extents
    from oracle import geometry as og
    H, W = FRAME_HW
    n = len(CROP_BOXES)
    dev = torch.device("cuda", 0)
    fr = _dev(_frame())
    rects = box_extents(CROP_BOXES)
    slots = torch.empty(n + 1, 384, 128, 3, dtype=torch.uint8, device=dev)              # slot n: the spare one poisoned destinations point at
    ptrs = slots.data_ptr() + CROP * np.arange(n, dtype=np.int64)[::-1].copy()           # crop i -> slot n - 1 - i
    u8 = torch.empty(n, 384, 128, 3, dtype=torch.uint8, device=dev)
    f16 = torch.empty(n, 384, 128, 4, dtype=torch.float16, device=dev)
    table = torch.empty(3 * n, dtype=torch.int64, pin_memory=True)
    table.numpy()[:2 * n] = rects.reshape(-1).view(np.int64)
    table.numpy()[2 * n:] = ptrs
    true, poison = [fr], [255 - fr]
    if tables == "device":
        r, p = _dev(rects), _dev(ptrs)
        true += [r, p]
        poison += [r.roll(1, 0).contiguous(), torch.full_like(p, slots.data_ptr() + CROP * n)]

    def call(x, o, st):
        rp, dp = (x[1].data_ptr(), x[2].data_ptr()) if tables == "device" else (table.data_ptr(), table.data_ptr() + 16 * n)
        ctx.check(ctx.lib.busca_crop_gather_ex(ctx.h, x[0].data_ptr(), H, W, x[0].stride(0), rp, n, dp if target == "dst_u8" else None,
                                               u8.data_ptr() if target == "out_u8" else None, f16.data_ptr() if target == "out_f16" else None, st))
    ctx.set_option("crop_band", band)
    try:
        want, _ = behind(busy, "busca_crop_gather_ex %s %s band %d" % (tables, target, band), call, true, poison,
                         lambda: [slots.fill_(0xA5), u8.fill_(0xA5), f16.fill_(float("nan"))])
    finally:
        ctx.set_option("crop_band", 1)
    ws, wu, wf = want[-3:]
    ref = _crop_oracle(CROP_BOXES)
    if target == "dst_u8":
        assert np.array_equal(ws[:n][::-1], ref) and (ws[n] == 0xA5).all() and (wu == 0xA5).all()
    elif target == "out_u8":
        assert np.array_equal(wu, ref) and (ws == 0xA5).all()
    else:
        assert np.array_equal(wf[..., :3], og.normalize_bgr(ref)[..., ::-1].astype(np.float16)) and (wf[..., 3] == 0).all() and (wu == 0xA5).all()


@gpu
def test_crop_gather_float_boxes(ctx, busy):
    """busca_crop_gather: float32 boxes in device memory, rounded to extents on the device."""
    import torch
    H, W = FRAME_HW
    n = len(CROP_BOXES)
    fr, bx = _dev(_frame()), _dev(CROP_BOXES.astype(np.float32))
    u8 = torch.empty(n, 384, 128, 3, dtype=torch.uint8, device=fr.device)
    want, _ = behind(busy, "busca_crop_gather", lambda x, o, st: ctx.check(ctx.lib.busca_crop_gather(
        ctx.h, x[0].data_ptr(), H, W, x[0].stride(0), x[1].data_ptr(), n, o[0].data_ptr(), None, st)), [fr, bx], [255 - fr, bx.roll(1, 0).contiguous()],
        lambda: [u8.fill_(0xA5)])
    assert not (want[2] == 0xA5).all(axis=(1, 2, 3)).any()


@gpu
def test_crop_gather_sized(ctx, busy):
    import torch
    from busca_amd.tracking import box_extents
    H, W = FRAME_HW
    n = len(SIZED_BOXES)
    fr, r = _dev(_frame()), _dev(box_extents(SIZED_BOXES))
    out = torch.empty(n, 192, 64, 3, dtype=torch.uint8, device=fr.device)
    want, _ = behind(busy, "busca_crop_gather_sized", lambda x, o, st: ctx.check(ctx.lib.busca_crop_gather_sized(
        ctx.h, x[0].data_ptr(), H, W, x[0].stride(0), x[1].data_ptr(), n, 192, 64, o[0].data_ptr(), st)), [fr, r], [255 - fr, r.roll(1, 0).contiguous()],
        lambda: [out.fill_(0xA5)])
    assert np.array_equal(want[2], _crop_oracle(SIZED_BOXES, (64, 192)))


@gpu
def test_gather_crops(ctx, busy):
    """Five sources, one of them 0 (an all-zero crop); the poisoned table is all 0."""
    import torch
    pool = _dev(synth.randint_u8(8, "pool", (4, 384, 128, 3)))
    x_pool = torch.empty_like(pool)                                                      # the tensor the addresses point into
    src = _dev(np.array([x_pool.data_ptr() + CROP * k if k >= 0 else 0 for k in (2, 0, -1, 3, 1)], dtype=np.int64))
    out = torch.empty(5, 384, 128, 3, dtype=torch.uint8, device=src.device)
    want, _ = behind(busy, "busca_gather_crops", lambda x, o, st: ctx.check(ctx.lib.busca_gather_crops(ctx.h, x[1].data_ptr(), 5, o[0].data_ptr(), st)),
                     [pool, src], [255 - pool, torch.zeros_like(src)], lambda: [out.fill_(0xA5)], x=[x_pool, torch.empty_like(src)])
    p = want[0]
    assert np.array_equal(want[2], np.stack([p[2], p[0], np.zeros_like(p[0]), p[3], p[1]]))


@gpu
def test_crop_gather_from_a_host_frame(ctx, busy):
    """geometry.crop_gather on a host frame outside a frame scope: the sub-frame and the extents go through pinned memory, asynchronously, on the current stream."""
    import torch
    from busca_amd import geometry as G
    from busca_amd.tracking import box_extents
    fr = _frame()
    boxes = np.array([[300.0, 100.0, 340.0, 180.0], [310.5, 120.2, 380.7, 200.9]])
    sub, _ = G._frame_for_rects(ctx, fr, box_extents(boxes), torch.device("cuda", ctx.device))
    assert tuple(sub.shape) == (101, 81, 3)                                   # the union of the two boxes, not the frame

    def warm():                                          # pinned blocks of both sizes in the host allocator's cache: no hipHostMalloc inside the call
        keep = [torch.empty(n, dtype=torch.uint8, pin_memory=True) for n in (101 * 81 * 3, 8 * 3 * len(boxes)) for _ in range(4)]
        del keep
    want, _ = behind(busy, "geometry.crop_gather(host frame)", lambda x, o, st: G.crop_gather(ctx, fr, boxes, want_u8=True)[0], form="current", prepare=warm)
    assert np.array_equal(want[0], _crop_oracle(boxes))


# ---- Kalman filter and association rounds (n = 23 tracks, m = 40 detections) ---------------------------------------------------
N_TRK, N_DET = 23, 40


def _kalman():
    with np.load(os.path.join(ROOT, "tests", "golden", "kalman.npz")) as f:
        return {k: f[k] for k in ("mean", "cov", "meas", "gate_meas", "init_meas")}


def _states(lo):
    g = _kalman()
    return _dev(g["mean"][lo:lo + N_TRK]), _dev(g["cov"][lo:lo + N_TRK]), _dev(g["meas"][lo:lo + N_TRK])


@gpu
def test_kalman_multi_predict(ctx, busy):
    import torch
    mean, cov, _ = _states(0)
    pm, pc, _ = _states(N_TRK)
    nt = _dev((np.arange(N_TRK) % 3 == 0).astype(np.uint8))
    behind(busy, "busca_kalman_multi_predict", lambda x, o, st: ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), N_TRK, st)),
           [mean, cov, nt], [pm, pc, 1 - nt])


@gpu
def test_kalman_update(ctx, busy):
    import torch
    true, poison = _states(0), _states(N_TRK)
    status = torch.empty(N_TRK, dtype=torch.int32, device=true[0].device)
    want, _ = behind(busy, "busca_kalman_update", lambda x, o, st: ctx.check(ctx.lib.busca_kalman_update(ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), N_TRK, o[0].data_ptr(), st)),
                     list(true), list(poison), lambda: [status.fill_(-7)])
    assert (want[3] == 0).all()


@gpu
def test_kalman_initiate_and_boxes(ctx, busy):
    import torch
    g = _kalman()
    z, pz = _dev(g["init_meas"][:N_TRK]), _dev(g["init_meas"][N_TRK:2 * N_TRK])
    mean = torch.empty(N_TRK, 8, dtype=torch.float64, device=z.device)
    cov = torch.empty(N_TRK, 8, 8, dtype=torch.float64, device=z.device)
    behind(busy, "busca_kalman_initiate", lambda x, o, st: ctx.check(ctx.lib.busca_kalman_initiate(ctx.h, x[0].data_ptr(), N_TRK, o[0].data_ptr(), o[1].data_ptr(), st)),
           [z], [pz], lambda: [mean.fill_(float("nan")), cov.fill_(float("nan"))])
    m, pm = _states(0)[0], _states(N_TRK)[0]
    box = torch.empty(N_TRK, 4, dtype=torch.float64, device=z.device)
    for tlbr in (0, 1):
        behind(busy, "busca_kalman_boxes tlbr %d" % tlbr, lambda x, o, st: ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, x[0].data_ptr(), N_TRK, tlbr, o[0].data_ptr(), st)),
               [m], [pm], lambda: [box.fill_(float("nan"))])


@gpu
@pytest.mark.parametrize("only_position", [0, 1])
@pytest.mark.parametrize("metric", [0, 1], ids=["maha", "gaussian"])
def test_kalman_gating(ctx, busy, metric, only_position):
    import torch
    g = _kalman()
    mean, cov, _ = _states(0)
    pm, pc, _ = _states(N_TRK)
    z = _dev(g["gate_meas"][:N_DET])
    out = torch.empty(N_TRK, N_DET, dtype=torch.float64, device=z.device)
    status = torch.empty(N_TRK, dtype=torch.int32, device=z.device)
    want, _ = behind(busy, "busca_kalman_gating metric %d only_position %d" % (metric, only_position), lambda x, o, st: ctx.check(ctx.lib.busca_kalman_gating(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), N_TRK, x[2].data_ptr(), N_DET, only_position, metric, o[0].data_ptr(), o[1].data_ptr(), st)),
        [mean, cov, z], [pm, pc, z.flip(0).contiguous()], lambda: [out.fill_(float("nan")), status.fill_(-7)])
    assert (want[4] == 0).all() and np.isfinite(want[3]).all()


def _tracks_and_detections():
    g = _kalman()
    tracks = [types.SimpleNamespace(mean=g["mean"][i].copy(), covariance=g["cov"][i].copy(), state=1 if i % 3 else 2) for i in range(N_TRK)]
    dets = []
    for z in g["gate_meas"][:N_DET]:
        w = z[2] * z[3]
        tlwh = np.array([z[0] - w / 2, z[1] - z[3] / 2, w, z[3]])
        dets.append(types.SimpleNamespace(tlwh=tlwh, tlbr=np.array([tlwh[0], tlwh[1], tlwh[0] + tlwh[2], tlwh[1] + tlwh[3]])))
    return tracks, dets, synth.uniform(2, "det", (N_DET,), 0.3, 1.0).astype(np.float64)


@gpu
@pytest.mark.parametrize("which", ["predicted_cost", "associate_round"])
def test_association_round_wrappers(ctx, busy, which):
    """Host tracks in, host values out, under `s`: uploads, the chain of launches and the one copy back are all on the current stream."""
    from busca_amd import tracking

    def call(x, o, st):
        tracks, dets, scores = _tracks_and_detections()
        if which == "predicted_cost":
            r = tracking.predicted_cost(tracks, dets, det_scores=scores, fuse_motion=True, ctx=ctx)
        else:
            r = tracking.associate_round(tracks, dets, 0.9, det_scores=scores, fuse_motion=True, ctx=ctx)
        return [r, [t.mean for t in tracks], [t.covariance for t in tracks]]
    behind(busy, "tracking." + which, call, form="current", host=True)


@gpu
@pytest.mark.parametrize("path", ["lds", "global"])
def test_linear_assignment(ctx, busy, path):
    """A batch of three problems inside 23 x 40 slabs with `dims`; one 141 x 141 problem, which does not fit the LDS beside the solver's state."""
    import torch
    b, n, m = (3, N_TRK, N_DET) if path == "lds" else (1, 141, 141)
    cost = _dev(synth.uniform_costs(31, b * n, m).reshape(b, n, m))
    dims = _dev(np.array([[23, 40], [20, 33], [7, 40]], dtype=np.int32)) if path == "lds" else None
    dev, i32, f64 = cost.device, torch.int32, torch.float64
    o = [torch.empty(b, n, dtype=i32, device=dev), torch.empty(b, m, dtype=i32, device=dev), torch.empty(b, n + m, dtype=f64, device=dev),
         torch.empty(b, dtype=f64, device=dev), torch.empty(b, dtype=i32, device=dev)]

    def call(x, o, st):
        ctx.check(ctx.lib.busca_linear_assignment(ctx.h, x[0].data_ptr(), b, n, m, x[1].data_ptr() if dims is not None else None, 0.8,
                                                  o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), st))
    true = [cost] + ([dims] if dims is not None else [])
    poison = [cost.flip(2).contiguous()] + ([torch.zeros_like(dims)] if dims is not None else [])
    want, _ = behind(busy, "busca_linear_assignment " + path, call, true, poison,
                     lambda: [o[0].fill_(-7), o[1].fill_(-7), o[2].fill_(-7.0), o[3].fill_(-7.0), o[4].fill_(-7)])
    assert ctx.get_option("last_assign_staged") == (1 if path == "lds" else 0)
    assert (want[-1] == 0).all() and (want[len(true)] >= 0).sum() >= 7


# ---- appearance and GHOST (n = 17 tracks, budget 3, m = 20 detections) ----------------------------------------------------------
A_N, A_BUDGET, A_M = 17, 3, 20
A_SLOT = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, -1, 9, 3, 10, 7], dtype=np.int32)
A_COUNT = np.array([3, 2, 1, 0, 3, 3, 2, 1, 3, 3, 2, 3, 1, 2, 3, 3, 1], dtype=np.int32)
A_NEWEST = np.array([2, 1, 0, 0, 0, 1, 1, 0, 2, 0, 1, 1, 0, 1, 2, 0, 0], dtype=np.int32)


def _appearance(E):
    """(true, poison) of gallery, slot, count, dets: NaN features, another in-range slot in every row, counts of 0."""
    import torch
    trk, det = synth.appearance_features(50 + E, A_N, A_M, E, A_BUDGET, twins=True)
    g, s, c, d = _dev(trk), _dev(A_SLOT), _dev(A_COUNT), _dev(det)
    return [g, s, c, d], [_nan(g), s.flip(0).contiguous(), torch.zeros_like(c), _nan(d)]


@gpu
@pytest.mark.parametrize("E", [16, 512])
@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("reduce", [0, 1], ids=["min", "mean"])
def test_appearance_cost(ctx, busy, reduce, clamp, E):
    import torch
    true, poison = _appearance(E)
    out = torch.empty(A_N, A_M, dtype=torch.float64, device=true[0].device)
    want, _ = behind(busy, "busca_appearance_cost", lambda x, o, st: ctx.check(ctx.lib.busca_appearance_cost(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), A_N, A_BUDGET, x[3].data_ptr(), A_M, E, reduce, clamp, o[0].data_ptr(), st)),
        true, poison, lambda: [out.fill_(float("nan"))])
    w = want[4]
    assert np.isinf(w[[3, 12, 14]]).all() and np.isfinite(np.delete(w, [3, 12, 14], 0)).all()        # slot 3 is empty, row 12 has no slot


@gpu
@pytest.mark.parametrize("E", [16, 512])
@pytest.mark.parametrize("reduce", range(5), ids=["min", "mean", "max", "midrange", "median"])
def test_ghost_distance(ctx, busy, reduce, E):
    import torch
    true, poison = _appearance(E)
    out = torch.empty(A_N, A_M, dtype=torch.float64, device=true[0].device)
    want, _ = behind(busy, "busca_ghost_distance", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_distance(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), A_N, A_BUDGET, x[3].data_ptr(), A_M, E, reduce, o[0].data_ptr(), st)),
        true, poison, lambda: [out.fill_(float("nan"))])
    assert np.isfinite(np.delete(want[4], [3, 12, 14], 0)).all()


@gpu
@pytest.mark.parametrize("E", [16, 512])
@pytest.mark.parametrize("mode", range(5), ids=["last", "first", "mean", "meannorm", "median"])
def test_ghost_proxies(ctx, busy, mode, E):
    import torch
    true, poison = _appearance(E)
    nw = _dev(A_NEWEST)
    true, poison = true[:3] + [nw], poison[:3] + [torch.zeros_like(nw)]
    out = torch.empty(A_N, E, dtype=torch.float32, device=nw.device)
    want, _ = behind(busy, "busca_ghost_proxies", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_proxies(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr(), A_N, A_BUDGET, E, mode, 2, o[0].data_ptr(), st)),
        true, poison, lambda: [out.fill_(-7.0)])
    assert np.isfinite(np.delete(want[4], [3, 12, 14], 0)).all()


@gpu
def test_ghost_thresholds_and_combine(ctx, busy):
    import torch
    n, m, na = A_N, A_M, 9
    app = _dev(synth.uniform_costs(6, n, m, 0.0, 2.0))
    motion = _dev(synth.uniform_costs(7, n, m))
    thr = torch.empty(2, dtype=torch.float64, device=app.device)
    want, _ = behind(busy, "busca_ghost_thresholds", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_thresholds(ctx.h, x[0].data_ptr(), n, m, na, 0.5, 1.0, o[0].data_ptr(), st)),
                     [app], [_nan(app)], lambda: [thr.fill_(-7.0)])
    assert np.isfinite(want[1]).all()
    tl, dl = _dev((np.arange(n) % 3).astype(np.int32)), _dev((np.arange(m) % 3).astype(np.int32))
    t = _dev(np.array([1.1, 0.9]))
    out = torch.empty(n, m, dtype=torch.float64, device=app.device)
    want, _ = behind(busy, "busca_ghost_combine", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_combine(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), n, m, 0.4, x[2].data_ptr(), x[3].data_ptr(), na, x[4].data_ptr(), o[0].data_ptr(), st)),
        [app, motion, tl, dl, t], [_nan(app), _nan(motion), torch.zeros_like(tl), torch.ones_like(dl), _nan(t)], lambda: [out.fill_(-7.0)])
    assert 0 < np.isfinite(want[5]).sum() < n * m


@gpu
def test_ghost_round(ctx, busy):
    """tracking.ghost_round on device-resident features (round 0 of the fixture of tests/test_ghost_round.py): the matches are host values."""
    import torch
    from busca_amd import tracking
    from tests.test_ghost_round import ROUND_CFG, gold, round_state
    state, det, labels, seed, n, m, na = round_state(0)
    cfg = dict(ROUND_CFG[0], nan_first=True, distance="cosine", use_bism=False)
    gal, d, mo = _dev(state.gallery), _dev(det), _dev(synth.tracker_costs(seed, n, m))
    cnt = np.asarray(state.count)
    valid = _dev(np.arange(gal.shape[1])[None, :, None] < cnt[:, None, None]).expand_as(gal)
    pg = torch.where(valid, -gal, gal)                                   # (rows beyond a track's count stay NaN and are never read)

    def call(x, o, st):
        st8 = types.SimpleNamespace(gallery=x[0], count=state.count, newest=state.newest, slot=None, num_active=na)
        dist, row, col = tracking.ghost_round(st8, x[1], labels, x[2], cfg, ctx=ctx)
        return [dist, row, col]
    want, _ = behind(busy, "tracking.ghost_round", call, [gal, d, mo], [pg, d.flip(0).contiguous(), mo.flip(1).contiguous()], form="current", host=True)
    assert np.array_equal(want[4], gold()["rd_row_0_0"]) and np.array_equal(want[5], gold()["rd_col_0_0"])


# ---- ECC ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("motion", [0, 1], ids=["euclidean", "affine"])
@pytest.mark.parametrize("form", ["explicit", "current"])
def test_ecc_align(ctx, busy, motion, form):
    """busca_ecc_align synchronises `stream` once per iteration and solves on the host: warp, cc and iters are host values.  Poison: the two frames swapped
    (the inverse motion)."""
    from busca_amd import tracking
    im1, im2 = (_dev(a) for a in _ecc_frames())
    H, W = im1.shape[:2]

    def call(x, o, st):
        if form == "current":
            cc, warp = tracking.find_transform_ecc(x[0], x[1], motion=("MOTION_EUCLIDEAN", "MOTION_AFFINE")[motion], number_of_iterations=6, termination_eps=-1.0, ctx=ctx)
            return [cc, warp, tracking.find_transform_ecc.last_iterations]
        warp, cc, its = np.eye(2, 3, dtype=np.float32), C.c_double(-7.0), C.c_int32(-7)
        ctx.check(ctx.lib.busca_ecc_align(ctx.h, x[0].data_ptr(), x[1].data_ptr(), H, W, 3 * W, 3 * W, motion, 6, -1.0, warp.ctypes.data, C.byref(cc), C.byref(its), st))
        return [cc.value, warp, its.value]
    want, _ = behind(busy, "busca_ecc_align motion %d %s" % (motion, form), call, [im1, im2], [im2, im1], form=form, host=True)
    assert want[2] > 0.9 and int(want[4]) == 6
