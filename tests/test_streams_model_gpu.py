"""Stream order, second part (helper and contract: tests/test_streams_gpu.py): the Decision Transformer, the ReID extractor and its per-stream
workspace pool, the model level with its side stream, and the stream crossings the library owns."""
import gc
import time
import types

import numpy as np
import pytest

from busca_amd import synth
from tests.test_streams_gpu import Busy, _dev, behind, same_bits

gpu = pytest.mark.gpu
PRECS = ["f32", "x3", "f16"]
FORMS = ["explicit", "current"]


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


# ---- Decision Transformer (device inputs) ----------------------------------------------------------------------------------------
_DT = {}


def _dt_model(ctx, prec, d, seed=11, sd=None):
    from busca_amd.dt import DecisionTransformerHIP
    key = (id(ctx), prec, d, seed, sd is not None)
    if key not in _DT:
        _DT[key] = DecisionTransformerHIP(ctx, sd if sd is not None else synth.dt_state_dict(seed, d=d, ff=2 * d), activation="relu", fake_bbox_f64=True, precision=prec)
    return _DT[key]


def _dt_inputs(B, L, P, seed=11, sentinel_every=4):
    """(true, poison) device tensors.  Poison stays finite and in range (a NaN box has no bucket, a NaN feature trips the x3 range report): the
    features negated and moved to the next track, the boxes moved to the next track."""
    inp = synth.dt_inputs(seed, B, L, P, sentinel_every=sentinel_every)
    true = [_dev(inp[k]) for k in ("mem_feat", "can_feat", "mem_boxes", "can_boxes")]
    poison = [(-t if k < 2 else t).roll(1, 0).contiguous() for k, t in enumerate(true)]
    return true, poison


def test_poison_is_distinguishable_dt_and_kalman():
    """The oracle's answers for the poisoned Decision-Transformer and Kalman inputs differ from the true ones, and the poison is finite (no GPU needed)."""
    import os
    from oracle import bytetrack as obt, dt as odt
    from tests.test_streams_gpu import N_TRK, _kalman
    inp = synth.dt_inputs(11, 5, 11, 5, sentinel_every=4)
    names = ("mem_feat", "can_feat", "mem_boxes", "can_boxes")
    bad = {k: np.roll(-inp[k] if k.endswith("feat") else inp[k], 1, 0) for k in names}
    assert all(np.isfinite(v).all() for v in bad.values())
    sd = synth.dt_state_dict(11, d=256, ff=512)
    cfg = odt.DTConfig(d=256, ff=512)
    a, b = odt.dt_forward(sd, cfg, **inp).numpy(), odt.dt_forward(sd, cfg, **bad).numpy()
    assert np.isfinite(b).all() and (np.abs(a - b).max(1) > 1e-3).all()             # every track's logits move
    g = _kalman()
    t = obt.kalman_multi_predict(g["mean"][:N_TRK], g["cov"][:N_TRK])
    p = obt.kalman_multi_predict(g["mean"][N_TRK:2 * N_TRK], g["cov"][N_TRK:2 * N_TRK])
    assert (np.abs(t[0] - p[0]).max(1) > 0).all() and (np.abs(t[1] - p[1]).max((1, 2)) > 0).all()
    assert not np.array_equal(g["meas"][:N_TRK], g["meas"][N_TRK:2 * N_TRK]) and not np.array_equal(g["init_meas"][:N_TRK], g["init_meas"][N_TRK:2 * N_TRK])


def _dt_call(m, form, **kw):
    def call(x, o, st):
        return dict(m.forward(*x, stream=st, **kw)) if form == "explicit" else dict(m.forward(*x, **kw))
    return call


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("full", [False, True], ids=["logits", "hidden+att"])
@pytest.mark.parametrize("prec", PRECS)
def test_dt_one_kernel(ctx, busy, prec, full, form):
    """(5, 11, 5, 256): without hidden states / attention maps the f32 and x3 launches take the pruned, unique-row kernel, with them the plain one.
    The outputs are allocated under the current stream and written on `stream`."""
    m = _dt_model(ctx, prec, 256)
    true, poison = _dt_inputs(5, 11, 5)
    behind(busy, "dt.forward %s %s %s" % (prec, "full" if full else "lean", form), _dt_call(m, form, want_hidden=full, want_att=full), true, poison, form=form)
    assert ctx.get_option("dt_status") == 0


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_dt_token_split_tail(ctx, busy, prec):
    m = _dt_model(ctx, prec, 256)
    true, poison = _dt_inputs(5, 11, 5)
    ctx.set_option("dt_ntrk", 1)
    ctx.set_option("dt_split", 1)
    try:
        behind(busy, "dt.forward split " + prec, _dt_call(m, "explicit", want_hidden=True, want_att=True), true, poison)
        assert ctx.get_option("last_dt_split") == 5 and ctx.get_option("dt_status") == 0
    finally:
        ctx.set_option("dt_ntrk", 0)
        ctx.set_option("dt_split", -1)


@gpu
@pytest.mark.parametrize("grow", [False, True], ids=["reserved", "grows-on-s"])
@pytest.mark.parametrize("prec", PRECS)
def test_dt_layerwise(busy, prec, grow):
    """(4, 11, 40, 64): 95 tokens, the layer-wise path.  The reference runs on one context; the run under test is the FIRST forward of a second context
    (same weights), with the workspace reserved on `s` beforehand or growing inside the forward on `s` (one stream synchronisation + hipMalloc, so the
    prefix has drained when the call returns: no query assertion there)."""
    import torch
    from busca_amd import _lib
    B, L, P = 4, 11, 40
    ca, cb = _lib.Context(0), _lib.Context(0)
    try:
        sd = synth.dt_state_dict(13, d=64, ff=128)
        ma, mb = _dt_model(ca, prec, 64, sd=sd), _dt_model(cb, prec, 64, sd=sd)
        if not grow:
            with torch.cuda.stream(busy.s):
                mb.reserve(B, L, P)
        true, poison = _dt_inputs(B, L, P, seed=13)
        behind(busy, "dt.forward layer-wise %s %s" % (prec, "grow" if grow else "reserved"),
               lambda x, o, st: dict((ma if st is None else mb).forward(*x, want_hidden=True, stream=st)), true, poison, need_busy=not grow)
        assert ca.get_option("dt_status") == 0 and cb.get_option("dt_status") == 0
    finally:
        _DT.clear()
        ca.close()
        cb.close()


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_dt_bucket_ids(ctx, busy, form):
    import torch
    m = _dt_model(ctx, "f32", 256)
    B, L, P = 5, 11, 5
    true, poison = _dt_inputs(B, L, P)
    if form == "current":
        behind(busy, "dt.bucket_ids", lambda x, o, st: m.bucket_ids(x[0], x[1]), true[2:], poison[2:], form="current")
        return
    ids = torch.empty(B, L + 2 * (P + 2), 3, dtype=torch.int32, device=true[0].device)
    m._ensure_loaded()
    behind(busy, "busca_dt_bucket_ids", lambda x, o, st: ctx.check(ctx.lib.busca_dt_bucket_ids(ctx.h, x[0].data_ptr(), x[1].data_ptr(), B, L, P, o[0].data_ptr(), st)),
           true[2:], poison[2:], lambda: [ids.fill_(-7)])


@gpu
def test_dt_x3_fallback_settles_on_the_stream(ctx, busy):
    """An x3 forward on `s` that leaves the split-fp16 range (weights of test_x3_reports_operands_beyond_its_range): once `s` is synchronised
    `settle` runs the step again in exact float32 on `s` and synchronises - the f32 flavour's bits, `dt_status` 0 afterwards."""
    import torch
    from busca_amd.dt import DecisionTransformerHIP
    sd = synth.dt_state_dict(11, d=256, ff=512)
    hot = dict(sd)
    hot["transformer_encoder.layers.1.norm1.weight"] = sd["transformer_encoder.layers.1.norm1.weight"] * 3000.0
    true, poison = _dt_inputs(8, 11, 16, sentinel_every=16)                 # the inputs of that test
    keys = ("logits", "probs", "argmax", "hidden")
    m32 = DecisionTransformerHIP(ctx, hot, activation="relu", fake_bbox_f64=True, precision="f32")
    w = m32.forward(*true, want_hidden=True)
    torch.cuda.synchronize()
    want = [w[k].cpu().numpy() for k in keys]
    assert ctx.get_option("dt_status") == 0
    mh = DecisionTransformerHIP(ctx, hot, activation="relu", fake_bbox_f64=True, precision="x3")
    t0 = time.perf_counter()
    o = mh.forward(*true, want_hidden=True)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    assert ctx.get_option("dt_status") == 2
    fixed = mh.settle(o)
    same_bits([fixed[k].cpu().numpy() for k in keys], want, "settle on the default stream")
    x = [p.clone() for p in poison]
    torch.cuda.synchronize()
    s = busy.s
    e0, e_busy, n = busy.enqueue(s, t_call)
    with torch.cuda.stream(s):
        for xi, ti in zip(x, true):
            xi.copy_(ti, non_blocking=True)
    o = mh.forward(*x, want_hidden=True, stream=s.cuda_stream)
    assert not e_busy.query(), "inconclusive - the %d-matmul prefix had drained before the forward was enqueued" % n
    s.synchronize()
    assert ctx.get_option("dt_status") == 2
    fixed = mh.settle(o)
    assert fixed is not o and ctx.get_option("dt_status") == 0 and ctx.get_option("dt_exact_f32") == 0
    same_bits([fixed[k].cpu().numpy() for k in keys], want, "settle after a forward on s")
    busy.log.append(("dt x3 fallback", t_call, n, e0.elapsed_time(e_busy) / 1e3))


# ---- ReID ----------------------------------------------------------------------------------------------------------------------------
def _crops(seed, n):
    base = synth.randint_u8(seed, "crops", (n, 24, 8, 3)).astype(np.float32)
    up = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    noise = synth.randint_u8(seed, "noise", (n, 384, 128, 3)).astype(np.float32) - 128
    return np.clip(up + 0.25 * noise, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def reid(busy):
    """One context and extractor per flavour (a context holds ONE ReID weight set), weights synth.reid_state_dict(3), running statistics of the fixture;
    workspaces for 5 crops reserved on the default stream and on `s` (a workspace that grows inside a forward synchronises the device:
    test_reid_workspace_pool has those cases)."""
    import os
    from busca_amd import _lib
    from busca_amd.reid import ReIDEncoderHIP
    from tests.test_streams_gpu import ROOT
    sd = synth.reid_state_dict(3)
    with np.load(os.path.join(ROOT, "tests", "golden", "reid_bn.npz")) as f:
        stats = np.array(f["r1_stats"])
    ctxs = {p: _lib.Context(0) for p in PRECS}
    ms = {p: ReIDEncoderHIP(ctxs[p], sd, precision=p) for p in PRECS}
    for m in ms.values():
        m.stats0 = stats
        m.reserve(5)
        m.reserve(5, stream=busy.s.cuda_stream)
    yield ms
    for c in ctxs.values():
        c.close()


def _u8(n):
    c = _dev(_crops(40 + n, n))
    return c, 255 - c


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("prec", PRECS)
def test_reid_forward(reid, busy, prec, n, form):
    """The batch-statistics forward: plain, and with multiplicities and a zero-normalised crop (the weights are staged through pinned memory on the stream
    of the pass).  `feats` is allocated under the current stream and written on `stream`."""
    m = reid[prec]
    c, p = _u8(n)
    zn = _dev((np.arange(n) == 1).astype(np.uint8))
    w = np.array([1, 3, 2, 1, 2][:n], np.float32)
    kw = lambda st: dict(stream=st) if form == "explicit" else {}
    behind(busy, "reid.forward %s n=%d %s" % (prec, n, form), lambda x, o, st: m.forward(x[0], **kw(st)), [c], [p], form=form)
    behind(busy, "reid.forward(weights, zero_norm) %s n=%d %s" % (prec, n, form), lambda x, o, st: m.forward(x[0], zero_norm=x[1], weights=w, **kw(st)),
           [c, zn], [p, 1 - zn], form=form)
    assert m.take_status() is False


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("prec", PRECS)
def test_reid_running_statistics(reid, busy, prec, n, form):
    """forward_running; adapt followed by a read of the running statistics on the same stream (host values: the read synchronises that stream)."""
    m = reid[prec]
    c, p = _u8(n)
    kw = lambda st: dict(stream=st) if form == "explicit" else {}
    m.load_running_stats(m.stats0)
    behind(busy, "reid.forward_running %s n=%d %s" % (prec, n, form), lambda x, o, st: m.forward_running(x[0], output="norm", **kw(st)), [c], [p], form=form)

    def reload():                                        # (synchronous, like a weight load: before the prefix)
        m.load_running_stats(m.stats0)
        return []

    def call(x, o, st):
        feats = m.adapt(x[0], 0.1, **kw(st))
        if form == "current":                            # the handle's own read, on torch's current stream
            return [feats, m.running_stats()]
        stats = np.empty(m.ctx.lib.busca_reid_running_floats(), np.float32)
        m.ctx.check(m.ctx.lib.busca_reid_get_running_stats(m.ctx.h, stats.ctypes.data, stats.size, st))
        return [feats, stats]
    want, _ = behind(busy, "reid.adapt + running stats %s n=%d %s" % (prec, n, form), call, [c], [p], reload, form=form, host=True)
    assert not np.array_equal(want[2], m.stats0)
    m.load_running_stats(m.stats0)
    assert m.take_status() is False


@gpu
def test_bn_stats_1x1(busy):
    """busca_bn_stats_1x1 at (5, 8, 6, 128 -> 512, transform) of tests/test_bn_stats_gpu.py: it synchronises `stream` and frees its scratch inside the call."""
    import torch
    from busca_amd import _lib
    ctx = _lib.Context(0)
    n, H, W, Cin, Cout, stride = 5, 8, 6, 128, 512, 1
    seed = 1000 + Cin + Cout + n
    x16 = _dev((synth.normal(seed, "x", (n, H, W, Cin)) * 1.5).astype(np.float16))
    w16 = _dev((synth.normal(seed, "w", (Cout, Cin)) * (1.0 / np.sqrt(Cin))).astype(np.float16))
    gamma = _dev((1.0 + 0.1 * synth.normal(seed, "g", (Cout,))).astype(np.float32))
    beta = _dev((0.1 * synth.normal(seed, "b", (Cout,))).astype(np.float32))
    ss = _dev(np.stack([1.0 + 0.2 * synth.normal(seed, "s", (Cin,)), 0.3 * synth.normal(seed, "t", (Cin,))], 1).astype(np.float32))
    out = torch.empty(Cout, 2, device=x16.device)
    true = [x16, ss, w16, gamma, beta]
    try:
        behind(busy, "busca_bn_stats_1x1", lambda x, o, st: ctx.check(ctx.lib.busca_bn_stats_1x1(
            ctx.h, x[0].data_ptr(), x[1].data_ptr(), n, H, W, Cin, stride, x[2].data_ptr(), Cout, x[3].data_ptr(), x[4].data_ptr(), o[0].data_ptr(), st)),
            true, [-t.roll(1, 0).contiguous() for t in true], lambda: [out.fill_(float("nan"))], host=True)
    finally:
        ctx.close()


@gpu
def test_reid_x3_status_after_a_forward_on_s(busy):
    """take_status once `s` is synchronised, after an x3 pass on `s` whose activations leave the split-fp16 range (weights of
    test_x3_reid_reports_operands_beyond_its_range, n = 6).  With these weights every batch overflows, the poisoned one too: the status word shows that
    the report of a pass on `s` is there once `s` is synchronised, the features (bit for bit, non-finite ones included) show the order."""
    import torch
    from busca_amd import _lib
    from busca_amd.reid import ReIDEncoderHIP
    ctx = _lib.Context(0)
    try:
        sd = synth.reid_state_dict(3)
        hot = dict(sd)
        hot["layer1.0.bn1.weight"] = sd["layer1.0.bn1.weight"] * 4000.0
        hot["layer1.0.bn1.bias"] = sd["layer1.0.bn1.bias"] * 4000.0
        m = ReIDEncoderHIP(ctx, hot, precision="x3")
        c = _dev(_crops(906, 6))
        seen = []

        def call(x, o, st):
            if st is None:                               # the reference runs: synchronised and read here
                f = m.forward(x[0])
                torch.cuda.synchronize()
                seen.append(m.take_status())
                return f
            return m.forward(x[0], stream=st)
        behind(busy, "reid.forward x3 overflow", call, [c], [255 - c])
        assert seen == [True, True]
        assert ctx.get_option("reid_status") == 2 and m.take_status() is True and m.take_status() is False
    finally:
        ctx.close()


@gpu
def test_reid_workspace_pool(busy):
    """reid_ws_acquire: a pool of 4 workspaces keyed by stream.  On a fresh context: the first-ever forward on a fresh stream (allocation and the ticket
    zero-fill inside the call), two forwards back to back on two streams with nothing between them, then forwards on five distinct streams in turn
    and again on the first (the fifth recycles slot 0 behind a device synchronisation).  Every result is the default-stream forward's bits of a second
    context with the same weights."""
    import torch
    from busca_amd import _lib
    from busca_amd.reid import ReIDEncoderHIP
    ca, cb = _lib.Context(0), _lib.Context(0)
    try:
        sd = synth.reid_state_dict(3)
        ma, mb = ReIDEncoderHIP(ca, sd, precision="f16"), ReIDEncoderHIP(cb, sd, precision="f16")
        crops = {n: _u8(n) for n in (3, 5)}
        want, t_call = {}, {}
        for n, (c, _) in crops.items():
            ma.forward(c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = ma.forward(c)
            torch.cuda.synchronize()
            t_call[n] = time.perf_counter() - t0
            want[n] = f.cpu().numpy()
        streams = [torch.cuda.Stream(busy.dev) for _ in range(5)]
        assert len({s.cuda_stream for s in streams}) == 5

        def start(s, n):
            """Poisoned crops, a prefix on `s`, the true crops behind it, the forward on `s` -> (features, e_busy, the input kept alive)."""
            c, p = crops[n]
            x = p.clone()
            torch.cuda.synchronize()
            e0, e_busy, k = busy.enqueue(s, t_call[n])
            with torch.cuda.stream(s):
                x.copy_(c, non_blocking=True)
            f = mb.forward(x, stream=s.cuda_stream)
            busy.log.append(("reid pool n=%d" % n, t_call[n], k, k * busy.t_mm))
            return f, e_busy, x

        # the first-ever forward of the context, on a fresh stream: hipMalloc + the ticket hipMemset inside the call
        f, e, x = start(streams[0], 3)
        streams[0].synchronize()
        same_bits([f.cpu().numpy()], [want[3]], "first forward on a fresh stream")
        # two streams, two batch sizes, back to back (the second takes the pool's second workspace inside the call)
        mb.reserve(5, stream=streams[1].cuda_stream)
        c3, p3 = crops[3]
        c5, p5 = crops[5]
        x3, x5 = p3.clone(), p5.clone()
        torch.cuda.synchronize()
        e0a, ea, _ = busy.enqueue(streams[0], t_call[3])
        e0b, eb, _ = busy.enqueue(streams[1], t_call[5])
        with torch.cuda.stream(streams[0]):
            x3.copy_(c3, non_blocking=True)
        with torch.cuda.stream(streams[1]):
            x5.copy_(c5, non_blocking=True)
        f3 = mb.forward(x3, stream=streams[0].cuda_stream)
        f5 = mb.forward(x5, stream=streams[1].cuda_stream)
        assert not ea.query() and not eb.query(), "inconclusive - a prefix had drained before both forwards were enqueued"
        streams[0].synchronize()
        streams[1].synchronize()
        same_bits([f3.cpu().numpy(), f5.cpu().numpy()], [want[3], want[5]], "two forwards on two streams")
        # five streams in turn, then the first again: streams 2, 3 claim the last two workspaces, stream 4 and then stream 0 recycle slot 0
        for k in (0, 1, 2, 3, 4, 0):
            f, e, x = start(streams[k], 3)
            streams[k].synchronize()
            same_bits([f.cpu().numpy()], [want[3]], "forward on stream %d of five" % k)
    finally:
        ca.close()
        cb.close()


# ---- stream crossings the library owns -----------------------------------------------------------------------------------------------
@gpu
def test_frame_scope_opened_on_one_stream_and_used_on_another(ctx, busy):
    """geometry.begin_frame on s1 behind a prefix (the frame arrives there), crops cut on s2: `_frame_on_device` makes s2 wait for the upload."""
    import torch
    from busca_amd import geometry as G
    from tests.test_streams_gpu import CROP_BOXES, _crop_oracle, _frame
    s1, s2 = busy.s, torch.cuda.Stream(busy.dev)
    fr = _dev(_frame())
    x = 255 - fr
    torch.cuda.synchronize()
    e0, e_busy, n = busy.enqueue(s1, 0.0)
    with torch.cuda.stream(s1):
        x.copy_(fr, non_blocking=True)
        G.begin_frame(ctx, x)
    try:
        with torch.cuda.stream(s2):
            u8, _ = G.crop_gather(ctx, x, CROP_BOXES, want_u8=True)
        assert not e_busy.query(), "inconclusive - the prefix had drained before the crops were enqueued"
        s2.synchronize()
        got = u8.cpu().numpy()
    finally:
        G.end_frame(ctx)
    assert np.array_equal(got, _crop_oracle(CROP_BOXES))


@gpu
def test_lazy_host_copy_read_from_another_stream(ctx, busy):
    """get_image_crops(host_copy="lazy") on `s` behind a prefix, the first host read of a crop from the default stream: FrameHostCopy.rows waits for the
    event recorded behind the crop kernel."""
    import torch
    from busca_amd import tracking
    from tests.test_streams_gpu import CROP_BOXES, _crop_oracle, _frame
    s = busy.s
    fr = _dev(_frame())
    x = 255 - fr
    torch.cuda.synchronize()
    e0, e_busy, n = busy.enqueue(s, 0.0)
    with torch.cuda.stream(s):
        x.copy_(fr, non_blocking=True)
        crops = tracking.get_image_crops(x, CROP_BOXES, normalize=False, ctx=ctx, host_copy="lazy")
    assert not e_busy.query(), "inconclusive - the prefix had drained before the crops were enqueued"
    got = np.asarray(crops[2])                           # default stream current: gather + copy there, behind the event
    assert np.array_equal(got, _crop_oracle(CROP_BOXES)[2])
    assert np.array_equal(np.stack([np.asarray(c) for c in crops]), _crop_oracle(CROP_BOXES))


# ---- model level (shipped-shape random model of tests/test_associate_gpu.py; 3 lost tracks, 5 candidates) -------------------------
def _args(precision="f32"):
    import torch
    return types.SimpleNamespace(num_layer=4, nhead=4, dim_embedding=512, trans_dim=64, ff_size=128, activation="gelu", dropout_p=0.1,
                                 input_flavour="MEM-SEP-CAN-BAD", output_flavour="CAN", encode_separator_as_reference=True, encode_special_tokens=False,
                                 reid_weights_file="no", device=torch.device("cuda:0"), precision=precision, pinned_numpy_semantics=True)


@pytest.fixture(scope="module")
def model():
    import torch
    from busca_amd.network import BUSCA
    m = BUSCA(_args()).to(torch.device("cuda:0")).eval()
    sd = dict(synth.dt_state_dict(17, d=64, ff=128))
    sd.update({"reid_encoder.model." + k: v for k, v in synth.reid_state_dict(17).items()})
    m.load_state_dict(sd)
    m.store_logits = True
    return m


def _reserve_on(model, s):
    """The step's workspaces for `s` as the current stream (and the side stream) now: one that is allocated inside a step synchronises the device."""
    import torch
    with torch.cuda.stream(s):
        model.reserve(3, 11, 5)
    torch.cuda.synchronize()


@gpu
def test_busca_forward_on_s(model, busy):
    """BUSCA.forward under `with torch.cuda.stream(s)`: device crops and boxes arrive on `s`; the candidate batch runs on the side stream, which must have
    waited for `s`, and `s` for it.  Logits and the published per-track state equal the default-stream run."""
    B, L, P = 3, 11, 5
    mem = _dev(_crops(5, B * L).reshape(B, L, 384, 128, 3))
    can = _dev(_crops(6, B * P).reshape(B, P, 384, 128, 3))
    inp = synth.dt_inputs(5, B, L, P, sentinel_every=0)
    mb, cb = _dev(inp["mem_boxes"]), _dev(inp["can_boxes"])
    _reserve_on(model, busy.s)
    waited = []

    def call(x, o, st):
        logits = model.forward(x[0], x[1], x[2], x[3])
        waited.append(not model._side_stream.query())
        return [logits]
    poison = [255 - mem, 255 - can, mb.roll(1, 0).contiguous(), cb.roll(1, 0).contiguous()]
    behind(busy, "BUSCA.forward", call, [mem, can, mb, cb], poison, form="current")
    assert waited[-1], "the side stream did not wait for s: its ReID batch was complete while the prefix on s was still running"

    def call_published(x, o, st):                        # return_logits: publishing the per-track state gathers rows by a host index list, a
        logits = model.forward(x[0], x[1], x[2], x[3], return_logits=True)      # synchronous upload on `s` - the host waits for the prefix there
        return [logits, model.logits, model.mem_logits]
    behind(busy, "BUSCA.forward(return_logits)", call_published, [mem, can, mb, cb], poison, form="current", need_busy=False)


def _scene(model, frame):
    """3 lost tracks with 12-crop memories, 5 detections, Kalman candidates; every crop device-resident (slots of the model's crop pool)."""
    boxes = np.array([[20 + 9 * i, 10 + 3 * i, 70 + 9 * i, 150 + 3 * i] for i in range(44)], np.float64)
    crops = model.get_image_crops(frame, boxes, normalize=False)
    trk = lambda tlwh, ims: types.SimpleNamespace(tlwh_mem=[np.asarray(b, np.float64) for b in tlwh], images_mem=list(ims), scale=1.0, tlwh=np.asarray(tlwh[-1], np.float64))
    hist = [trk([[50 + 100 * t, 40, 60, 220]] * 12, [crops[12 * t + i] for i in range(12)]) for t in range(3)]
    dets = [trk([[55 + 60 * j, 45, 60, 220]], [crops[36 + j]]) for j in range(5)]
    kal = [trk([[52 + 100 * t, 42, 60, 220]], [crops[41 + t]]) for t in range(3)]
    dists = np.array([[abs((50 + 100 * t) - (55 + 60 * j)) + 0.5 * j for j in range(5)] for t in range(3)], np.float64)
    return hist, dets, kal, dists


@gpu
@pytest.mark.parametrize("which", ["associate_embeddings", "batcher"])
def test_association_step_on_s(model, busy, which):
    """The crops are cut from a device frame that arrives on `s` behind the prefix and stay in pool slots; the step (index gathers, the memory batch on
    the side stream, the candidate batch and the Decision Transformer on `s`, the copy back) returns host values."""
    from busca_amd.batcher import StepBatcher
    from tests.test_streams_gpu import _frame
    fr = _dev(_frame())
    _reserve_on(model, busy.s)
    waited = []

    def call(x, o, st):
        hist, dets, kal, dists = _scene(model, x[0])
        if which == "batcher":
            b = StepBatcher(model)
            t1 = b.submit(hist, dets, dists, 11, 5, True, False, extra_kalman_candidates=kal, normalize_ims=True)
            t2 = b.submit(hist[:2], dets[:4], dists[:2, :4], 11, 5, True, True, extra_kalman_candidates=kal[:2], normalize_ims=True)
            waited.append(not model._side_stream.query())
            b.flush()
            r = [t1.result(), t2.result()]
        else:
            r = list(model.associate_embeddings(hist, dets, dists, 11, 5, True, False, extra_kalman_candidates=kal, normalize_ims=True))
            assert model.last_gather[1] == 0 and model.last_gather[0] > 0           # everything came from the device pool
        return r + [model.logits, model.mem_logits]

    def poison_slots():                                  # the slots the run under test will get hold the crops of the inverted frame
        _scene(model, 255 - fr)
        gc.collect()
    want, _ = behind(busy, "BUSCA " + which, call, [fr], [255 - fr], form="current", host=True, prepare=poison_slots)
    assert np.asarray(want[1]).max() > 0
    if which == "batcher":
        assert waited[-1], "the side stream did not wait for s: its memory batch was complete while the prefix on s was still running"
