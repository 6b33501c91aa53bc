"""Running-statistics BatchNorm of the ReID extractor (include/busca_reid_bn.h): busca_reid_load_running_stats / _reset / _get / _forward_running / _adapt,
their mirrors on ReIDEncoderHIP and the standalone busca_amd.network.ReID_Encoder.

The reference is tests/golden/reid_bn.npz, recorded by tests/golden/make_golden_reid_bn.py from the reference's own ReID_Encoder on the CPU (weights
synth.reid_state_dict(3), crops rebuilt here from the seeds).

Bars, none of them taken from a kernel's output:
  * features, `plain`: the bars of tests/test_reid_gpu.py - 5e-5 for the float32-class flavours (f32, x3), FEAT_ATOL = 1e-2 for f16.  `norm` (fc7 before
    F.normalize): the same bar times the 2-norm of the reference row, since plain = norm / |norm|.
  * batch independence (eval mode): a crop alone against the same crop in a batch - both within one bar of the reference, so within two of each other.
  * running statistics, as |d mean| / sqrt(var + eps) and |d (var + eps)| / (var + eps):
      f32, x3: twice the same distance between the fixture's float32 and float64 statistics (what float32 arithmetic alone moves them by), floor 1e-5.
      f16: its activations are fp16.  The project's bar for what that does to a feature vector is cosine >= COS_MIN = 0.9990 (tests/test_reid_gpu.py),
           a relative deviation of sqrt(2 (1 - COS_MIN)) = 4.5e-2.  A batch mean can move by at most the relative deviation of its elements (no
           averaging assumed), a variance by twice that: 4.5e-2 of sigma for the mean, 8.9e-2 for var + eps.
    Each test prints the measured gap (pytest -s)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from busca_amd import synth, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reid_bn.npz")
FLAVOURS = ("f32", "x3", "f16")
FEAT_BAR = {"f32": 5e-5, "x3": 5e-5, "f16": 1e-2}       # tests/test_reid_gpu.py: 5e-5 (exact flavours), FEAT_ATOL
COS_MIN = 0.9990                                        # tests/test_reid_gpu.py
R1_CASE, R2_CASE, EVAL_CASES, R2_EVAL_CASE, R2_MOMENTUM = (6, 61), (4, 62), ((1, 71), (3, 73), (5, 75)), (3, 73), 0.1     # make_golden_reid_bn.py
EINVAL, ENOWEIGHTS = -1, -2
EPS = 1e-5

_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            g = {k: f[k] for k in f.files}
        for v in g.values():
            v.setflags(write=False)
        _CACHE["g"] = g
    return _CACHE["g"]


def crops(seed, n):
    """make_golden.smooth_crops"""
    key = ("c", seed, n)
    if key not in _CACHE:
        base = synth.randint_u8(seed, "crops", (n, 24, 8, 3)).astype(np.float32)
        up = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
        noise = synth.randint_u8(seed, "noise", (n, 384, 128, 3)).astype(np.float32) - 128
        c = np.clip(up + 0.25 * noise, 0, 255).astype(np.uint8)
        c.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key].copy()              # (computed once; a writable copy per use: torch.from_numpy wants one)


def split(stats):
    """blob -> (mean [26560], var [26560]) in channel order"""
    mean, var, off = [], [], 0
    for spec in synth.reid_conv_specs():
        C = spec[1]
        mean.append(stats[off:off + C])
        var.append(stats[off + C:off + 2 * C])
        off += 2 * C
    assert off == stats.size
    return np.concatenate(mean).astype(np.float64), np.concatenate(var).astype(np.float64)


def stat_gap(got, ref):
    """(max |d mean| / sqrt(var + eps), max |d (var + eps)| / (var + eps)), the scale taken from `ref`"""
    gm, gv = split(got)
    rm, rv = split(ref)
    return float((np.abs(gm - rm) / np.sqrt(rv + EPS)).max()), float((np.abs(gv - rv) / (rv + EPS)).max())


def stat_bars(prec, which):
    g = gold()
    if prec == "f16":
        rel = float(np.sqrt(2.0 * (1.0 - COS_MIN)))
        return rel, 2.0 * rel
    f32 = g[which + "_stats"]
    f64 = f32.astype(np.float64) + g[which + "_stats_f64_minus_f32"].astype(np.float64)
    dm, dv = stat_gap(f32.astype(np.float64), f64)
    return max(2.0 * dm, 1e-5), max(2.0 * dv, 1e-5)


def shrink_var(stats, conv):
    """`stats` with the running variance of conv `conv` (forward order) brought down to var + eps = 1e-9: its BatchNorm then scales by gamma x 31 623"""
    out, off = np.array(stats, dtype=np.float32), 0
    for i, spec in enumerate(synth.reid_conv_specs()):
        if i == conv:
            out[off + spec[1]:off + 2 * spec[1]] = np.float32(1e-9) - np.float32(EPS)
        off += 2 * spec[1]
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_reid_bn.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    assert names == set(_lib.REID_BN_SIGNATURES) and len(names) == 6
    for header, table in _lib.HEADERS.items():
        assert header == "busca_reid_bn.h" or not names & set(table)
    lib = _lib.load()
    for name in names:
        assert len(getattr(lib, name).argtypes) == len(_lib.REID_BN_SIGNATURES[name][1])
    assert lib.busca_version() >= 2004 and lib.busca_version() // 1000 == 2
    assert lib.busca_reid_running_floats() == 2 * 26560
    for name, val in (("BUSCA_REID_OUT_PLAIN", _lib.REID_OUT_PLAIN), ("BUSCA_REID_OUT_NORM", _lib.REID_OUT_NORM)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name


def test_running_blob_layout_and_errors():
    sd, k = {}, 0
    for (_name, cout, _cin, _k, _s, _p, bn) in synth.reid_conv_specs():
        sd["m." + bn + ".running_mean"] = np.full(cout, 2.0 * k, np.float32)
        sd["m." + bn + ".running_var"] = np.full(cout, 2.0 * k + 1.0, np.float32)
        sd["m." + bn + ".num_batches_tracked"] = np.array(7)
        k += 1
    blob = weights.reid_running_blob(sd, "m.")
    assert blob.dtype == np.float32 and blob.shape == (2 * 26560,)
    mean, var = split(blob)
    counts = [s[1] for s in synth.reid_conv_specs()]
    assert np.array_equal(mean, np.repeat(2.0 * np.arange(53), counts)) and np.array_equal(var, mean + 1.0)
    assert blob[:128].tolist() == [0.0] * 64 + [1.0] * 64 and blob[128] == 2.0          # conv 0: mean[64], var[64]; then conv 1
    assert np.array_equal(weights.reid_running_blob({k_: torch.from_numpy(v) for k_, v in sd.items()}, "m."), blob)
    reset = weights.reid_running_reset()
    assert np.array_equal(split(reset)[0], np.zeros(26560)) and np.array_equal(split(reset)[1], np.ones(26560)) and reset.dtype == np.float32
    for lost in ("m.layer3.2.bn2.running_var", "m.bn1.running_mean", "m.layer4.0.downsample.1.running_mean"):
        with pytest.raises(KeyError, match=re.escape(lost)):
            weights.reid_running_blob({k_: v for k_, v in sd.items() if k_ != lost}, "m.")
    with pytest.raises(KeyError, match="bn1.running_mean"):
        weights.reid_running_blob(sd)                                                    # wrong prefix


def test_encoder_takes_the_reference_signature():
    from busca_amd.network import BUSCA, ReID_Encoder
    enc = ReID_Encoder(299, torch.device("cuda"), "no", False, "plain", False, False)
    assert ReID_Encoder.PRETRAINED_SIZE == (384, 128) and enc.PRETRAINED_SIZE == (384, 128) and enc.embedding_size == 512
    assert (enc.num_classes, enc.pretrained_path, enc.use_domain_adaptation, enc.output_option, enc.trainable, enc.use_checkpointing) == (299, "no", False, "plain", False, False)
    assert enc.training is False and enc.momentum == 0.1 and enc.exact_reruns == 0
    assert enc.train() is enc and enc.training is True and enc.eval() is enc and enc.training is False
    dflt = ReID_Encoder(num_classes=10, device="cuda:0")
    assert dflt.use_domain_adaptation is True and dflt.output_option == "plain" and dflt.pretrained_path is None
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.network as bn
    finally:
        sys.path.pop(0)
    assert bn.ReID_Encoder is ReID_Encoder and bn.BUSCA is BUSCA


def test_encoder_refuses_training_and_unknown_outputs():
    from busca_amd.network import ReID_Encoder
    with pytest.raises(NotImplementedError):
        ReID_Encoder(299, "cuda", "no", True, "plain", True)
    with pytest.raises(ValueError):
        ReID_Encoder(299, "cuda", "no", True, "fc")


def test_encoder_reads_a_checkpoint_as_load_net_does(tmp_path):
    from busca_amd.network import ReID_Encoder
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.reid_state_dict(5, with_fc=True).items()}
    want = np.arange(2 * 26560, dtype=np.float32) / 26560.0 + 0.5
    off = 0
    for (_name, cout, _cin, _k, _s, _p, bn) in synth.reid_conv_specs():
        sd[bn + ".running_mean"] = torch.from_numpy(want[off:off + cout].copy())
        sd[bn + ".running_var"] = torch.from_numpy(want[off + cout:off + 2 * cout].copy())
        sd[bn + ".num_batches_tracked"] = torch.tensor(3)
        off += 2 * cout
    path = str(tmp_path / "reid.pth")
    torch.save({"model_state_dict": sd, "optimizer_state_dict": None}, path)
    enc = ReID_Encoder(299, "cuda", path, False)
    assert np.array_equal(enc._running0, want)
    assert np.array_equal(enc._sd["layer2.0.conv1.weight"], synth.reid_state_dict(5)["layer2.0.conv1.weight"]) and "fc.weight" not in enc._sd
    bad = dict(sd)
    bad["module.extra.weight"] = torch.zeros(3)
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="module.extra.weight"):
        ReID_Encoder(299, "cuda", path, False)
    del sd["layer1.0.bn2.running_var"]
    torch.save(sd, path)
    with pytest.raises(KeyError, match="layer1.0.bn2.running_var"):
        ReID_Encoder(299, "cuda", path, False)


def test_fixture_contents():
    g = gold()
    assert os.path.getsize(GOLD) < (1 << 20)
    for r in ("r1", "r2"):
        assert g[r + "_stats"].shape == (2 * 26560,) and g[r + "_stats"].dtype == np.float32 and g[r + "_stats_f64_minus_f32"].shape == (2 * 26560,)
        assert (split(g[r + "_stats"])[1] > 0).all()
        dm, dv = stat_bars("f32", r)
        assert 1e-5 <= dm < 1e-3 and 1e-5 <= dv < 1e-3, (dm, dv)                  # float32 noise, no more
    for n, _seed in EVAL_CASES:
        plain, norm = g["r1_eval_plain_n%d" % n], g["r1_eval_norm_n%d" % n]
        assert plain.shape == norm.shape == (n, 512)
        assert np.abs(norm / np.linalg.norm(norm, axis=1, keepdims=True) - plain).max() < 1e-6
    assert g["r1_feats"].shape == (6, 512) and g["r2_feats"].shape == (4, 512) and g["r2_eval_plain_n3"].shape == (3, 512)
    assert np.abs(g["r2_eval_plain_n3"] - g["r1_eval_plain_n3"]).max() > 1e-4       # R2 is not R1: the eval features moved


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encs():
    """One context and extractor per flavour (a context holds ONE weight set), weights synth.reid_state_dict(3)"""
    from busca_amd import _lib
    from busca_amd.reid import ReIDEncoderHIP
    sd = synth.reid_state_dict(3)
    ctxs = {p: _lib.Context(0) for p in FLAVOURS}
    yield {p: ReIDEncoderHIP(ctxs[p], sd, precision=p) for p in FLAVOURS}
    for c in ctxs.values():
        c.close()


def feat_check(got, ref, bar, what, norm=False):
    scale = np.linalg.norm(ref.astype(np.float64), axis=1, keepdims=True) if norm else 1.0
    err = float((np.abs(got.astype(np.float64) - ref) / scale).max())
    print("%s: max |d feature|%s = %.3g (bar %.1g)" % (what, " / |fc7|" if norm else "", err, bar))
    assert got.shape == ref.shape and np.isfinite(got).all() and err <= bar, (what, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_eval_features_under_r1(encs, prec):
    g, m = gold(), encs[prec]
    m.load_running_stats(g["r1_stats"])
    assert np.array_equal(m.running_stats(), g["r1_stats"])                       # get after load: bit for bit
    for n, seed in EVAL_CASES:
        for option in ("plain", "norm"):
            got = m.forward_running(crops(seed, n), output=option).cpu().numpy()
            feat_check(got, g["r1_eval_%s_n%d" % (option, n)], FEAT_BAR[prec], "%s eval %s n=%d" % (prec, option, n), norm=option == "norm")
    assert np.array_equal(m.forward_running(crops(73, 3), output="neck").cpu().numpy(), m.forward_running(crops(73, 3), output="norm").cpu().numpy())
    assert m.take_status() is False


@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_eval_features_do_not_depend_on_the_batch(encs, prec):
    m = encs[prec]
    m.load_running_stats(gold()["r1_stats"])
    batch = m.forward_running(crops(75, 5)).cpu().numpy()
    for i in range(5):
        alone = m.forward_running(crops(75, 5)[i:i + 1]).cpu().numpy()
        gap = float(np.abs(alone[0] - batch[i]).max())
        print("%s crop %d alone vs in the batch: %.3g (bar %.1g)" % (prec, i, gap, 2 * FEAT_BAR[prec]))
        assert gap <= 2 * FEAT_BAR[prec], (prec, i, gap)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_adapt_reproduces_the_reference_statistics(encs, prec):
    g, m = gold(), encs[prec]
    m.reset_running_stats()
    assert np.array_equal(m.running_stats(), weights.reid_running_reset())
    f1 = m.adapt(crops(R1_CASE[1], R1_CASE[0]), 1.0).cpu().numpy()
    r1 = m.running_stats()
    bm, bv = stat_bars(prec, "r1")
    dm, dv = stat_gap(r1, g["r1_stats"])
    print("%s R1: |d mean| / sigma = %.3g (bar %.3g), |d var| / var = %.3g (bar %.3g)" % (prec, dm, bm, dv, bv))
    feat_check(f1, g["r1_feats"], FEAT_BAR[prec], "%s R1 pass" % prec)
    assert dm <= bm and dv <= bv, (prec, dm, bm, dv, bv)
    # R2 from the FIXTURE's R1 (so that the bar measures one update), momentum 0.1
    m.load_running_stats(g["r1_stats"])
    f2 = m.adapt(crops(R2_CASE[1], R2_CASE[0]), R2_MOMENTUM).cpu().numpy()
    r2 = m.running_stats()
    bm, bv = stat_bars(prec, "r2")
    dm, dv = stat_gap(r2, g["r2_stats"])
    print("%s R2: |d mean| / sigma = %.3g (bar %.3g), |d var| / var = %.3g (bar %.3g)" % (prec, dm, bm, dv, bv))
    feat_check(f2, g["r2_feats"], FEAT_BAR[prec], "%s R2 pass" % prec)
    assert dm <= bm and dv <= bv, (prec, dm, bm, dv, bv)
    # eval under the device's own R2 (the table adapt rebuilt on the stream)
    got = m.forward_running(crops(R2_EVAL_CASE[1], R2_EVAL_CASE[0])).cpu().numpy()
    feat_check(got, g["r2_eval_plain_n3"], FEAT_BAR[prec], "%s eval under its own R2" % prec)
    assert m.take_status() is False


@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_adapt_with_momentum_zero_is_the_plain_forward(encs, prec):
    g, m = gold(), encs[prec]
    m.load_running_stats(g["r2_stats"])
    c = crops(R1_CASE[1], R1_CASE[0])
    want = m.forward(c).cpu().numpy()
    got = m.adapt(c, 0.0).cpu().numpy()
    raw = m.adapt(c, 0.0, output="norm").cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(m.running_stats(), g["r2_stats"])
    feat_check(raw / np.linalg.norm(raw, axis=1, keepdims=True), want, 1e-6, "%s norm output, normalised on the host" % prec)
    assert np.array_equal(m.forward(c).cpu().numpy(), want)


@pytest.mark.gpu
def test_return_codes():
    from busca_amd import _lib
    ctx = _lib.Context(0)
    lib, h = ctx.lib, ctx.h
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(np.array(crops(73, 3))).to(dev)
    out = torch.zeros(3, 512, device=dev)
    host = np.zeros(2 * 26560, np.float32)
    s = torch.cuda.current_stream(dev).cuda_stream
    good = np.array(gold()["r1_stats"])
    try:
        assert lib.busca_reid_load_running_stats(h, good.ctypes.data, good.size) == ENOWEIGHTS
        assert lib.busca_reid_reset_running_stats(h) == ENOWEIGHTS
        assert lib.busca_reid_get_running_stats(h, host.ctypes.data, host.size, s) == ENOWEIGHTS
        assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 0, out.data_ptr(), s) == ENOWEIGHTS
        assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, 0.0, 0, out.data_ptr(), s) == ENOWEIGHTS
        blob = weights.reid_blob(synth.reid_state_dict(3))
        for prec in (0, 2):
            ctx.check(lib.busca_reid_load_weights_ex(h, blob.ctypes.data, blob.size, prec))
            # weights without statistics
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_get_running_stats(h, host.ctypes.data, host.size, s) == EINVAL
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, 0.5, 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, 0.0, 1, out.data_ptr(), s) == 0
            # bad statistics leave none loaded
            assert lib.busca_reid_load_running_stats(h, good.ctypes.data, good.size - 1) == EINVAL
            assert lib.busca_reid_load_running_stats(h, None, good.size) == EINVAL
            for pos, val in ((5, np.nan), (26559 * 2, np.inf), (64 + 3, -1e-5), (64 + 3, -1.0)):        # (64 + 3: a variance of the stem)
                bad = good.copy()
                bad[pos] = val
                assert lib.busca_reid_load_running_stats(h, bad.ctypes.data, bad.size) == EINVAL, (pos, val)
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 0, out.data_ptr(), s) == EINVAL
            ctx.check(lib.busca_reid_load_running_stats(h, good.ctypes.data, good.size))
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 0, out.data_ptr(), s) == 0
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 2, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_forward_running(h, c.data_ptr(), -1, None, 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 0, None, 0, out.data_ptr(), s) == 0
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, 1.5, 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, -0.1, 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, float("nan"), 0, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_adapt(h, c.data_ptr(), 3, None, 0.5, 7, out.data_ptr(), s) == EINVAL
            assert lib.busca_reid_get_running_stats(h, host.ctypes.data, host.size - 2, s) == EINVAL
            ctx.check(lib.busca_reid_get_running_stats(h, host.ctypes.data, host.size, s))
            assert np.array_equal(host, good)                      # none of the refused calls touched them
            # a weight reload drops the statistics
            ctx.check(lib.busca_reid_load_weights_ex(h, blob.ctypes.data, blob.size, prec))
            assert lib.busca_reid_forward_running(h, c.data_ptr(), 3, None, 0, out.data_ptr(), s) == EINVAL
            assert b"running statistics" in lib.busca_last_error(h)
        torch.cuda.synchronize()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_second_handle_on_the_context_restores_weights_and_statistics():
    from busca_amd import _lib
    from busca_amd.reid import ReIDEncoderHIP
    g = gold()
    ctx = _lib.Context(0)
    try:
        a = ReIDEncoderHIP(ctx, synth.reid_state_dict(3), precision="f32")
        a.load_running_stats(g["r1_stats"])
        c = crops(73, 3)
        fa = a.forward_running(c).cpu().numpy()
        feat_check(fa, g["r1_eval_plain_n3"], 5e-5, "handle a")
        b = ReIDEncoderHIP(ctx, synth.reid_state_dict(4), precision="f32")              # replaces a's weights: the context has no statistics now
        with pytest.raises(_lib.BuscaError):
            b.forward_running(c)
        b.reset_running_stats()
        fb = b.forward_running(c).cpu().numpy()
        assert np.abs(fb - fa).max() > 1e-3
        assert np.array_equal(a.forward_running(c).cpu().numpy(), fa) and np.array_equal(a.running_stats(), g["r1_stats"])
        assert np.array_equal(b.forward_running(c).cpu().numpy(), fb) and np.array_equal(b.running_stats(), weights.reid_running_reset())
        # statistics an adapt() moved on the device survive the swap too
        a.adapt(crops(R2_CASE[1], R2_CASE[0]), R2_MOMENTUM)
        moved = a.running_stats()
        a.load_running_stats(g["r1_stats"])
        a.adapt(crops(R2_CASE[1], R2_CASE[0]), R2_MOMENTUM)
        b.forward_running(c)                                                              # a yields the context with its moved statistics unread
        assert np.array_equal(a.running_stats(), moved) and not np.array_equal(moved, g["r1_stats"])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conv,what", [(0, "behind the stem"), (51, "conv3's operand of the last bottleneck")])
def test_x3_running_mode_reports_operands_beyond_its_range(encs, conv, what):
    """As test_x3_reid_reports_operands_beyond_its_range, in running mode, where no consumer reads the batch statistics: the variance of one BatchNorm shrunk until
    relu(bn(.)) leaves |x| = 1023.5 - the stem's (its output is the first staged operand) and layer4.2.bn2's (conv3 of the last bottleneck stages it; no
    statistics are computed downstream).  The x3 pass raises `reid_status` 2; ReID_Encoder returns the exact-f32 extractor's features instead."""
    from busca_amd.network import ReID_Encoder
    g, m3, m32 = gold(), encs["x3"], encs["f32"]
    c = crops(75, 5)
    hot = shrink_var(g["r1_stats"], conv)
    m3.load_running_stats(g["r1_stats"])
    m3.forward_running(c)
    torch.cuda.synchronize()
    assert m3.ctx.get_option("reid_status") == 0
    m3.load_running_stats(hot)
    m3.forward_running(c)
    torch.cuda.synchronize()
    assert m3.ctx.get_option("reid_status") == 2, what
    assert m3.take_status() is True and m3.take_status() is False
    m32.load_running_stats(hot)
    want = m32.forward_running(c).cpu().numpy()
    assert np.isfinite(want).all()
    enc = ReID_Encoder(299, torch.device("cuda", 0), "no", False, "plain", False, False, precision="x3", seed=3)
    enc.load_running_stats(hot)
    cls, feats = enc(torch.from_numpy(np.array(c)))
    assert cls is None and enc.exact_reruns == 1 and np.array_equal(feats.cpu().numpy(), want)
    enc.load_running_stats(g["r1_stats"])                              # healthy statistics afterwards: the x3 pass itself, no re-run
    _, ok = enc(torch.from_numpy(np.array(c)))
    feat_check(ok.cpu().numpy(), g["r1_eval_plain_n5"], 5e-5, "ReID_Encoder x3, healthy")
    assert enc.exact_reruns == 1


@pytest.mark.gpu
def test_encoder_reruns_an_overflowed_x3_adaptation_in_f32(tmp_path):
    """A train-mode call whose batch leaves the x3 range (BatchNorm affine of layer1.0.bn1 x 4000, as test_x3_reid_reports_operands_beyond_its_range): features AND the
    update of the running statistics come from the exact-f32 extractor, started from the statistics the x3 extractor had before the call."""
    from busca_amd import _lib
    from busca_amd.network import ReID_Encoder
    from busca_amd.reid import ReIDEncoderHIP
    hot = dict(synth.reid_state_dict(3))
    hot["layer1.0.bn1.weight"] = hot["layer1.0.bn1.weight"] * 4000.0
    hot["layer1.0.bn1.bias"] = hot["layer1.0.bn1.bias"] * 4000.0
    path = str(tmp_path / "hot.pth")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in hot.items()}, path)
    c = crops(R2_CASE[1], R2_CASE[0])
    ctx = _lib.Context(0)
    try:
        exact = ReIDEncoderHIP(ctx, hot, precision="f32")
        exact.reset_running_stats()
        want = exact.adapt(c, 0.5).cpu().numpy()
        want_stats = exact.running_stats()
    finally:
        ctx.close()
    enc = ReID_Encoder(299, torch.device("cuda", 0), path, False, precision="x3")
    enc.momentum = 0.5
    _, got = enc.train()(c)
    assert enc.exact_reruns == 1 and np.isfinite(want).all()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(enc.running_stats(), want_stats)
    assert not np.array_equal(want_stats, weights.reid_running_reset())


@pytest.mark.gpu
def test_encoder_modes():
    """GHOST's modes on the standalone class: eval (default), train-mode adaptation with a momentum, batch statistics, float input."""
    from busca_amd.network import ReID_Encoder
    g = gold()
    enc = ReID_Encoder(299, torch.device("cuda", 0), "no", False, "plain", False, False, precision="x3", seed=3)
    assert np.array_equal(enc.running_stats(), weights.reid_running_reset())
    # first_batch_reset: reset, momentum 1, one train-mode call; then eval
    enc.reset_running_stats()
    enc.momentum = 1.0
    cls, f1 = enc.train()(crops(R1_CASE[1], R1_CASE[0]))
    assert cls is None
    feat_check(f1.cpu().numpy(), g["r1_feats"], 5e-5, "ReID_Encoder train-mode call")
    enc.eval()
    dm, dv = stat_gap(enc.running_stats(), g["r1_stats"])
    bm, bv = stat_bars("x3", "r1")
    assert dm <= bm and dv <= bv, (dm, bm, dv, bv)
    _, f = enc(crops(73, 3))
    feat_check(f.cpu().numpy(), g["r1_eval_plain_n3"], 5e-5, "ReID_Encoder eval call")
    _, fn = enc(crops(73, 3), output_option="norm")
    feat_check(fn.cpu().numpy(), g["r1_eval_norm_n3"], 5e-5, "ReID_Encoder eval call, norm", norm=True)
    # the reference's normalised float RGB NCHW input maps back to the same bytes
    x = crops(73, 3).astype(np.float64) / 255.0
    x = (x - np.array([0.406, 0.456, 0.485])) / np.array([0.225, 0.224, 0.299])
    xt = torch.from_numpy(x).float()[..., [2, 1, 0]].permute(0, 3, 1, 2)
    assert np.array_equal(enc(xt)[1].cpu().numpy(), f.cpu().numpy())
    assert enc.exact_reruns == 0
    # use_domain_adaptation=True: batch statistics, the features BUSCA.reid_encoder gives
    da = ReID_Encoder(299, torch.device("cuda", 0), "no", True, precision="x3", seed=3)
    feat_check(da(crops(R1_CASE[1], R1_CASE[0]))[1].cpu().numpy(), g["r1_feats"], 5e-5, "ReID_Encoder batch statistics")
    assert np.array_equal(da.running_stats(), weights.reid_running_reset())
