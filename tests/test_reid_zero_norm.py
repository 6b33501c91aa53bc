"""`zero_norm` of the ReID extractor - the per-crop flag "this crop is 0.0 AFTER normalisation" (the reference's float zero padding when normalize_ims=False) - in
busca_reid_forward_ex / _w / _forward_running / _adapt, against a float64 oracle in which a flagged crop is `x[i] = 0`.

The flag is honoured in four places (reid_preprocess_kernel, reid_preprocess_f32_kernel, the byte-fed fp16 stem and the byte-fed split-fp16 stem); every flavour is
run on every stem route it has, switched with busca_set_option between forwards of one handle.  A stem that ignored the flag, zeroed another crop, or let the byte
table's value for byte 0 (-mean / std, not 0.0) into the padding of a flagged crop moves the features by 4e-2 .. 7e-2 (the CPU tests below assert > 2e-2 for every
batch used): several times the fp16 bar, a thousand times the exact one.

Bars, none of them from a kernel's output: those of tests/test_reid_gpu.py and tests/test_reid_bn.py, imported.  Each test prints what it measured (pytest -s)."""
import contextlib

import numpy as np
import pytest
import torch

from busca_amd import synth, weights
from tests.test_reid_bn import FEAT_BAR, feat_check, gold, split, stat_bars, stat_gap
from tests.test_reid_gpu import COS_MIN, EXACT_FLAVOURS, FEAT_ATOL, _crops

# Measured once on an MI355X against the float64 oracle (max |d feature|; the bars are the imported ones and do not move with these figures):
#   each crop once      f32 2.7e-6 .. 4.0e-6;  x3 2.6e-6 .. 3.8e-6, the same on all five stem routes;  f16 4.2e-3 .. 5.6e-3 (byte-table stem, cosine >= 0.99932),
#                       4.1e-3 .. 5.4e-3 (preprocess + generic stem, cosine >= 0.99929)
#   multiplicities      f32 2.3e-6 .. 3.1e-6;  x3 1.5e-6 .. 2.7e-6 on both routes;  f16 3.6e-3 .. 6.1e-3 / 3.1e-3 .. 6.4e-3 (cosine >= 0.99946);
#                       weighted against expanded on the device: f32 <= 2.8e-6, x3 <= 1.8e-6, f16 <= 2.1e-3 (cosine >= 0.99990)
#   eval mode           plain / norm: f32 4.1e-6 / 4.1e-6, x3 4.0e-6 / 4.1e-6, f16 6.2e-3 / 6.2e-3;  a flagged crop alone against in the batch: 0, 0, 4.3e-4
#   adapt               |d mean| / sigma, |d var| / var at momentum 1: f32 7.3e-6, 3.8e-5; x3 5.7e-6, 2.8e-5; f16 9.0e-3, 5.5e-2 (bars 1.9e-5, 8.1e-5; fp16 4.5e-2, 8.9e-2);
#                       at momentum 0.1 a tenth of that;  the features are those of forward(), bit for bit
#   a stem that is handed no flags (a scratch build, both byte-fed stems) fails every test of sections 2 - 4 of its flavour.
FLAVOURS = ("f32", "x3", "f16")
# (f32 and x3: FEAT_BAR of tests/test_reid_bn.py, the 5e-5 tests/test_reid_gpu.py holds them to wherever it meets the oracle; f16: FEAT_ATOL and COS_MIN)
W_VS_EXPANDED = {"exact": 2e-5, "f16": (5e-3, 0.9998)}      # test_reid_weighted_statistics_equal_the_expanded_batch: weighted against expanded
WELL_POSED = 2e-2

# (n, flagged crops, seed of the crops)
ONCE = ((6, (1, 4), 5106), (5, (0,), 5105), (5, (4,), 5205), (8, (0, 3, 7), 5108), (2, (1,), 5102), (1, (), 5101))
# six distinct crops (seed), multiplicities, flagged crops: flagged shares 0.36, 0.75, 0.44 of the expanded batch
WEIGHTED = ((5306, (2, 5, 1, 3, 1, 2), (1,)), (5406, (1, 9, 1, 1, 3, 1), (1, 4)), (5506, (4, 1, 1, 1, 1, 1), (0,)))
EVAL = (5, (1, 4), 5605)                        # running-statistics forward
ADAPT = ONCE[0]                                 # train-mode update of the running statistics

ROUTES = {
    "f32": (("its one route", {}),),
    "f16": (("byte-table stem (reid_halo 1)", {"reid_halo": 1}), ("preprocess + generic stem (reid_halo 0)", {"reid_halo": 0})),
    "x3": tuple(("stem halo/u8/pool %d%d%d" % t, dict(zip(("reid_x3_stem_halo", "reid_x3_stem_u8", "reid_x3_stem_pool"), t)))
                for t in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1))),
}
SECOND_ROUTE = {"f16": ROUTES["f16"][1], "x3": ROUTES["x3"][3]}           # section 3 runs it next to the default

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def crops(seed, n):
    return cached(("crops", seed, n), lambda: _crops(seed, n)).copy()


def flag_array(n, flagged):
    z = np.zeros(n, np.uint8)
    z[list(flagged)] = 1
    return z


def oracle64(c, flags, **kw):
    """float64 oracle of the u8 crops `c` with the crops flagged in `flags` 0.0 after normalisation"""
    from oracle import reid as oreid
    x = oreid.crops_to_reid_input(c).clone()
    x[torch.from_numpy(flags.astype(bool))] = 0.0
    return oreid.reid_forward(synth.reid_state_dict(3), x, dtype=torch.float64, **kw)


def ref_once(case):
    """(float64 features, {bn: (mean, biased variance, samples)}) of a batch in which every crop stands once"""
    n, flagged, seed = case

    def make():
        stats = {}
        f = oracle64(crops(seed, n), flag_array(n, flagged), batch_stats=stats).numpy()
        return f, {k: (m.numpy(), v.numpy(), cnt) for k, (m, v, cnt) in stats.items()}
    return cached(("once",) + tuple(case), make)


def expanded_of(case):
    seed, counts, flagged = case
    inverse = np.repeat(np.arange(6), counts)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return crops(seed, 6), np.array(counts), flag_array(6, flagged), inverse, first


def ref_weighted(case):
    """float64 features of the expanded batch, rows at first occurrences"""
    def make():
        uniq, _counts, flags, inverse, first = expanded_of(case)
        return oracle64(uniq[inverse], flags[inverse]).numpy()[first]
    return cached(("weighted",) + tuple(case), make)


def running_r1():
    def make():
        mean, var, out, off = *split(gold()["r1_stats"]), {}, 0
        for spec in synth.reid_conv_specs():
            out[spec[6]] = (mean[off:off + spec[1]], var[off:off + spec[1]])
            off += spec[1]
        return out
    return cached("r1", make)


def ref_eval(c, flags):
    """float64 eval-mode oracle under the fixture's R1: (plain, norm)"""
    feats, stages = oracle64(c, flags, running=running_r1(), return_stages=True)
    return feats.numpy(), stages["fc7"].numpy()


def ref_eval_case():
    n, flagged, seed = EVAL
    return cached("eval", lambda: ref_eval(crops(seed, n), flag_array(n, flagged)))


def noise_like(c, seed):
    """seeded bytes, 255 (the byte table's largest entry) among them - in the image corners too, next to the stem's padding"""
    z = synth.randint_u8(seed, "zero_norm_noise", c.shape)
    z[:, ::383, ::127, :] = 255
    return z


# ---- 1. CPU: a wrong stem is visible -----------------------------------------------------------------------------------------
def check_well_posed(what, c, flags, ref, **kw):
    zeroed = c.copy()
    zeroed[flags.astype(bool)] = 0
    not_flagged = float(np.abs(oracle64(c, np.zeros_like(flags), **kw).numpy() - ref).max())
    u8_zero = float(np.abs(oracle64(zeroed, np.zeros_like(flags), **kw).numpy() - ref).max())
    print("%s: flagged vs not flagged %.3g, vs u8 zeros %.3g (more than %.1g)" % (what, not_flagged, u8_zero, WELL_POSED))
    assert not_flagged > WELL_POSED and u8_zero > WELL_POSED, (what, not_flagged, u8_zero)


@pytest.mark.parametrize("case", [c for c in ONCE if c[1]], ids=lambda c: "n%d" % c[0] + "".join("_%d" % i for i in c[1]))
def test_flag_ignored_or_taken_for_black_bytes_moves_the_oracle(case):
    n, flagged, seed = case
    check_well_posed("n=%d flags %s" % (n, set(flagged)), crops(seed, n), flag_array(n, flagged), ref_once(case)[0])


@pytest.mark.parametrize("case", WEIGHTED, ids=lambda c: "seed%d" % c[0])
def test_flag_ignored_or_taken_for_black_bytes_moves_the_oracle_with_multiplicities(case):
    uniq, counts, flags, inverse, first = expanded_of(case)
    from oracle import reid as oreid                    # (rows at first occurrences, as the GPU test reads them)

    def rows(c):
        return oreid.reid_forward(synth.reid_state_dict(3), oreid.crops_to_reid_input(c), dtype=torch.float64).numpy()[first]
    ref, zeroed = ref_weighted(case), uniq.copy()
    zeroed[flags.astype(bool)] = 0
    not_flagged, u8_zero = float(np.abs(rows(uniq[inverse]) - ref).max()), float(np.abs(rows(zeroed[inverse]) - ref).max())
    print("counts %s flags %s: flagged vs not flagged %.3g, vs u8 zeros %.3g (more than %.1g)" % (counts.tolist(), set(case[2]), not_flagged, u8_zero, WELL_POSED))
    assert not_flagged > WELL_POSED and u8_zero > WELL_POSED, (not_flagged, u8_zero)


def test_flag_ignored_or_taken_for_black_bytes_moves_the_eval_oracle():
    n, flagged, seed = EVAL
    check_well_posed("eval n=%d flags %s" % (n, set(flagged)), crops(seed, n), flag_array(n, flagged), ref_eval_case()[0], running=running_r1())


def test_eval_oracle_is_the_train_oracle_on_the_batch_s_own_statistics():
    """The oracle's eval path, checked against its train path: running statistics equal to a batch's own (biased) statistics give that batch's train-mode
    features; `batch_stats` is what supplies them."""
    from oracle import reid as oreid
    sd, x = synth.reid_state_dict(3), oreid.crops_to_reid_input(crops(5102, 2))
    stats = {}
    train = oreid.reid_forward(sd, x, dtype=torch.float64, batch_stats=stats)
    assert len(stats) == 53 and stats["bn1"][2] == 2 * 192 * 64 and stats["layer4.2.bn3"][2] == 2 * 12 * 4
    ev = oreid.reid_forward(sd, x, dtype=torch.float64, running={k: (m, v) for k, (m, v, _cnt) in stats.items()})
    as_sd = {k + s: t for k, (m, v, _cnt) in stats.items() for s, t in ((".running_mean", m), (".running_var", v))}
    assert float((ev - train).abs().max()) < 1e-12 and torch.equal(ev, oreid.reid_forward(sd, x, dtype=torch.float64, running=as_sd))
    other = oreid.reid_forward(sd, x[:1], dtype=torch.float64, running=as_sd)
    assert float((other - ev[:1]).abs().max()) < 1e-12                       # eval mode: a crop's features are its own
    assert torch.equal(oreid.reid_forward(sd, x), oreid.reid_forward(sd, x, running=None))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
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


@contextlib.contextmanager
def route(ctx, options):
    before = {k: ctx.get_option(k) for k in options}
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            ctx.set_option(k, v)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def against_oracle(got, ref, prec, what):
    """the suite's bars for batch-statistics features: 5e-5 on max |d| (f32, x3); FEAT_ATOL and cosine COS_MIN (f16)"""
    err, cos = float(np.abs(got.astype(np.float64) - ref).max()), float((got * ref).sum(1).min())
    print("%s: max |d feature| = %.3g, min cosine = %.6f" % (what, err, cos))
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    if prec in EXACT_FLAVOURS:
        assert err <= FEAT_BAR[prec], (what, err)
    else:
        assert err <= FEAT_ATOL and cos >= COS_MIN, (what, err, cos)
    return err


# ---- 2. batch statistics, each crop once -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
@pytest.mark.parametrize("case", ONCE, ids=lambda c: "n%d" % c[0] + "".join("_%d" % i for i in c[1]))
def test_flagged_crops_vs_float64_oracle(encs, case, prec):
    n, flagged, seed = case
    m, c, flags, ref = encs[prec], crops(seed, n), flag_array(n, flagged), ref_once(case)[0]
    cd, zn = dev(c), dev(flags)
    assert [m.ctx.get_option(k) for k in ROUTES[prec][0][1]] == [1] * len(ROUTES[prec][0][1])        # the first route listed is the default one
    for name, options in ROUTES[prec]:
        with route(m.ctx, options):
            got = m.forward(cd, zero_norm=zn).cpu().numpy()
        against_oracle(got, ref, prec, "%s n=%d flags %s, %s" % (prec, n, set(flagged), name))
    # the default route
    base = m.forward(cd, zero_norm=zn).cpu().numpy()
    plain = m.forward(cd).cpu().numpy()
    assert np.array_equal(m.forward(cd, zero_norm=dev(np.zeros(n, np.uint8))).cpu().numpy(), plain)                    # (b) no flag set: zero_norm=None
    if flagged:
        for what, fill in (("0", 0), ("noise", noise_like(c, seed)[flags.astype(bool)])):                              # (a) a flagged crop's bytes are not read
            other = c.copy()
            other[flags.astype(bool)] = fill
            assert np.array_equal(m.forward(dev(other), zero_norm=zn).cpu().numpy(), base), (prec, "flagged crops' bytes: " + what)
        moved = float(np.abs(base - plain).max())                                                                      # (c) the flag reached the kernel
        assert moved > FEAT_BAR[prec], (prec, moved)
    assert m.take_status() is False                                                                                    # (d)


# ---- 3. flags with multiplicities ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
@pytest.mark.parametrize("case", WEIGHTED, ids=lambda c: "seed%d" % c[0])
def test_flagged_crops_with_multiplicities_vs_float64_oracle(encs, case, prec):
    """The 5e-5 bar of the exact flavours stands against the FLOAT64 oracle: the extractor accumulates its statistics in float64, while the float32 oracle moves by
    up to 1.75e-3 with the CPU's thread count on batches in which one (zero) crop repeats - the reference's conditioning, not an allowance for the kernel."""
    uniq, counts, flags, inverse, first = expanded_of(case)
    m, ref = encs[prec], ref_weighted(case)
    ud, zn, ed, ezn = dev(uniq), dev(flags), dev(uniq[inverse]), dev(flags[inverse])
    for name, options in (ROUTES[prec][0],) + ((SECOND_ROUTE[prec],) if prec in SECOND_ROUTE else ()):
        what = "%s counts %s flags %s, %s" % (prec, counts.tolist(), set(case[2]), name)
        with route(m.ctx, options):
            w = m.forward(ud, zero_norm=zn, weights=counts).cpu().numpy()
            full = m.forward(ed, zero_norm=ezn).cpu().numpy()[first]
        gap, cos = float(np.abs(w - full).max()), float((w * full).sum(1).min())
        print("%s: weighted vs expanded on the device %.3g (cosine %.6f)" % (what, gap, cos))
        against_oracle(w, ref, prec, what)
        if prec in EXACT_FLAVOURS:
            assert gap <= W_VS_EXPANDED["exact"], (what, gap)
        else:
            assert gap <= W_VS_EXPANDED["f16"][0] and cos >= W_VS_EXPANDED["f16"][1], (what, gap, cos)
    assert m.take_status() is False


# ---- 4. running statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_flagged_crops_in_eval_mode_vs_float64_oracle(encs, prec):
    n, flagged, seed = EVAL
    m, c, flags = encs[prec], crops(seed, n), flag_array(n, flagged)
    ref = dict(zip(("plain", "norm"), ref_eval_case()))
    m.load_running_stats(gold()["r1_stats"])
    cd, zn = dev(c), dev(flags)
    for option in ("plain", "norm"):
        got = m.forward_running(cd, output=option, zero_norm=zn).cpu().numpy()
        feat_check(got, ref[option], FEAT_BAR[prec], "%s eval %s n=%d flags %s" % (prec, option, n, set(flagged)), norm=option == "norm")
        moved = float(np.abs(got - m.forward_running(cd, output=option).cpu().numpy())[list(flagged)].max())
        assert moved > FEAT_BAR[prec], (prec, option, moved)                                        # the flag reached the kernel
    # a flagged crop alone and in the batch: the bar of test_eval_features_do_not_depend_on_the_batch
    batch = m.forward_running(cd, zero_norm=zn).cpu().numpy()
    for i in flagged:
        alone = m.forward_running(cd[i:i + 1], zero_norm=zn[i:i + 1]).cpu().numpy()
        gap = float(np.abs(alone[0] - batch[i]).max())
        print("%s flagged crop %d alone vs in the batch: %.3g (bar %.1g)" % (prec, i, gap, 2 * FEAT_BAR[prec]))
        assert gap <= 2 * FEAT_BAR[prec], (prec, i, gap)
    noisy = c.copy()
    noisy[flags.astype(bool)] = noise_like(c, seed)[flags.astype(bool)]
    assert np.array_equal(m.forward_running(dev(noisy), zero_norm=zn).cpu().numpy(), batch)         # a flagged crop's bytes are not read
    assert m.take_status() is False


def restated_update(before, batch_stats, momentum):
    """torch's train-mode update in float64, in the blob's layout: (1 - m) running + m batch, the batch variance unbiased"""
    out, off = np.array(before, dtype=np.float64), 0
    for spec in synth.reid_conv_specs():
        C, (mean, var, cnt) = spec[1], batch_stats[spec[6]]
        out[off:off + C] = (1.0 - momentum) * out[off:off + C] + momentum * mean
        out[off + C:off + 2 * C] = (1.0 - momentum) * out[off + C:off + 2 * C] + momentum * var * (cnt / (cnt - 1.0))
        off += 2 * C
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("momentum,start", [(1.0, "reset"), (0.1, "r1")])
@pytest.mark.parametrize("prec", FLAVOURS)
def test_adapt_with_flagged_crops(encs, prec, momentum, start):
    """Bars of test_adapt_reproduces_the_reference_statistics: momentum 1 from reset statistics at R1's, momentum 0.1 from the fixture's R1 at R2's."""
    n, flagged, seed = ADAPT
    m, flags = encs[prec], flag_array(n, flagged)
    ref_feats, batch_stats = ref_once(ADAPT)
    cd, zn = dev(crops(seed, n)), dev(flags)
    before = weights.reid_running_reset() if start == "reset" else np.array(gold()["r1_stats"])
    m.load_running_stats(before)
    want = m.forward(cd, zero_norm=zn).cpu().numpy()
    got = m.adapt(cd, momentum, zero_norm=zn).cpu().numpy()
    after = m.running_stats()
    assert np.array_equal(got, want)                                                                # as test_adapt_with_momentum_zero_is_the_plain_forward
    against_oracle(got, ref_feats, prec, "%s adapt momentum %g, features" % (prec, momentum))
    bm, bv = stat_bars(prec, "r1" if start == "reset" else "r2")
    dm, dv = stat_gap(after, restated_update(before, batch_stats, momentum))
    print("%s adapt momentum %g: |d mean| / sigma = %.3g (bar %.3g), |d var| / var = %.3g (bar %.3g)" % (prec, momentum, dm, bm, dv, bv))
    assert dm <= bm and dv <= bv, (prec, momentum, dm, bm, dv, bv)
    raw = m.adapt(cd, 0.0, output="norm", zero_norm=zn).cpu().numpy()
    feat_check(raw / np.linalg.norm(raw, axis=1, keepdims=True), want, 1e-6, "%s norm output, normalised on the host" % prec)
    assert np.array_equal(m.running_stats(), after) and m.take_status() is False


# ---- 6. what the handle accepts as flags -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flags_of_another_dtype_device_or_length_are_refused(encs):
    m = encs["f16"]
    cd = dev(crops(ONCE[1][2], 5))
    m.load_running_stats(gold()["r1_stats"])
    calls = (lambda z: m.forward(cd, zero_norm=z), lambda z: m.forward(cd, zero_norm=z, weights=[1, 2, 1, 1, 3]), lambda z: m.forward_running(cd, zero_norm=z),
             lambda z: m.adapt(cd, 0.0, zero_norm=z))
    for call in calls:
        with pytest.raises(ValueError, match="int64"):
            call(torch.zeros(5, dtype=torch.int64, device="cuda:0"))
        with pytest.raises(ValueError, match="cpu"):
            call(torch.zeros(5, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"\(4,\)"):
            call(torch.zeros(4, dtype=torch.uint8, device="cuda:0"))
        with pytest.raises(ValueError, match=r"\(5, 1\)"):
            call(np.zeros((5, 1), np.uint8))
        with pytest.raises(ValueError, match="float64"):
            call([0.0, 1.0, 0.0, 0.0, 0.0])
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", FLAVOURS)
def test_host_flags_give_the_bits_of_device_flags(encs, prec):
    n, flagged, seed = ONCE[2]
    m, flags = encs[prec], flag_array(n, flagged)
    cd, zn = dev(crops(seed, n)), dev(flags)
    want = m.forward(cd, zero_norm=zn).cpu().numpy()
    for form in (flags, flags.astype(bool), flags.tolist(), flags.astype(np.int64) * 7, dev(flags.astype(bool))):
        assert np.array_equal(m.forward(cd, zero_norm=form).cpu().numpy(), want), type(form)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    on_side = m.forward(cd, zero_norm=flags, stream=side.cuda_stream)              # staged on the stream of the call
    side.synchronize()
    assert np.array_equal(on_side.cpu().numpy(), want)
    m.load_running_stats(gold()["r1_stats"])
    assert np.array_equal(m.forward_running(cd, zero_norm=flags).cpu().numpy(), m.forward_running(cd, zero_norm=zn).cpu().numpy())
    assert np.array_equal(m.adapt(cd, 0.0, zero_norm=flags).cpu().numpy(), want)
    assert not np.array_equal(m.forward(cd).cpu().numpy(), want) and m.take_status() is False
