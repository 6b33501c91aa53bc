"""The fused Decision-Transformer kernel's "unique rows" mode (option `dt_unique`, DESIGN.md "K-DT"): with the separator encoded as the reference the
SEP tokens of the P candidate pairs and of the NON pair are one and the same row in every layer, so the one-track-per-workgroup f32 / x3 kernel keeps
each distinct row once (T - P rows, one token tile less) and runs everything local to a token on those; K and V are still projected for every key in the
original order, each key reading the operand row of the unique row that holds it.  Every row sees the same products in the same order: logits,
probabilities, argmax and the x3 range status are BIT-identical to the kernel with the mode off (`dt_unique` = 0), whatever the shape, depth,
activation, token layout or `dt_prune`; launches that need every row (hidden states, attention maps), layouts whose separators differ and shapes the
rule excludes keep the full kernel.  `last_dt_unique` is read back every time, so no comparison can compare a run with itself."""
import os

import numpy as np
import pytest
import torch

from busca_amd import synth
from .test_dt_gpu import TOL

pytestmark = pytest.mark.gpu

KEYS = ("logits", "probs", "argmax")
PRECS = ["f32", "x3"]
_ids = lambda s: "B%d_L%d_P%d_d%d" % s


@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _tiles(L, P, nspec=2):
    return (L + 2 * (P + nspec) + 15) // 16


def _rule(L, P, nspec=2, sep_ref=True):
    """The launch rule of the mode: two token tiles or more, separators encoded as the reference, and the T - P distinct rows fit one tile less."""
    mt = _tiles(L, P, nspec)
    return int(mt >= 2 and sep_ref and L + P + 2 * nspec <= 16 * (mt - 1))


def _prune_rule(L, P, nspec=2):
    mt = _tiles(L, P, nspec)
    return int(mt >= 2 and P + nspec <= 16 * (mt - 1))


def _model(ctx, sd, prec, act="relu", f64=True, **kw):
    from busca_amd.dt import DecisionTransformerHIP
    return DecisionTransformerHIP(ctx, sd, activation=act, fake_bbox_f64=f64, precision=prec, **kw)


def _args(inp):
    return inp["mem_feat"], inp["can_feat"], inp["mem_boxes"], inp["can_boxes"]


def _forward(ctx, m, inp, **kw):
    out = m.forward(*_args(inp), **kw)
    torch.cuda.synchronize()
    assert ctx.get_option("dt_status") == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def _both(ctx, m, inp, B, want_unique, want_prune, **kw):
    """One forward with dt_unique = -1 and one with 0 on the same context, the whole batch on the one-workgroup-per-track kernel (dt_split = 0);
    `want_unique` / `want_prune`: what last_dt_unique / last_dt_prune must read after the automatic run."""
    try:
        ctx.set_option("dt_split", 0)
        ctx.set_option("dt_unique", -1)
        auto = _forward(ctx, m, inp, **kw)
        assert ctx.get_option("last_dt_unique") == want_unique and ctx.get_option("last_dt_prune") == want_prune
        assert ctx.get_option("last_dt_grid") == B and ctx.get_option("last_dt_split") == 0 and ctx.get_option("last_dt_ntrk") == 1
        ctx.set_option("dt_unique", 0)
        off = _forward(ctx, m, inp, **kw)
        assert ctx.get_option("last_dt_unique") == 0 and ctx.get_option("last_dt_prune") == want_prune
        assert ctx.get_option("last_dt_grid") == B and ctx.get_option("last_dt_split") == 0 and ctx.get_option("last_dt_ntrk") == 1
    finally:
        ctx.set_option("dt_unique", -1)
        ctx.set_option("dt_split", -1)
    for k in auto:
        assert np.array_equal(auto[k], off[k]), k
    assert (auto["argmax"] == auto["probs"].argmax(-1)).all()
    return auto


def _four(ctx, m, inp, L, P):
    """The four combinations of dt_prune and dt_unique in {0, -1}: each reads back what its rule says, all four give the same bits."""
    outs = []
    try:
        ctx.set_option("dt_split", 0)
        for prune in (0, -1):
            for unique in (0, -1):
                ctx.set_option("dt_prune", prune)
                ctx.set_option("dt_unique", unique)
                outs.append(_forward(ctx, m, inp))
                assert ctx.get_option("last_dt_unique") == (_rule(L, P) if unique else 0)
                assert ctx.get_option("last_dt_prune") == (_prune_rule(L, P) if prune else 0)
    finally:
        ctx.set_option("dt_prune", -1)
        ctx.set_option("dt_unique", -1)
        ctx.set_option("dt_split", -1)
    for o in outs[1:]:
        for k in KEYS:
            assert np.array_equal(outs[0][k], o[k]), k
    return outs[0]


def _case(B, L, P, d, nl=4, flavour="MEM-SEP-CAN-BAD"):
    seed = 900 + B + P + d + 7 * nl
    return synth.dt_state_dict(seed, d=d, ff=2 * d, nlayers=nl, flavour=flavour), synth.dt_inputs(seed, B, L, P, sentinel_every=4)


# (5, 11, 16, 64): 3 -> 2 tiles, U = 31, the tight fit; (3, 11, 9, 64): T = 33, the smallest P that reaches three tiles; (4, 11, 1, 64): 2 -> 1 tile, U = 16
# fills it exactly (no padding row); (2, 11, 24, 64): 4 -> 3 tiles; (3, 11, 16, 256): the flagship instantiation
SHAPES = [(5, 11, 16, 64), (3, 11, 9, 64), (4, 11, 1, 64), (2, 11, 24, 64), (3, 11, 16, 256)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_unique_is_bit_identical_to_every_row(ctx, shape, prec):
    B, L, P, d = shape
    assert _rule(L, P) == 1
    sd, inp = _case(B, L, P, d)
    _both(ctx, _model(ctx, sd, prec), inp, B, 1, _prune_rule(L, P))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(4, 11, 5, 64), (3, 11, 5, 512)], ids=_ids)
def test_shapes_the_rule_excludes(ctx, shape, prec):
    """T = 25 is two tiles and its U = 20 distinct rows do not fit one ((3, 11, 5, 512): the shipped shape): the full kernel runs."""
    B, L, P, d = shape
    assert _rule(L, P) == 0
    sd, inp = _case(B, L, P, d)
    _both(ctx, _model(ctx, sd, prec), inp, B, 0, _prune_rule(L, P))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nl", [1, 2, 8])
def test_unique_and_prune_switches_for_other_layer_counts(ctx, nl, prec):
    """One layer: the embed feeds a layer that is first and (pruned) last at once; eight: DT_MAX_LAYERS."""
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d, nl)
    m = _model(ctx, sd, prec)
    assert m.nlayers == nl
    _four(ctx, m, inp, L, P)


@pytest.mark.parametrize("prec", PRECS)
def test_unique_and_prune_switches_with_gelu(ctx, prec):
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    gelu = _four(ctx, _model(ctx, sd, prec, "gelu"), inp, L, P)
    relu = _four(ctx, _model(ctx, sd, prec, "relu"), inp, L, P)
    assert not np.array_equal(gelu["logits"], relu["logits"])          # the activation asked for really ran


def _layouts():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "flavours_dt.npz"))
    names = sorted({k.split("/")[0] for k in g.files if "/" in k})
    lay = [(n, str(g[n + "/flavour"]), bool(int(g[n + "/meta"][4]))) for n in names]
    # (the file has MEM-SEP-CAN-BAD only with its separators encoded as candidates; with the reference it is the default layout of every other test here)
    return lay + [("sep_can_bad", "MEM-SEP-CAN-BAD", True)]


def test_layouts_cover_both_separator_encodings():
    lay = _layouts()
    assert {(("MEM-CAN-SEP" in f), ("BAD" in f)) for _, f, s in lay if s} == {(c, b) for c in (True, False) for b in (True, False)}
    assert {"MEM-CAN-SEP" in f for _, f, s in lay if not s} == {True, False} and {"BAD" in f for _, f, s in lay if not s} == {True, False}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", _layouts(), ids=lambda v: v[0])
def test_unique_for_every_token_layout(ctx, layout, prec):
    """The token layouts of tests/golden/flavours_dt.npz at P = 12 (three tiles, 25 or 27 distinct rows): candidate first or second in its pair, with and
    without the BAD pair, whose separator is a row of its own.  Separators encoded with their candidate's box all differ: the full kernel runs."""
    _, flavour, sep_ref = layout
    B, L, P, d = 4, 11, 12, 64
    sd, inp = _case(B, L, P, d, flavour=flavour)
    m = _model(ctx, sd, prec, input_flavour=flavour, encode_separator_as_reference=sep_ref)
    want = _rule(L, P, m.nspec, sep_ref)
    assert want == int(sep_ref) and _tiles(L, P, m.nspec) == 3
    out = _both(ctx, m, inp, B, want, _prune_rule(L, P, m.nspec))
    assert out["logits"].shape == (B, P + m.nspec)


@pytest.mark.parametrize("f64", [True, False], ids=["fake_f64", "fake_f32"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_shared_separators_are_one_row_in_the_full_kernel(ctx, prec, f64):
    """The premise: in the kernel that computes every row, the hidden states of the P + 1 separators of the candidate and NON pairs are equal bit for bit
    (and the BAD pair's separator, encoded with the fake box, is not one of them)."""
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    hid = _both(ctx, _model(ctx, sd, prec, f64=f64), inp, B, 0, 0, want_hidden=True)["hidden"]
    sep = hid[:, L + 2 * np.arange(P + 2)]            # MEM-SEP-CAN-BAD: the separator comes first in its pair
    for j in range(1, P + 1):
        assert np.array_equal(sep[:, 0], sep[:, j]), j
    assert not np.array_equal(sep[:, 0], sep[:, P + 1])


@pytest.mark.parametrize("prec", PRECS)
def test_outputs_that_need_every_row_take_the_full_kernel(ctx, prec):
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    m = _model(ctx, sd, prec)
    plain = _both(ctx, m, inp, B, 1, 1)
    hid = _both(ctx, m, inp, B, 0, 0, want_hidden=True)
    att = _both(ctx, m, inp, B, 0, 0, want_att=True)
    for k in KEYS:
        assert np.array_equal(plain[k], hid[k]) and np.array_equal(plain[k], att[k]), k
    assert hid["hidden"].shape == (B, L + 2 * (P + 2), d) and att["att"].shape == (4, B, 4, L + 2 * (P + 2), L + 2 * (P + 2))


@pytest.mark.parametrize("prec", PRECS)
def test_mixed_launch_unique_rounds_and_split_tail(ctx, prec):
    """300 tracks of three tiles with the automatic options: f32 runs 256 one-workgroup tracks on the unique rows and 44 tracks on the token-split tail, which
    holds every row (x3 keeps such a tail unsplit: 300 workgroups) - equal to the launch with every switch off, bit for bit."""
    B, L, P, d = 300, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    m = _model(ctx, sd, prec)
    split, grid = (44, 256 + 132) if prec == "f32" else (0, 300)
    try:
        auto = _forward(ctx, m, inp)
        assert ctx.get_option("last_dt_unique") == 1 and ctx.get_option("last_dt_prune") == 1
        assert ctx.get_option("last_dt_split") == split and ctx.get_option("last_dt_grid") == grid
        ctx.set_option("dt_unique", 0)
        ctx.set_option("dt_prune", 0)
        ctx.set_option("dt_split", 0)
        off = _forward(ctx, m, inp)
        assert ctx.get_option("last_dt_unique") == 0 and ctx.get_option("last_dt_prune") == 0
        assert ctx.get_option("last_dt_split") == 0 and ctx.get_option("last_dt_grid") == 300
    finally:
        ctx.set_option("dt_unique", -1)
        ctx.set_option("dt_prune", -1)
        ctx.set_option("dt_split", -1)
    for k in KEYS:
        assert np.array_equal(auto[k], off[k]), k


def test_x3_range_status_is_the_same(ctx):
    """An x3 forward whose LayerNorm outputs leave the split-fp16 range (as in test_dt_gpu.test_x3_reports_operands_beyond_its_range) raises `dt_status` 2 with
    the mode on as with it off, `settle` then returns the f32 flavour's bits; a forward in range reads 0 both ways."""
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    hot = dict(sd)
    hot["transformer_encoder.layers.1.norm1.weight"] = sd["transformer_encoder.layers.1.norm1.weight"] * 3000.0
    mh = _model(ctx, hot, "x3")
    try:
        ctx.set_option("dt_split", 0)
        want = _forward(ctx, _model(ctx, hot, "f32"), inp)             # exact f32: in range by construction
        assert ctx.get_option("last_dt_unique") == 1
        for unique in (-1, 0):
            ctx.set_option("dt_unique", unique)
            o = mh.forward(*_args(inp))
            torch.cuda.synchronize()
            assert ctx.get_option("last_dt_unique") == (1 if unique else 0)
            assert ctx.get_option("dt_status") == 2, unique
            fixed = mh.settle(o)
            assert fixed is not o and ctx.get_option("dt_status") == 0
            for k in KEYS:
                assert np.array_equal(fixed[k].cpu().numpy(), want[k]), (unique, k)
        m = _model(ctx, sd, "x3")
        for unique in (-1, 0):
            ctx.set_option("dt_unique", unique)
            _forward(ctx, m, inp)                                        # (asserts dt_status == 0)
            assert ctx.get_option("last_dt_unique") == (1 if unique else 0)
    finally:
        ctx.set_option("dt_status", 0)
        ctx.set_option("dt_unique", -1)
        ctx.set_option("dt_split", -1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(8, 11, 16, 256), (5, 11, 16, 64)], ids=_ids)
def test_unique_vs_oracle(ctx, shape, prec):
    """The automatic path (read back: unique rows) against the oracle at the bars of test_dt_gpu.py."""
    from oracle import dt as odt
    B, L, P, d = shape
    sd, inp = _case(B, L, P, d)
    try:
        ctx.set_option("dt_split", 0)
        out = _forward(ctx, _model(ctx, sd, prec), inp)
        assert ctx.get_option("last_dt_unique") == 1
    finally:
        ctx.set_option("dt_split", -1)
    ref = odt.dt_forward(sd, odt.DTConfig(d=d, ff=2 * d), **inp, return_all=True)
    tol = TOL[prec]
    dl, dp = np.abs(out["logits"] - ref["logits"].numpy()).max(), np.abs(out["probs"] - ref["probs"].numpy()).max()
    print("unique vs oracle %s %s: logits %.3g probs %.3g" % (_ids(shape), prec, dl, dp))
    assert dl <= tol["logit"] and dp <= tol["prob"]
    rp = ref["probs"].numpy()
    srt = np.sort(rp, axis=-1)
    clear = (srt[:, -1] - srt[:, -2]) > tol["margin"]
    assert (out["argmax"][clear] == ref["argmax"].numpy()[clear]).all()
