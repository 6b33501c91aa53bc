"""The fused Decision-Transformer kernel's pruned last layer (option `dt_prune`, DESIGN.md "K-DT"): the decoder reads only the P + nspec
candidate rows, so the one-track-per-workgroup f32 / x3 kernel runs the token-local half of its last encoder layer (Q, attention
queries, out-proj, LayerNorms, FFN) on those rows alone, compacted into one token tile less.  Every computed row sees the same
products in the same order: logits, probabilities and argmax are BIT-identical to the unpruned kernel (`dt_prune` = 0), whatever
the shape, depth, activation or token layout; launches that need every row of the last layer (hidden states, attention maps) or
that the rule excludes do not prune.  `last_dt_prune` is read back every time, so no comparison can compare a run with itself."""
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


def _rule(L, P, nspec=2):
    """The launch rule: two token tiles or more, and the candidate rows fit one tile less."""
    mt = (L + 2 * (P + nspec) + 15) // 16
    return int(mt >= 2 and P + nspec <= 16 * (mt - 1))


def _model(ctx, sd, prec, act="relu", **kw):
    from busca_amd.dt import DecisionTransformerHIP
    return DecisionTransformerHIP(ctx, sd, activation=act, fake_bbox_f64=True, precision=prec, **kw)


def _forward(ctx, m, inp, **kw):
    out = m.forward(inp["mem_feat"], inp["can_feat"], inp["mem_boxes"], inp["can_boxes"], **kw)
    torch.cuda.synchronize()
    assert ctx.get_option("dt_status") == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def _both(ctx, m, inp, B, want_prune, **kw):
    """One forward with dt_prune = -1 and one with 0 on the same context, the whole batch on the one-workgroup-per-track kernel
    (dt_split = 0); `want_prune`: what last_dt_prune must read after the automatic run."""
    try:
        ctx.set_option("dt_split", 0)
        ctx.set_option("dt_prune", -1)
        auto = _forward(ctx, m, inp, **kw)
        assert ctx.get_option("last_dt_prune") == want_prune
        ntrk = ctx.get_option("last_dt_ntrk")
        assert ctx.get_option("last_dt_grid") == (B + ntrk - 1) // ntrk and ctx.get_option("last_dt_split") == 0
        ctx.set_option("dt_prune", 0)
        off = _forward(ctx, m, inp, **kw)
        assert ctx.get_option("last_dt_prune") == 0
    finally:
        ctx.set_option("dt_prune", -1)
        ctx.set_option("dt_split", -1)
    for k in auto:
        assert np.array_equal(auto[k], off[k]), k
    assert (auto["argmax"] == auto["probs"].argmax(-1)).all()
    return auto


def _case(B, L, P, d, nl=4, flavour="MEM-SEP-CAN-BAD"):
    seed = 700 + B + P + d + 7 * nl
    return synth.dt_state_dict(seed, d=d, ff=2 * d, nlayers=nl, flavour=flavour), synth.dt_inputs(seed, B, L, P, sentinel_every=4)


# (5, 11, 16, 64): 3 -> 2 tiles, the smallest shape with the flagship's layout; (3, 11, 16, 256): the flagship instantiation; (3, 11, 5, 512): 2 -> 1
# tile, the shipped shape, two FFN chunks; (4, 9, 4, 64): 2 -> 1 tile, L != 11; (2, 11, 24, 64): 4 -> 3 tiles, 26 decoder rows
SHAPES = [(5, 11, 16, 64), (3, 11, 16, 256), (3, 11, 5, 512), (4, 9, 4, 64), (2, 11, 24, 64)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pruned_is_bit_identical_to_unpruned(ctx, shape, prec):
    B, L, P, d = shape
    assert _rule(L, P) == 1
    sd, inp = _case(B, L, P, d)
    _both(ctx, _model(ctx, sd, prec), inp, B, 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nl", [1, 2, 8])
def test_pruned_is_bit_identical_for_other_layer_counts(ctx, nl, prec):
    """One layer: the pruned layer is fed directly by the embed (whose weight prefetch must then point at the K projection); eight: DT_MAX_LAYERS."""
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d, nl)
    m = _model(ctx, sd, prec)
    assert m.nlayers == nl
    _both(ctx, m, inp, B, 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(5, 11, 16, 64), (3, 11, 5, 512)], ids=_ids)
def test_pruned_is_bit_identical_with_gelu(ctx, shape, prec):
    B, L, P, d = shape
    sd, inp = _case(B, L, P, d)
    gelu = _both(ctx, _model(ctx, sd, prec, "gelu"), inp, B, 1)
    relu = _both(ctx, _model(ctx, sd, prec, "relu"), inp, B, 1)
    assert not np.array_equal(gelu["logits"], relu["logits"])          # the activation asked for really ran


def _layouts():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "flavours_dt.npz"))
    names = sorted({k.split("/")[0] for k in g.files if "/" in k})
    return [(n, str(g[n + "/flavour"]), bool(int(g[n + "/meta"][4]))) for n in names]


def test_layout_file_covers_every_layout_dimension():
    lay = _layouts()
    assert {"MEM-CAN-SEP" in f for _, f, _ in lay} == {True, False} and {"BAD" in f for _, f, _ in lay} == {True, False} and {s for _, _, s in lay} == {True, False}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", _layouts(), ids=lambda v: v[0])
def test_pruned_is_bit_identical_for_every_token_layout(ctx, layout, prec):
    """The token layouts of tests/golden/flavours_dt.npz (candidate first or second in its pair, with and without the BAD token, separators encoded
    with the reference box or their candidate's): the compact row of candidate j is token row L + 2 j + can_pos in each."""
    _, flavour, sep_ref = layout
    B, L, P, d = 4, 11, 5, 64
    sd, inp = _case(B, L, P, d, flavour=flavour)
    m = _model(ctx, sd, prec, input_flavour=flavour, encode_separator_as_reference=sep_ref)
    out = _both(ctx, m, inp, B, _rule(L, P, m.nspec))
    assert _rule(L, P, m.nspec) == 1 and out["logits"].shape == (B, P + m.nspec)


@pytest.mark.parametrize("prec", PRECS)
def test_outputs_that_need_every_row_do_not_prune(ctx, prec):
    """Hidden states and attention maps read every row of the last layer: such a launch runs unpruned, and its logits are the pruned launch's."""
    B, L, P, d = 5, 11, 16, 64
    sd, inp = _case(B, L, P, d)
    m = _model(ctx, sd, prec)
    plain = _both(ctx, m, inp, B, 1)
    hid = _both(ctx, m, inp, B, 0, want_hidden=True)
    att = _both(ctx, m, inp, B, 0, want_att=True)
    for k in KEYS:
        assert np.array_equal(plain[k], hid[k]) and np.array_equal(plain[k], att[k]), k
    assert hid["hidden"].shape == (B, L + 2 * (P + 2), d) and att["att"].shape == (4, B, 4, L + 2 * (P + 2), L + 2 * (P + 2))


@pytest.mark.parametrize("prec", PRECS)
def test_the_rule_decides_small_shapes(ctx, prec):
    """(4, 11, 1, 64): T = 17 is two tiles and its 3 decoder rows fit one, so by the rule (MT >= 2, P + nspec <= 16 (MT - 1)) it DOES prune - the rule is
    what is checked, not the tile count; (3, 3, 1, 64): T = 9 is one tile, nothing to drop.  Same bits either way."""
    for (B, L, P, d), want in (((4, 11, 1, 64), 1), ((3, 3, 1, 64), 0)):
        assert _rule(L, P) == want
        sd, inp = _case(B, L, P, d)
        _both(ctx, _model(ctx, sd, prec), inp, B, want)


@pytest.mark.parametrize("ntrk", [1, 2])
def test_f16_does_not_prune(ctx, ntrk):
    B, L, P, d = 5, 11, 5, 256
    sd, inp = _case(B, L, P, d)
    try:
        ctx.set_option("dt_ntrk", ntrk)
        _both(ctx, _model(ctx, sd, "f16"), inp, B, 0)
        assert ctx.get_option("last_dt_ntrk") == ntrk
    finally:
        ctx.set_option("dt_ntrk", 0)


def test_mixed_launch_pruned_rounds_and_split_tail(ctx):
    """300 tracks at the flagship shape with default options: 256 one-workgroup tracks, pruned, and 44 tracks on the token-split tail, which runs every
    layer on every row - the geometry test_token_split_tail_policy pins - equal to the same launch with dt_prune = 0, bit for bit."""
    B, L, P, d = 300, 11, 16, 256
    sd, inp = _case(B, L, P, d)
    m = _model(ctx, sd, "f32")
    try:
        auto = _forward(ctx, m, inp)
        assert ctx.get_option("last_dt_prune") == 1 and ctx.get_option("last_dt_split") == 44 and ctx.get_option("last_dt_grid") == 256 + 132
        ctx.set_option("dt_prune", 0)
        off = _forward(ctx, m, inp)
        assert ctx.get_option("last_dt_prune") == 0 and ctx.get_option("last_dt_split") == 44 and ctx.get_option("last_dt_grid") == 256 + 132
    finally:
        ctx.set_option("dt_prune", -1)
    for k in KEYS:
        assert np.array_equal(auto[k], off[k]), k


@pytest.mark.parametrize("shape", [(5, 11, 16, 64), (3, 11, 5, 512)], ids=_ids)
def test_pruned_vs_oracle(ctx, shape):
    """The automatic path (read back: pruned) against the oracle at the f32 bars of test_dt_gpu.py."""
    from oracle import dt as odt
    B, L, P, d = shape
    sd, inp = _case(B, L, P, d)
    try:
        ctx.set_option("dt_split", 0)
        out = _forward(ctx, _model(ctx, sd, "f32"), inp)
        assert ctx.get_option("last_dt_prune") == 1
    finally:
        ctx.set_option("dt_split", -1)
    ref = odt.dt_forward(sd, odt.DTConfig(d=d, ff=2 * d), **inp, return_all=True)
    tol = TOL["f32"]
    dl, dp = np.abs(out["logits"] - ref["logits"].numpy()).max(), np.abs(out["probs"] - ref["probs"].numpy()).max()
    print("pruned vs oracle %s: logits %.3g probs %.3g" % (_ids(shape), dl, dp))
    assert dl <= tol["logit"] and dp <= tol["prob"]
    rp = ref["probs"].numpy()
    srt = np.sort(rp, axis=-1)
    clear = (srt[:, -1] - srt[:, -2]) > tol["margin"]
    assert (out["argmax"][clear] == ref["argmax"].numpy()[clear]).all()
