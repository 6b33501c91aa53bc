"""GHOST's linear motion model on the device: busca_ghost_motion_append / _warp / _step (include/busca_ghost_motion.h) and their mirrors in
busca_amd.tracking (GhostMotion, ghost_motion_check_config, ghost_round(det_boxes=...)).

The reference is tests/golden/ghost_motion.npz, written by tests/golden/make_golden_ghost_motion.py from the reference's own Track, motion(),
motion_step, motion_compensation and get_motion_dist: two scripted sequences with the reference's full state recorded before and after every
operation of every frame.  Each device operation is run ONCE from a recorded state and compared with the next recorded state, so an error cannot
hide behind an earlier one; the replay test then runs a whole sequence through GhostMotion with rings that wrap.

Bars, none of them taken from a kernel's output:
  * step, append, motion cost: exact.  The generator asserts that a sequential float64 restatement (oldest pair first) has the reference's bits, and
    that oracle.geometry.iou_distance - what busca_pairwise is tested against - has the bits of get_motion_dist.
  * warp: warp_err + one float32 ulp of the largest |coordinate|.  The device evaluates W . (x, y, 1) in float64 and rounds once to float32 (within
    half a float32 ulp of the exact value); the reference rounds the corner to float32 and runs a float32 torch.mm, and warp_err is the largest
    distance of its output from a float64 evaluation, recorded by the generator.
  * edge shapes: np_step below, the numpy restatement that the CPU test pins to both recorded sequences (float64 and float32 differences)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from tests.test_streams_gpu import behind, busy, ctx  # noqa: F401  (busy, ctx: fixtures)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ghost_motion.npz")
KEYS = ("hist", "frames", "count", "newest", "pos", "vel")
SEQ = {"static": 0, "moving": 1}            # sequence -> diff32 of its steps
NAMES = {"busca_ghost_motion_append": 17, "busca_ghost_motion_warp": 10, "busca_ghost_motion_step": 16}

_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
        for v in _CACHE["g"].values():
            v.setflags(write=False)
    return _CACHE["g"]


def recorded(name, f, stage):
    g = gold()
    return {k: g["%s_%s" % (name, k)][f, stage] for k in KEYS}


def frame_of(name, f):
    """-> (slots [n], num_active, dets [m,4], dist [m,n], adds [k,3])"""
    g = gold()
    n, m, k = (int(v) for v in g[name + "_nmk"][f])
    return g[name + "_slots"][f, :n], int(g[name + "_na"][f]), g[name + "_dets"][f, :m], g[name + "_dist"][f, :m, :n], g[name + "_add"][f, :k]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def np_step(st, slots, na, last_n, diff32):
    """busca_ghost_motion_step in numpy, one scalar operation at a time -> (pos [S,4], vel [S,4], out [n,4])."""
    S, H = st["frames"].shape
    pos, vel, out = st["pos"].copy(), st["vel"].copy(), np.full((len(slots), 4), np.nan)
    with np.errstate(all="ignore"):
        for i, s in enumerate(slots):
            if not 0 <= s < S:
                continue
            cnt, nw = int(st["count"][s]), int(st["newest"][s])
            if cnt > 1:
                if i < na:
                    w = min(cnt, last_n)
                    rows = [(nw - (w - 1) + k) % H for k in range(w)]
                    for c in range(4):
                        acc = None
                        for a, b in zip(rows, rows[1:]):
                            p0, p1 = st["hist"][s, a, c], st["hist"][s, b, c]
                            d = np.float64(np.float32(p1) - np.float32(p0)) if diff32 else p1 - p0
                            q = d / np.float64(int(st["frames"][s, b]) - int(st["frames"][s, a]))
                            acc = q if acc is None else acc + q
                        vel[s, c] = acc / np.float64(w - 1)
                pos[s] = pos[s] + vel[s]
            out[i] = pos[s]
    return pos, vel, out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_typed_and_exported():
    from busca_amd.build import build
    build()
    from busca_amd import _lib

    def declared(header):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(busca_[a-z0-9_]+)\s*\(", hdr))
    assert declared("busca_ghost_motion.h") == set(NAMES) == set(_lib.GHOST_MOTION_SIGNATURES)
    for header, table in _lib.HEADERS.items():
        if header == "busca_ghost_motion.h":
            continue
        assert not set(NAMES) & declared(header) and not set(NAMES) & set(table)
    lib = _lib.load()
    for name, nargs in NAMES.items():
        fn = getattr(lib, name)                                            # exported
        assert fn.restype is not None and len(fn.argtypes) == nargs == len(_lib.GHOST_MOTION_SIGNATURES[name][1])
    assert lib.busca_version() >= 2005 and lib.busca_version() // 1000 == 2


def test_mirrors_reachable_from_the_alias_package():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.tracking as bt
    finally:
        sys.path.pop(0)
    for name in ("GhostMotion", "ghost_motion_check_config", "ghost_round"):
        assert callable(getattr(bt, name)), name
    for name in ("add", "compensate", "step", "cost"):
        assert callable(getattr(bt.GhostMotion, name)), name


def test_check_config_refuses_the_broken_branches():
    from busca_amd.tracking import ghost_check_config, ghost_motion_check_config
    ok = {"apply_motion_model": True, "combi": "sum_0.4", "center_only": False, "last_n_frames": 3}
    assert ghost_motion_check_config(ok) is ok and ghost_motion_check_config({}) == {}
    with pytest.raises(ValueError, match="IndexError"):
        ghost_motion_check_config(dict(ok, center_only=True))
    with pytest.raises(ValueError, match="AttributeError"):
        ghost_motion_check_config(dict(ok, approximate=True))
    with pytest.raises(ValueError, match="only_vel"):
        ghost_motion_check_config(ok, kalman=True)
    cfg = {"use_bism": False, "distance": "cosine", "motion_config": dict(ok, center_only=True)}
    assert ghost_check_config(cfg) is cfg                                  # the association check is what it was


def test_fixture_contents():
    g = gold()
    F = len(g["static_frame"])
    assert F == 12 and set(np.diff(g["static_frame"])) == {1, 2, 3} and np.array_equal(g["static_frame"], g["moving_frame"])
    assert g["static_params"].tolist() == [4, 3] and g["moving_params"].tolist() == [16, 100000000]
    assert 0.0 < float(g["warp_err"][0]) < 1e-3
    for name in SEQ:
        H = int(g[name + "_params"][0])
        assert g[name + "_hist"].shape == (F, 4, 8, H, 4) and g[name + "_frames"].dtype == np.int32 and g[name + "_pos"].dtype == np.float64
        nmk = g[name + "_nmk"]
        assert nmk[:, 1].min() >= 5 and nmk[:, 1].max() <= 7 and nmk[-1, 0] == 8
        for f in range(F):
            slots, na, dets, dist, adds = frame_of(name, f)
            assert len(set(slots.tolist())) == len(slots) and 0 <= na <= len(slots) and dist.shape == (len(dets), len(slots))
            assert np.isfinite(dist).all() and (len(slots) == 0 or dist.min() < 0.5)       # the model tracks: some detection overlaps its track
            for k in KEYS:                                                                  # the stages chain
                a = g["%s_%s" % (name, k)]
                assert f + 1 == F or same(a[f, 3], a[f + 1, 0])
                assert name == "moving" or same(a[f, 0], a[f, 1])
                assert k in ("pos", "vel") or same(a[f, 1], a[f, 2])                        # a step changes pos and vel only
        cnt = g[name + "_count"][:, 1]
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 2).any() and cnt.max() == min(H, 11)           # (the twelfth row joins after the last step)
        assert (g[name + "_add"][:, :, 2] == 1).sum() == 8 and (g[name + "_add"][4:, :, 2] == 1).sum() == 2     # two tracks start mid-sequence
        assert g[name + "_count"][-1, 3, 5] == 1                                            # one track never gets a second position
        inactive_moved = [f for f in range(F) if g[name + "_na"][f] < g[name + "_nmk"][f, 0]]
        assert len(inactive_moved) >= 8
    assert (g["static_newest"][:, 1] < g["static_count"][:, 1] - 1).any()                  # a wrapped ring
    assert g["static_f32"].sum() == 0 and (g["moving_f32"][1:] == (g["moving_count"][1:, 1] > 0)).all()
    moved = g["moving_hist"][1:, 1] != g["moving_hist"][1:, 0]
    assert moved.any(axis=(1, 2, 3)).all() and len({g["moving_warp"][f].tobytes() for f in range(1, F)}) == F - 1


@pytest.mark.parametrize("name", list(SEQ))
def test_recorded_steps_equal_the_sequential_restatement(name):
    """The summation order and the dtype rule of the header, stated in numpy (np_step), reproduce every recorded step bit for bit: float64
    differences in `static`, float32 differences in `moving`."""
    g = gold()
    last_n = int(g[name + "_params"][1])
    crossed = 0
    for f in range(len(g[name + "_frame"])):
        slots, na, _, _, _ = frame_of(name, f)
        pre, post = recorded(name, f, 1), recorded(name, f, 2)
        pos, vel, out = np_step(pre, slots, na, last_n, SEQ[name])
        assert same(pos, post["pos"]) and same(vel, post["vel"]) and same(out, post["pos"][slots]), (name, f)
        crossed += int(not same(np_step(pre, slots, na, last_n, 1 - SEQ[name])[1], post["vel"]))
    # `static` rows are not float32 numbers: the float32 rule gives other bits.  `moving` rows are, and the float32 difference of two float32 numbers this
    # close is exact, so there both rules agree; the edge-shape tests, whose rows are not float32 numbers, tell the two apart on the device
    assert crossed >= 8 if name == "static" else crossed == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def model(st, diff32=0):
    """A GhostMotion holding copies of the state arrays `st`."""
    import torch
    from busca_amd import tracking
    S, H = st["frames"].shape
    gm = tracking.GhostMotion(S, H, ctx=model.ctx)
    for k in KEYS:
        getattr(gm, k).copy_(torch.from_numpy(np.array(st[k])))
    gm.all_warped = bool(diff32)
    return gm


def state_of(gm):
    return {k: getattr(gm, k).cpu().numpy() for k in KEYS}


def assert_state(gm, want, what, only=KEYS):
    got = state_of(gm)
    for k in only:
        assert same(got[k], np.asarray(want[k])), (what, k)


@pytest.fixture(autouse=True)
def _ctx_for_model(request):
    if "gpu" in request.keywords:
        model.ctx = request.getfixturevalue("ctx")
    yield


@gpu
@pytest.mark.parametrize("name", list(SEQ))
def test_step_and_cost_from_every_recorded_state(name):
    g = gold()
    last_n = int(g[name + "_params"][1])
    for f in range(len(g[name + "_frame"])):
        slots, na, dets, dist, _ = frame_of(name, f)
        pre, post = recorded(name, f, 1), recorded(name, f, 2)
        gm = model(pre, SEQ[name])
        out = gm.step(slots, na, last_n).cpu().numpy()
        assert same(out, post["pos"][slots]), (name, f)
        assert_state(gm, post, (name, f))                                  # pos and vel stepped, the rings as they were
        gm = model(pre, SEQ[name])
        cost = gm.cost(slots, na, dets, last_n).cpu().numpy()
        assert same(cost, np.ascontiguousarray(dist.T)), (name, f)
        assert_state(gm, post, (name, f, "cost"))


@gpu
@pytest.mark.parametrize("name", list(SEQ))
def test_append_from_every_recorded_state(name):
    import torch
    g = gold()
    for f in range(len(g[name + "_frame"])):
        _, _, dets, _, adds = frame_of(name, f)
        pre, post = recorded(name, f, 2), recorded(name, f, 3)
        gm = model(pre)
        fresh = torch.from_numpy(adds[adds[:, 2] == 1, 0].astype(np.int64)).to(gm.dev)
        gm.count[fresh], gm.newest[fresh], gm.vel[fresh] = 3, 2, 7.0       # what an earlier tenant of a new track's slot left behind
        gm.add(adds[:, 0], dets, int(g[name + "_frame"][f]), det_index=adds[:, 1], new=adds[:, 2])
        assert_state(gm, post, (name, f))
        assert not gm.diff32
        gm = model(pre)                                                    # the same add with slots, detection indices and flags as device tensors
        gm.count[fresh], gm.newest[fresh], gm.vel[fresh] = 3, 2, 7.0
        on_dev = [torch.from_numpy(np.array(adds[:, i])).to(gm.dev) for i in range(3)]
        gm.add(on_dev[0], torch.from_numpy(np.array(dets)).to(gm.dev), int(g[name + "_frame"][f]), det_index=on_dev[1], new=on_dev[2].to(torch.uint8))
        assert_state(gm, post, (name, f, "device tensors"))
    # without det_index the i-th box goes to the i-th slot; a negative slot and a detection index beyond the boxes are skipped
    _, _, dets, _, _ = frame_of(name, 5)
    pre = recorded(name, 5, 2)
    gm = model(pre)
    gm.add([2, -1, 0], dets[:3], 77)
    got = state_of(gm)
    H = pre["frames"].shape[1]
    for s, j in ((2, 0), (0, 2)):
        row = (int(pre["newest"][s]) + 1) % H
        assert same(got["pos"][s], dets[j]) and same(got["hist"][s, row], dets[j]) and got["frames"][s, row] == 77 and got["newest"][s] == row
        assert got["count"][s] == min(int(pre["count"][s]) + 1, H) and same(got["vel"][s], pre["vel"][s])
    rest = [s for s in range(8) if s not in (0, 2)]
    for k in KEYS:
        assert same(got[k][rest], pre[k][rest]), k
    before = state_of(gm)
    gm.add([1, 3], dets[:3], 78, det_index=[3, -1])                        # index 3 of 3 boxes, index -1
    assert_state(gm, before, "skipped pairs")


@gpu
def test_warp_from_every_recorded_state():
    g = gold()
    for f in range(1, len(g["moving_frame"])):
        pre, post = recorded("moving", f, 0), recorded("moving", f, 1)
        gm = model(pre)
        listed = None if f % 2 else np.arange(8)[::-1]                     # all slots / an explicit list
        gm.compensate(g["moving_warp"][f].reshape(2, 3), listed)
        assert gm.diff32 == (listed is None)
        got = state_of(gm)
        bar = float(g["warp_err"][0]) + float(np.spacing(np.float32(np.abs(post["hist"]).max())))
        err = float(np.abs(got["hist"] - post["hist"]).max())
        print("warp frame %d: max |device - reference| %.3g, bar %.3g" % (f, err, bar))
        assert err <= bar
        assert same(got["hist"], got["hist"].astype(np.float32).astype(np.float64))         # rounded once to float32
        valid = np.arange(16)[None, :] < pre["count"][:, None]             # (these rings have not wrapped)
        assert same(got["hist"][~valid], pre["hist"][~valid])
        assert_state(gm, pre, f, only=("frames", "count", "newest", "pos", "vel"))          # pos is not warped
    # a listed subset leaves the other slots alone; a negative entry is skipped
    pre = recorded("moving", 9, 0)
    gm = model(pre)
    gm.compensate(g["moving_warp"][9], [6, -1, 1])
    got = state_of(gm)
    post = recorded("moving", 9, 1)
    assert same(got["hist"][[0, 2, 3, 4, 5, 7]], pre["hist"][[0, 2, 3, 4, 5, 7]])
    assert np.abs(got["hist"][[1, 6]] - post["hist"][[1, 6]]).max() <= bar and (got["hist"][[1, 6]] != pre["hist"][[1, 6]]).any()


@gpu
def test_wrapped_ring_is_warped_row_by_row():
    """Every valid row of a wrapped ring moves exactly once, rows that hold nothing stay."""
    g = gold()
    pre = recorded("static", 11, 0)
    assert (pre["newest"] < pre["count"] - 1).any() and (pre["count"] == 1).any()
    gm = model(pre)
    W = np.array([[1.0, 0.0, 8.0], [0.0, 1.0, -16.0]], dtype=np.float32)
    gm.compensate(W)
    got = state_of(gm)
    H = 4
    for s in range(8):
        cnt, nw = int(pre["count"][s]), int(pre["newest"][s])
        rows = {(nw - k) % H for k in range(cnt)}
        for r in range(H):
            want = pre["hist"][s, r]
            if r in rows:
                want = (want + np.array([8.0, -16.0, 8.0, -16.0])).astype(np.float32).astype(np.float64)
            assert same(got["hist"][s, r], want), (s, r)


@gpu
def test_replay_of_the_static_sequence():
    """add / cost over all twelve frames with H = 4: the rings wrap, `newest` walks, tracks leave and return."""
    from busca_amd import tracking
    g = gold()
    gm = tracking.GhostMotion(8, 4, ctx=model.ctx)
    for f in range(len(g["static_frame"])):
        slots, na, dets, dist, adds = frame_of("static", f)
        assert_state(gm, recorded("static", f, 1), (f, "before"))
        if len(slots):
            cost = gm.cost(slots, na, dets, 3).cpu().numpy()
            assert same(cost, np.ascontiguousarray(dist.T)), f
        assert_state(gm, recorded("static", f, 2), (f, "stepped"))
        gm.add(adds[:, 0], dets, int(g["static_frame"][f]), det_index=adds[:, 1], new=adds[:, 2])
        assert_state(gm, recorded("static", f, 3), (f, "added"))


def edge_state():
    """S = 6 slots, H = 5: counts 0, 1, 2 and three full rings whose newest row sits at the end, in the middle and at the start."""
    from busca_amd import synth
    S, H = 6, 5
    st = dict(hist=synth.uniform(60, "hist", (S, H, 4), 0, 1000).astype(np.float64) * (1 + 2.0 ** -30), count=np.array([0, 1, 2, 5, 5, 5], np.int32),
              newest=np.array([0, 0, 1, 4, 2, 0], np.int32), pos=synth.uniform(60, "pos", (S, 4), 0, 1000).astype(np.float64),
              vel=synth.uniform(60, "vel", (S, 4), -5, 5).astype(np.float64), frames=np.zeros((S, H), np.int32))
    gaps = 1 + (synth.uniform(60, "gap", (S, H), 0, 3).astype(np.int32) % 3)
    for s in range(S):
        for k in range(H):                                                 # frames ascend in chronological order
            st["frames"][s, (int(st["newest"][s]) + 1 + k) % H] = 10 * s + int(gaps[s, :k + 1].sum())
    return st


def raw_step(c, gm, slots, na, last_n, diff32, n=None, S=None, H=None, out_shift=0):
    import torch
    slot = torch.from_numpy(np.asarray(slots, dtype=np.int32)).to(gm.dev)
    n = len(slots) if n is None else n
    out = torch.full((max(n, 0) + 1, 4), -7.0, dtype=torch.float64, device=gm.dev)
    c.check(c.lib.busca_ghost_motion_step(c.h, gm.hist.data_ptr(), gm.frames.data_ptr(), gm.count.data_ptr(), gm.newest.data_ptr(), gm.pos.data_ptr(),
                                          gm.vel.data_ptr(), gm.capacity if S is None else S, gm.history if H is None else H, slot.data_ptr(), n, na, last_n,
                                          diff32, out.data_ptr() + out_shift, None))
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize("diff32", [0, 1])
@pytest.mark.parametrize("last_n", [2, 10], ids=["pairs", "beyond_H"])
@pytest.mark.parametrize("active", ["none", "all", "some"])
def test_step_edge_shapes(ctx, active, last_n, diff32):
    st = edge_state()
    slots = [4, -1, 2, 0, 5, 6, 3, 1]                                      # permuted; a negative entry and one at S: skipped
    na = {"none": 0, "all": len(slots), "some": 4}[active]
    gm = model(st)
    out = raw_step(ctx, gm, slots, na, last_n, diff32)
    pos, vel, want = np_step(st, slots, na, last_n, diff32)
    assert same(out[:-1], want) and (out[-1] == -7.0).all()
    if na:                                                                 # on these rows the two difference rules give other bits: diff32 is told apart
        assert not same(np_step(st, slots, na, last_n, 0)[1], np_step(st, slots, na, last_n, 1)[1])
    assert np.isnan(want[[1, 5]]).all() and np.isfinite(np.delete(want, [1, 5], 0)).all()
    assert_state(gm, dict(st, pos=pos, vel=vel), (active, last_n, diff32))
    assert same(pos[:2], st["pos"][:2]) and same(vel[:2], st["vel"][:2])    # counts 0 and 1: untouched
    moved = [s for s in (2, 3, 4, 5)]
    assert (pos[moved] != st["pos"][moved]).all()
    assert same(vel, st["vel"]) == (active == "none")


@gpu
def test_step_of_nothing_and_equal_frames(ctx):
    st = edge_state()
    gm = model(st)
    assert gm.step([], 0, 3).shape == (0, 4)
    assert (raw_step(ctx, gm, [], 0, 3, 0) == -7.0).all()
    assert_state(gm, st, "n = 0")
    st["frames"] = st["frames"].copy()
    st["frames"][3, :] = 7                                                 # frame difference 0: inf / NaN as numpy gives them
    st["hist"] = st["hist"].copy()
    st["hist"][3, :, 1] = 5.0                                              # 0 / 0 in coordinate 1
    gm = model(st)
    out = raw_step(ctx, gm, [3], 1, 10, 0)
    pos, vel, want = np_step(st, [3], 1, 10, 0)
    assert same(out[:1], want) and np.isnan(want[0, 1]) and not np.isfinite(want[0]).any()
    assert_state(gm, dict(st, pos=pos, vel=vel), "equal frames")


@gpu
def test_invalid_arguments(ctx):
    import torch
    from busca_amd import _lib, tracking
    st = edge_state()
    gm = model(st)
    for kw, msg in ((dict(n=-1), "n -1"), (dict(S=-1), "negative"), (dict(H=1), "at least 2 rows"), (dict(H=-3), "negative"),
                    (dict(out_shift=4), "misaligned")):
        with pytest.raises(_lib.BuscaError, match=msg):
            raw_step(ctx, gm, [0, 1], 1, 3, 0, **kw)
    for last_n in (1, 0, -2):
        with pytest.raises(_lib.BuscaError, match="last_n_frames"):
            raw_step(ctx, gm, [0, 1], 1, last_n, 0)
    for na in (-1, 3):
        with pytest.raises(_lib.BuscaError, match="num_active"):
            raw_step(ctx, gm, [0, 1], na, 3, 0)
    lib, h, p = ctx.lib, ctx.h, lambda t: t.data_ptr()
    slot = torch.tensor([0, 1], dtype=torch.int32, device=gm.dev)
    boxes = torch.zeros(2, 4, dtype=torch.float64, device=gm.dev)
    out = torch.zeros(2, 4, dtype=torch.float64, device=gm.dev)
    W = np.eye(2, 3, dtype=np.float32)
    S, H = gm.capacity, gm.history
    state = (p(gm.hist), p(gm.frames), p(gm.count), p(gm.newest), p(gm.pos), p(gm.vel))
    bad = [
        ("null", lambda: lib.busca_ghost_motion_step(h, None, *state[1:], S, H, p(slot), 2, 1, 3, 0, p(out), None)),
        ("null", lambda: lib.busca_ghost_motion_step(h, *state, S, H, None, 2, 1, 3, 0, p(out), None)),
        ("null", lambda: lib.busca_ghost_motion_step(h, *state, S, H, p(slot), 2, 1, 3, 0, None, None)),
        ("misaligned", lambda: lib.busca_ghost_motion_step(h, *state[:2], state[2] + 2, *state[3:], S, H, p(slot), 2, 1, 3, 0, p(out), None)),
        ("null", lambda: lib.busca_ghost_motion_append(h, *state, S, H, None, None, None, 2, p(boxes), 2, 5, None)),
        ("null", lambda: lib.busca_ghost_motion_append(h, *state, S, H, p(slot), None, None, 2, None, 2, 5, None)),
        ("null", lambda: lib.busca_ghost_motion_append(h, *state[:4], None, state[5], S, H, p(slot), None, None, 2, p(boxes), 2, 5, None)),
        ("k -2", lambda: lib.busca_ghost_motion_append(h, *state, S, H, p(slot), None, None, -2, p(boxes), 2, 5, None)),
        ("negative", lambda: lib.busca_ghost_motion_append(h, *state, S, H, p(slot), None, None, 2, p(boxes), -1, 5, None)),
        ("at least 2 rows", lambda: lib.busca_ghost_motion_append(h, *state, S, 0, p(slot), None, None, 2, p(boxes), 2, 5, None)),
        ("misaligned", lambda: lib.busca_ghost_motion_append(h, *state, S, H, p(slot), None, None, 2, p(boxes) + 4, 2, 5, None)),
        ("null", lambda: lib.busca_ghost_motion_warp(h, None, state[2], state[3], S, H, None, 0, W.ctypes.data, None)),
        ("null", lambda: lib.busca_ghost_motion_warp(h, state[0], state[2], state[3], S, H, None, 0, None, None)),
        ("negative", lambda: lib.busca_ghost_motion_warp(h, state[0], state[2], state[3], S, H, p(slot), -1, W.ctypes.data, None)),
        ("at least 2 rows", lambda: lib.busca_ghost_motion_warp(h, state[0], state[2], state[3], S, 1, None, 0, W.ctypes.data, None)),
        ("misaligned", lambda: lib.busca_ghost_motion_warp(h, state[0] + 4, state[2], state[3], S, H, None, 0, W.ctypes.data, None)),
    ]
    for msg, call in bad:
        rc = call()
        assert rc == -1 and msg in lib.busca_last_error(h).decode(), (msg, rc, lib.busca_last_error(h).decode())
    torch.cuda.synchronize()
    assert_state(gm, st, "refused calls write nothing")
    # nothing to do: 0 and no launch
    assert lib.busca_ghost_motion_append(h, *state, S, H, p(slot), None, None, 0, p(boxes), 2, 5, None) == 0
    assert lib.busca_ghost_motion_warp(h, state[0], state[2], state[3], S, H, p(slot), 0, W.ctypes.data, None) == 0
    # the wrapper's host checks
    for call in (lambda: gm.step([1, 1], 1, 3), lambda: gm.step([0, 6], 1, 3), lambda: gm.add([2, 2], np.zeros((2, 4)), 1),
                 lambda: gm.add([9], np.zeros((1, 4)), 1), lambda: gm.compensate(W, [3, 3]), lambda: gm.add([0, 1, 2], np.zeros((2, 4)), 1),
                 lambda: tracking.GhostMotion(4, 1, ctx=ctx), lambda: tracking.GhostMotion(4, 4, box_dtype=np.float16, ctx=ctx)):
        with pytest.raises(ValueError):
            call()
    assert_state(gm, st, "refused wrapper calls write nothing")


@gpu
def test_box_dtype_float32_takes_float32_differences(ctx):
    from busca_amd import tracking
    st = edge_state()
    gm = tracking.GhostMotion(6, 5, box_dtype=np.float32, ctx=ctx)
    assert gm.diff32
    boxes = st["hist"][:, 0]                                               # not float32-representable: add() rounds them as the reference's dtype does
    for t in range(3):
        gm.add(np.arange(6), boxes + 3.7 * t, 2 * t)
    got = state_of(gm)
    assert same(got["hist"][:, 1], (boxes + 3.7).astype(np.float32).astype(np.float64))
    out = gm.step(np.arange(6), 6, 5).cpu().numpy()
    assert same(out, np_step(got, list(range(6)), 6, 5, 1)[2])


@gpu
def test_ghost_round_runs_the_motion_model_itself(ctx):
    """ghost_round(state with motion_state, det_boxes=...) = ghost_round(motion=<GhostMotion.cost computed separately>): same dist bits, same matches."""
    from busca_amd import synth, tracking
    from tests.test_ghost_round import ROUND_CFG, round_state
    from tests.test_streams_gpu import _boxes
    state, det, labels, seed, n, m, na = round_state(0)
    cfg = dict(ROUND_CFG[0], nan_first=True, distance="cosine", use_bism=False)
    cfg["motion_config"] = dict(cfg["motion_config"], last_n_frames=3)
    base = _boxes(seed, n)
    drift = synth.uniform(seed, "drift", (n, 4), -4, 4).astype(np.float64)
    det_boxes = np.concatenate([base[:m] + 3 * drift[:m], _boxes(seed + 1, max(m - n, 0))])[:m]

    def motion_state():
        gm = tracking.GhostMotion(n + 3, 4, ctx=ctx)
        for t in range(3):
            gm.add(np.arange(n)[t % 2:], base + t * drift, 1 + 2 * t, det_index=np.arange(n)[t % 2:], new=None)      # track 0 has two samples
        return gm
    slots = np.arange(n)
    motion = motion_state().cost(slots, na, det_boxes, 3)
    assert np.isfinite(motion.cpu().numpy()).all() and float(motion.min()) < 0.5
    want = tracking.ghost_round(state, det, labels, motion, cfg, ctx=ctx)
    with pytest.raises(ValueError, match="motion cost"):
        tracking.ghost_round(state, det, labels, None, cfg, ctx=ctx)
    for slot in (None, slots):
        st = types.SimpleNamespace(gallery=state.gallery, count=state.count, newest=state.newest, slot=slot, num_active=na, motion_state=motion_state())
        with pytest.raises(ValueError, match="motion cost"):
            tracking.ghost_round(st, det, labels, None, cfg, ctx=ctx)      # no det_boxes: as before
        got = tracking.ghost_round(st, det, labels, None, cfg, ctx=ctx, det_boxes=det_boxes)
        assert same(got[0].cpu().numpy(), want[0].cpu().numpy()) and same(got[1], want[1]) and same(got[2], want[2])
        assert len(got[1]) >= 5
        with pytest.raises(ValueError, match="IndexError"):
            tracking.ghost_round(st, det, labels, None, dict(cfg, motion_config=dict(cfg["motion_config"], center_only=True)), ctx=ctx, det_boxes=det_boxes)
        with pytest.raises(ValueError, match="only_vel"):
            tracking.ghost_round(st, det, labels, None, dict(cfg, kalman=True), ctx=ctx, det_boxes=det_boxes)
    other = tracking.ghost_round(state, det, labels, motion.flip(0).contiguous(), cfg, ctx=ctx)
    assert not same(other[0].cpu().numpy(), want[0].cpu().numpy())         # the motion cost takes part in the result


# ---- stream order ---------------------------------------------------------------------------------------------------------
def _stream_state():
    """(true, poison) of hist, frames, count, newest, pos, vel: frame 9 of `static` before its step; empty rings full of NaN as poison."""
    import torch
    from tests.test_streams_gpu import _dev, _nan
    true = [_dev(np.array(recorded("static", 9, 1)[k])) for k in KEYS]
    poison = [_nan(true[0]), torch.zeros_like(true[1]), torch.zeros_like(true[2]), torch.full_like(true[3], 3), _nan(true[4]), _nan(true[5])]
    return true, poison


@gpu
def test_stream_order_append(ctx, busy):
    import torch
    from tests.test_streams_gpu import _dev, _nan
    true, poison = _stream_state()
    _, _, dets, _, adds = frame_of("static", 9)
    slot, det, new, boxes = _dev(adds[:, 0]), _dev(adds[:, 1]), _dev(adds[:, 2].astype(np.uint8)), _dev(np.array(dets))
    k, m = len(adds), len(dets)
    true += [slot, det, new, boxes]
    poison += [slot.flip(0).contiguous(), torch.zeros_like(det), torch.ones_like(new), _nan(boxes)]
    want, _ = behind(busy, "busca_ghost_motion_append", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_motion_append(
        ctx.h, *[t.data_ptr() for t in x[:6]], 8, 4, x[6].data_ptr(), x[7].data_ptr(), x[8].data_ptr(), k, x[9].data_ptr(), m, 16, st)), true, poison)
    post = recorded("static", 9, 3)                                        # (frame 9's step has not run here: only the rings and the new positions are stage 3's)
    for i, key in enumerate(KEYS[:4]):
        assert same(want[i], post[key]), key
    assert same(want[4][adds[:, 0]], post["pos"][adds[:, 0]])


@gpu
def test_stream_order_warp(ctx, busy):
    import torch
    true, poison = _stream_state()
    W = np.array([[1.01, 0.002, 5.0], [-0.003, 0.99, -2.0]], dtype=np.float32)
    want, _ = behind(busy, "busca_ghost_motion_warp", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_motion_warp(
        ctx.h, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), 8, 4, None, 0, W.ctypes.data, st)),
        [true[0], true[2], true[3]], [poison[0], poison[2], poison[3]])
    assert np.isfinite(want[0]).all() and (want[0] != recorded("static", 9, 1)["hist"]).any()


@gpu
def test_stream_order_step(ctx, busy):
    import torch
    from tests.test_streams_gpu import _dev
    true, poison = _stream_state()
    slots, na, _, _, _ = frame_of("static", 9)
    slot = _dev(np.array(slots))
    out = torch.empty(len(slots), 4, dtype=torch.float64, device=slot.device)
    want, _ = behind(busy, "busca_ghost_motion_step", lambda x, o, st: ctx.check(ctx.lib.busca_ghost_motion_step(
        ctx.h, *[t.data_ptr() for t in x[:6]], 8, 4, x[6].data_ptr(), len(slots), na, 3, 0, o[0].data_ptr(), st)),
        true + [slot], poison + [slot.flip(0).contiguous()], lambda: [out.fill_(-7.0)])
    post = recorded("static", 9, 2)
    assert same(want[4], post["pos"]) and same(want[5], post["vel"]) and same(want[7], post["pos"][slots])


@gpu
def test_stream_order_cost(ctx, busy):
    """GhostMotion.cost on torch's current stream: the slot upload, the step and the IoU kernel all behind the prefix."""
    from busca_amd import tracking
    from tests.test_streams_gpu import _dev, _nan
    true, poison = _stream_state()
    slots, na, dets, dist, _ = frame_of("static", 9)
    d, slot = _dev(np.array(dets)), _dev(np.array(slots))
    gm = tracking.GhostMotion(8, 4, ctx=ctx)

    def call(x, o, st):
        gm.hist, gm.frames, gm.count, gm.newest, gm.pos, gm.vel = x[:6]
        return gm.cost(x[7], na, x[6], 3)
    want, _ = behind(busy, "GhostMotion.cost", call, true + [d, slot], poison + [_nan(d), slot.flip(0).contiguous()], form="current")
    assert same(want[8], np.ascontiguousarray(dist.T))
