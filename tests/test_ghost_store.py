"""GHOST's and StrongSORT's appearance state on the device: busca_amd.tracking.GhostGallery (feature rings + the moving-average table),
ghost_round's 'mv_avg' proxy on that table, and NearestNeighborDistanceMetric.partial_fit(ema_alpha=...).

The reference is tests/golden/ghost_store.npz, written by tests/golden/make_golden_ghost_store.py: real Track objects and get_proxy
(adapters/GHOST/src/tracking_utils.py) driven through a scripted sequence of 12 frames - E = 32, budget 4, 8 slots, 6 tracks: one matched in every
frame (its ring wraps twice), one inactive for frames 4-7 and then matched again, one released at frame 6 whose slot a new track takes at frame 8,
one born at frame 5, one inactive from frame 2 on; the track matched in every frame gets the same feature at frames 1 and 2 (a tie in the median).
A frame of the script: releases, then adds (slot, detection row, new flag), then the proxies of the live tracks, active ones first.

`NpStore` below restates the script in plain numpy and reproduces every recorded array bit for bit, so the fixture is checkable without the
reference.  torch's CPU bits, restated: mean = the float32 sum in sample order / k; F.normalize's norm = 8 lanes of fused multiply-adds (lane j takes
elements j, j + 8, ..), the lanes summed in order, sqrt; mv_avg = two float32 products and one float32 sum.

Bars, none of them taken from the device's output:
  * last, median, the mv_avg proxies and tables, ring bookkeeping: exact.
  * mean, meannorm: the rule of tests/test_ghost_round.py for px_mean_* / px_meannorm_*: the recorded distance between the reference's float32
    output and a float64 restatement + one float32 ulp of the value (the device rounds a float64 result once).
  * EMA (parity-unpinned like the rest of NearestNeighborDistanceMetric: deep_sort/track.py imports modules that are not in the reference tree, so
    the checker is a numpy restatement of track.py:244-248): 4 x the largest elementwise distance between that restatement in float32 and the same
    lines in float64 over the scenario; the 4 is for the reduction order of the norm."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ghost_store.npz")
gpu = pytest.mark.gpu
E, BUDGET, CAPACITY, FRAMES, TRACKS = 32, 4, 8, 12, 6
A_ACT, A_INACT = 0.9, 0.5
MODES = [("last", 3), ("mean", 3), ("median", 3), ("meannorm", 3), ("mean", "all"), ("median", "all"), ("meannorm", "all")]
_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
        for v in _CACHE["g"].values():
            v.setflags(write=False)
    return _CACHE["g"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def norm8(v):
    """torch CPU's float32 2-norm of a contiguous vector: 8 lanes of fused multiply-adds, the lanes summed in order."""
    acc = np.zeros(8, dtype=np.float32)
    for i in range(0, len(v), 8):
        d = np.zeros(8, dtype=np.float64)
        d[:len(v[i:i + 8])] = v[i:i + 8]
        acc = (d * d + acc.astype(np.float64)).astype(np.float32)          # the product of two float32 is exact in float64: one rounding, as an FMA
    s = acc[0]
    for j in range(1, 8):
        s = np.float32(s + acc[j])
    return np.sqrt(np.float32(s))


class NpStore:
    """GhostGallery in plain numpy: the ring rule and get_proxy's arithmetic with torch CPU's bits."""

    def __init__(self, capacity, budget, e):
        self.budget = budget
        self.gallery = np.zeros((capacity, budget, e), dtype=np.float32)
        self.count, self.newest = np.zeros(capacity, dtype=np.int32), np.zeros(capacity, dtype=np.int32)
        self.mv_avg, self.mv_seen = np.zeros((capacity, e), dtype=np.float32), np.zeros(capacity, dtype=np.uint8)

    def release(self, slots):
        for s in slots:
            self.count[s] = self.mv_seen[s] = 0

    def add(self, slots, feats, det_index=None, new=None):
        for i, s in enumerate(slots):
            if s < 0:
                continue
            if new is not None and new[i]:
                self.count[s] = self.mv_seen[s] = 0
            row = 0 if self.count[s] == 0 else (self.newest[s] + 1) % self.budget
            self.gallery[s, row] = feats[i if det_index is None else det_index[i]]
            self.newest[s], self.count[s] = row, min(self.count[s] + 1, self.budget)

    def rows(self, s):
        """The stored samples of slot s, oldest first."""
        c, n = int(self.count[s]), int(self.newest[s])
        return self.gallery[s, [(n - (c - 1) + k) % self.budget for k in range(c)]]

    def proxy(self, slots, mode, num):
        out = []
        for s in slots:
            rows = self.rows(s)
            w = rows if num == "all" or len(rows) < num else rows[-num:]
            if mode == "last":
                out.append(rows[-1])
            elif mode == "median":
                out.append(np.sort(w, 0)[(len(w) - 1) // 2])                # torch.median: the lower of two
            else:
                acc = w[0].copy()
                for r in w[1:]:
                    acc = acc + r
                mu = acc / np.float32(len(w))
                out.append(mu / np.maximum(norm8(mu), np.float32(1e-12)) if mode == "meannorm" else mu)
        return np.stack(out)

    def mv(self, slots, a):
        """get_proxy's mv_avg branch for one group: the proxies, and the table updated."""
        out = []
        for s in slots:
            last = self.rows(s)[-1]
            f = self.mv_avg[s] * np.float32(a) + last * np.float32(1 - a) if self.mv_seen[s] else last
            self.mv_avg[s], self.mv_seen[s] = f, 1
            out.append(f)
        return np.stack(out) if out else np.zeros((0, self.gallery.shape[2]), dtype=np.float32)


def frame(g, f):
    adds = g["adds_%d" % f]
    return dict(release=g["release_%d" % f], slots=adds[:, 0], det_index=adds[:, 1], new=adds[:, 2], det=g["det_%d" % f], active=g["active_%d" % f],
                inactive=g["inactive_%d" % f])


def recorded_modes(g, f):
    return [(mode, num) for mode, num in MODES if "px_%d_%s_%s" % (f, mode, num) in g]


def replay_numpy(upto=FRAMES):
    """The script through NpStore -> the store after frame `upto` - 1 (a fresh one per call: callers may go on writing)."""
    g, st = gold(), NpStore(CAPACITY, BUDGET, E)
    for f in range(upto):
        fr = frame(g, f)
        st.release(fr["release"])
        st.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        st.mv(fr["active"], A_ACT)
        st.mv(fr["inactive"], A_INACT)
    return st


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_fixture_contents():
    g = gold()
    assert [int(v) for v in g["params"]] == [E, BUDGET, CAPACITY, FRAMES, TRACKS] and os.path.getsize(GOLD) < 1 << 20
    total = np.zeros(CAPACITY, dtype=np.int64)                                 # samples of the track now in the slot
    owner, owners = {}, set()
    all_frames, wrapped_frames, gap, rebirth = 0, 0, set(), False
    for f in range(FRAMES):
        fr = frame(g, f)
        m = fr["det"].shape[0]
        assert fr["det"].shape == (m, E) and fr["det"].dtype == np.float32 and len(set(fr["det_index"])) == len(fr["det_index"]) and fr["det_index"].max() < m
        assert m > len(fr["slots"])                                            # an unmatched detection: det_index is no identity
        for s in fr["release"]:
            total[s] = 0
            owner.pop(int(s))
        for s, new in zip(fr["slots"], fr["new"]):
            if new:
                rebirth = rebirth or (int(s) not in owner and total[s] == 0 and any(int(s) == o[0] for o in owners))
                total[s] = 0
                owner[int(s)] = f
                owners.add((int(s), f))
            total[s] += 1
        live = sorted(owner)
        assert sorted(list(fr["active"]) + list(fr["inactive"])) == live and set(fr["active"]) == set(fr["slots"])
        gap |= {(int(s), f) for s in fr["inactive"]}
        n = len(live)
        for mode, num in recorded_modes(g, f):
            assert g["px_%d_%s_%s" % (f, mode, num)].shape == (n, E) and g["px_%d_%s_%s" % (f, mode, num)].dtype == np.float32
            if mode in ("mean", "meannorm"):
                assert 0 <= float(g["err_%d_%s_%s" % (f, mode, num)]) < 1e-6
        have = set(recorded_modes(g, f))
        assert {("last", 3), ("mean", 3), ("median", 3)} <= have
        if ("mean", "all") in have:
            assert total[live].max() <= BUDGET and {("median", "all"), ("meannorm", "all")} <= have
            all_frames += 1
        else:
            assert total[live].max() > BUDGET
        if total[live].max() > BUDGET:
            wrapped_frames += 1
        assert (("meannorm", 3) in have) == (total[live].max() < 3)            # its num <= len branch raises in the reference (normalize over dim 1 of a vector)
        assert g["mv_px_%d" % f].shape == (n, E) and g["mv_tab_%d" % f].shape == (CAPACITY, E) and g["mv_seen_%d" % f].dtype == np.uint8
        assert sorted(np.nonzero(g["mv_seen_%d" % f])[0]) == live
    assert all_frames >= 3 and wrapped_frames >= 3 and total.max() == FRAMES >= 3 * BUDGET      # 'all' frames, wrapped frames, a ring that wrapped twice
    assert rebirth and len(owners) == TRACKS
    s1 = [s for s in range(CAPACITY) if {(s, f) for f in (4, 5, 6, 7)} <= gap and (s, 3) not in gap and (s, 8) not in gap]
    assert len(s1) == 1                                                        # the inactive gap of frames 4-7
    assert any(owner_f == 5 for _, owner_f in owners)                          # born at frame 5
    s, f = [int(v) for v in g["tie"]]
    a, b = frame(g, f - 1), frame(g, f)
    assert same(a["det"][a["det_index"][list(a["slots"]).index(s)]], b["det"][b["det_index"][list(b["slots"]).index(s)]])
    px = g["px_%d_median_3" % f][list(b["active"]).index(s)]
    assert same(px, b["det"][b["det_index"][list(b["slots"]).index(s)]])       # two of three samples equal: the median is that sample


def test_numpy_restatement_reproduces_the_fixture():
    g, st = gold(), NpStore(CAPACITY, BUDGET, E)
    checked = 0
    for f in range(FRAMES):
        fr = frame(g, f)
        st.release(fr["release"])
        st.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        slots = list(fr["active"]) + list(fr["inactive"])
        for mode, num in recorded_modes(g, f):
            assert same(st.proxy(slots, mode, num), g["px_%d_%s_%s" % (f, mode, num)]), (f, mode, num)
            checked += 1
        px = np.concatenate([st.mv(fr["active"], A_ACT), st.mv(fr["inactive"], A_INACT)])
        assert same(px, g["mv_px_%d" % f]) and same(st.mv_seen, g["mv_seen_%d" % f]), f
        assert same(st.mv_avg[slots], g["mv_tab_%d" % f][slots]), f
    assert checked >= 3 * FRAMES + 3 * 3
    assert st.count.max() == BUDGET and (st.newest != st.count - 1).any()      # wrapped rings


def test_reachable_from_the_facade_and_the_alias_package():
    import inspect
    from busca_amd import appearance, ghost_gallery, tracking
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        import busca.tracking as bt
    finally:
        sys.path.pop(0)
    assert tracking.GhostGallery is ghost_gallery.GhostGallery is bt.GhostGallery
    assert tracking.NearestNeighborDistanceMetric is appearance.NearestNeighborDistanceMetric is bt.NearestNeighborDistanceMetric
    sig = inspect.signature(bt.NearestNeighborDistanceMetric.partial_fit)
    assert list(sig.parameters) == ["self", "features", "targets", "active_targets", "ema_alpha"] and sig.parameters["ema_alpha"].default is None
    for name in ("add", "release", "state"):
        assert callable(getattr(bt.GhostGallery, name)), name
    assert list(inspect.signature(tracking.GhostGallery.add).parameters) == ["self", "slots", "feats", "det_index", "new"]
    assert list(inspect.signature(tracking.GhostGallery.__init__).parameters) == ["self", "capacity", "budget", "E", "ctx"]


def test_the_c_interface_is_what_it_was():
    from busca_amd import _lib
    assert {h: len(t) for h, t in _lib.HEADERS.items()} == {"busca_hip.h": 37, "busca_assign.h": 1, "busca_appearance.h": 1, "busca_ghost.h": 4,
                                                            "busca_ghost_motion.h": 3, "busca_ecc.h": 3, "busca_reid_bn.h": 6}
    assert sorted(_lib.GHOST_SIGNATURES) == ["busca_ghost_combine", "busca_ghost_distance", "busca_ghost_proxies", "busca_ghost_thresholds"]
    assert (_lib.GHOST_PROXY_LAST, _lib.GHOST_PROXY_FIRST, _lib.GHOST_PROXY_MEAN, _lib.GHOST_PROXY_MEANNORM, _lib.GHOST_PROXY_MEDIAN) == (0, 1, 2, 3, 4)
    assert not [n for n in dir(_lib) if "MV_AVG" in n.upper() or "EMA" in n.upper()]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from busca_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))                  # a copy: the fixture's arrays are read-only


def check_proxies(store, g, f, slots, ctx, what):
    from busca_amd import tracking
    for mode, num in recorded_modes(g, f):
        ref = g["px_%d_%s_%s" % (f, mode, num)]
        got = tracking.ghost_proxies(store.gallery, mode, num, slot=slots, count=store.count, newest=store.newest, ctx=ctx).cpu().numpy()
        if mode in ("last", "median"):
            assert same(got, ref), (what, f, mode, num)
        else:
            bar = float(g["err_%d_%s_%s" % (f, mode, num)]) + np.spacing(np.abs(ref)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - ref)
            print("%s frame %d %s %s: max |d| %.3g, bar >= %.3g" % (what, f, mode, num, err.max(), bar.min()))
            assert got.shape == ref.shape and (err <= bar).all(), (what, f, mode, num)


@gpu
@pytest.mark.parametrize("device", [False, True], ids=["host_operands", "device_operands"])
def test_replay_against_the_reference(ctx, device):
    import torch
    from busca_amd import tracking
    g, ref = gold(), NpStore(CAPACITY, BUDGET, E)
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)
    assert tuple(store.gallery.shape) == (CAPACITY, BUDGET, E) and store.gallery.dtype == torch.float32 and store.gallery.is_contiguous()
    assert store.count.dtype == store.newest.dtype == torch.int32 and store.mv_seen.dtype == torch.uint8 and tuple(store.mv_avg.shape) == (CAPACITY, E)
    for f in range(FRAMES):
        fr = frame(g, f)
        ref.release(fr["release"])
        ref.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        slots = np.concatenate([fr["active"], fr["inactive"]]).astype(np.int32)
        if device:
            if len(fr["release"]):
                store.release(_dev(fr["release"].astype(np.int32)))
            store.add(_dev(fr["slots"].astype(np.int32)), _dev(fr["det"]), _dev(fr["det_index"].astype(np.int32)), _dev(fr["new"].astype(np.uint8)))
            slots = _dev(slots)
        else:
            store.release(fr["release"])
            store.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        assert same(store.count.cpu().numpy(), ref.count) and same(store.newest.cpu().numpy()[ref.count > 0], ref.newest[ref.count > 0]), f
        live = ref.count > 0
        host = store.gallery.cpu().numpy()
        for s in np.nonzero(live)[0]:
            assert same(host[s, :ref.count[s]], ref.gallery[s, :ref.count[s]]), (f, s)      # stored as given
        check_proxies(store, g, f, slots, ctx, "replay")


@gpu
def test_mv_avg_through_ghost_round(ctx):
    import torch
    from busca_amd import tracking
    g = gold()
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)
    cfg = dict(avg_act={"do": True, "proxy": "mv_avg", "num": A_ACT}, avg_inact={"do": True, "proxy": "mv_avg", "num": A_INACT})
    before = store.mv_avg.cpu().numpy()
    for f in range(FRAMES):
        fr = frame(g, f)
        store.release(fr["release"])
        store.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        slots = list(fr["active"]) + list(fr["inactive"])
        state = store.state(fr["active"], fr["inactive"])
        assert state["num_active"] == len(fr["active"]) and state["slot"].dtype == torch.int32 and same(state["slot"].cpu().numpy(), np.asarray(slots, dtype=np.int32))
        assert state["mv_avg"] is store.mv_avg and state["gallery"] is store.gallery and state["motion_state"] is None
        if f == 3:                                                             # refused before either group has written its table
            bare = {k: v for k, v in state.items() if k not in ("mv_avg", "mv_seen")}
            with pytest.raises(NotImplementedError, match=r"GhostGallery\.state"):
                tracking.ghost_round(bare, fr["det"], cfg=cfg, ctx=ctx)
            with pytest.raises(ValueError, match="TypeError"):
                tracking.ghost_round(state, fr["det"], cfg=dict(cfg, avg_inact=dict(cfg["avg_inact"], num="all")), ctx=ctx)
            with pytest.raises(NotImplementedError, match="mv_avg"):
                tracking.ghost_proxies(store.gallery, mode="mv_avg", ctx=ctx)
            assert same(store.mv_avg.cpu().numpy(), before)
        dist, row, col = tracking.ghost_round(state, fr["det"], cfg=cfg, ctx=ctx)
        table, seen = store.mv_avg.cpu().numpy(), store.mv_seen.cpu().numpy()
        assert same(table[slots], g["mv_tab_%d" % f][slots]) and same(seen, g["mv_seen_%d" % f]), f
        rest = [s for s in range(CAPACITY) if s not in slots]
        assert same(table[rest], before[rest]), f                              # unqueried slots keep their rows
        want = tracking.ghost_distance(g["mv_px_%d" % f], fr["det"], "min", ctx=ctx).cpu().numpy()
        assert same(dist.cpu().numpy().T, want), f
        assert len(row) == len(col) == min(len(slots), fr["det"].shape[0])
        before = table
    # a negative slot and a track without samples: NaN rows, table untouched
    store.release([int(fr["active"][0])])
    held = store.mv_avg.cpu().numpy()
    state = store.state([int(fr["active"][0]), -1, int(fr["active"][1])])
    dist, _, _ = tracking.ghost_round(state, fr["det"], cfg=cfg, ctx=ctx)
    d = dist.cpu().numpy().T
    assert np.isnan(d[:2]).all() and np.isfinite(d[2]).all()
    now = store.mv_avg.cpu().numpy()
    keep = [s for s in range(CAPACITY) if s != int(fr["active"][1])]
    assert same(now[keep], held[keep]) and not same(now, held) and int(store.mv_seen.cpu().numpy()[int(fr["active"][0])]) == 0


@gpu
@pytest.mark.parametrize("inact", [{"do": True, "proxy": "mv_avg", "num": A_ACT}, {"do": True, "proxy": "mean", "num": 3}, {"do": False}],
                         ids=["one_weight", "mean_beside", "last_beside"])
def test_mv_avg_in_the_other_groupings(ctx, inact):
    """The fixture's round blends both groups with their own weights in one pass.  Here the other shapes of a round - both groups one weight (one group
    of rows), and 'mv_avg' for the active tracks beside another proxy for the inactive ones - against NpStore, which reproduces the fixture's bits."""
    from busca_amd import tracking
    g, ref = gold(), NpStore(CAPACITY, BUDGET, E)
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)
    cfg = dict(avg_act={"do": True, "proxy": "mv_avg", "num": A_ACT}, avg_inact=inact)
    for f in range(FRAMES):
        fr = frame(g, f)
        for st in (store, ref):
            st.release(fr["release"])
            st.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        px = [ref.mv(fr["active"], A_ACT)]
        if len(fr["inactive"]):
            px.append(ref.mv(fr["inactive"], A_ACT) if inact.get("proxy") == "mv_avg" else ref.proxy(fr["inactive"], "last", 3))
        dist, _, _ = tracking.ghost_round(store.state(fr["active"], fr["inactive"]), fr["det"], cfg=cfg, ctx=ctx)
        assert same(store.mv_avg.cpu().numpy()[ref.mv_seen > 0], ref.mv_avg[ref.mv_seen > 0]) and same(store.mv_seen.cpu().numpy(), ref.mv_seen), f
        if inact.get("proxy") != "mean":
            assert same(dist.cpu().numpy().T, tracking.ghost_distance(np.concatenate(px), fr["det"], "min", ctx=ctx).cpu().numpy()), f
        else:
            na = len(fr["active"])
            assert same(dist.cpu().numpy().T[:na], tracking.ghost_distance(px[0], fr["det"], "min", ctx=ctx).cpu().numpy()), f


@gpu
def test_add_and_state_make_no_synchronising_call(ctx):
    import torch
    from busca_amd import tracking
    g = gold()
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)
    ops = []
    for f in range(3):
        fr = frame(g, f)
        ops.append((_dev(fr["slots"].astype(np.int32)), _dev(fr["det"]), _dev(fr["det_index"].astype(np.int32)), _dev(fr["new"].astype(np.uint8)),
                    _dev(fr["active"].astype(np.int32)), _dev(fr["inactive"].astype(np.int32))))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for slots, det, det_index, new, active, inactive in ops:
            store.add(slots, det, det_index, new)
            state = store.state(active, inactive)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert state["num_active"] == len(frame(g, 2)["active"]) and state["slot"].is_cuda
    check_proxies(store, g, 2, state["slot"], ctx, "no-sync")


@gpu
def test_stream_order_add_then_proxies(ctx, busy):
    """Frame 8 of the script (a wrap, a reactivation, a new track in a reused slot) on a busy side stream: the state of frame 7 is copied in behind the
    prefix, poison is what the tensors hold until then."""
    import torch
    from busca_amd import tracking
    from tests.test_streams_gpu import _nan, behind
    g, ref = gold(), replay_numpy(8)
    fr = frame(g, 8)
    pad = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:], dtype=a.dtype)])      # noqa: E731  (the spare slot of the store's own tensors)
    true = [_dev(pad(ref.gallery)), _dev(pad(ref.count)), _dev(pad(ref.newest)), _dev(pad(ref.mv_seen)), _dev(fr["det"]), _dev(fr["slots"].astype(np.int32)),
            _dev(fr["det_index"].astype(np.int32)), _dev(fr["new"].astype(np.uint8))]
    true.append(_dev(np.concatenate([fr["active"], fr["inactive"]]).astype(np.int32)))
    poison = [_nan(true[0]), torch.zeros_like(true[1]), torch.full_like(true[2], 3), torch.ones_like(true[3]), _nan(true[4]), true[5].flip(0).contiguous(),
              torch.zeros_like(true[6]), 1 - true[7], true[8].flip(0).contiguous()]
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)

    def call(x, o, st):
        store._gallery, store._count, store._newest, store._mv_seen = x[:4]
        store.gallery, store.count, store.newest, store.mv_seen = (t[:CAPACITY] for t in x[:4])
        store.add(x[5], x[4], x[6], x[7])
        return [tracking.ghost_proxies(store.gallery, mode, num, slot=x[8], count=store.count, newest=store.newest, ctx=ctx)
                for mode, num in (("last", 3), ("median", 3), ("mean", 3))]
    want, _ = behind(busy, "GhostGallery.add + ghost_proxies", call, true, poison, form="current")
    assert same(want[-3], g["px_8_last_3"]) and same(want[-2], g["px_8_median_3"])
    assert (np.abs(want[-1].astype(np.float64) - g["px_8_mean_3"]) <= float(g["err_8_mean_3"]) + np.spacing(np.abs(g["px_8_mean_3"])).astype(np.float64)).all()


@gpu
def test_lifecycle_and_argument_errors(ctx):
    from busca_amd import synth, tracking
    feats = synth.normal(41, "life", (5, E))
    store = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx)
    for t in range(3):
        store.add([2, 6], feats[2 * t % 4:2 * t % 4 + 2])
    store.mv_seen[2] = 1
    store.mv_seen[6] = 1
    assert store.count.cpu().numpy().tolist() == [0, 0, 3, 0, 0, 0, 3, 0]
    store.release([2])
    store.add([2, -1, 4], feats, det_index=[4, 0, 1], new=[True, True, False])     # the negative slot is skipped
    count, seen, host = store.count.cpu().numpy(), store.mv_seen.cpu().numpy(), store.gallery.cpu().numpy()
    assert count.tolist() == [0, 0, 1, 0, 1, 0, 3, 0] and seen.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert same(host[2, 0], feats[4]) and same(host[4, 0], feats[1]) and int(store.newest.cpu().numpy()[2]) == 0
    store.add([6], feats[3:4], new=[True])                                        # `new` on a live slot discards its history
    assert int(store.count.cpu().numpy()[6]) == 1 and int(store.mv_seen.cpu().numpy()[6]) == 0 and same(store.gallery.cpu().numpy()[6, 0], feats[3])
    got = tracking.ghost_proxies(store.gallery, "mean", "all", slot=[6, 0], count=store.count, newest=store.newest, ctx=ctx).cpu().numpy()
    assert same(got[0], feats[3]) and np.isnan(got[1]).all()
    held = [t.cpu().numpy() for t in (store.gallery, store.count, store.newest, store.mv_seen)]
    for call in (lambda: store.add([1, 1], feats), lambda: store.add([CAPACITY], feats), lambda: store.release([3, 3]), lambda: store.release([CAPACITY]),
                 lambda: store.state([1], [1]), lambda: store.state([CAPACITY]), lambda: store.add([0, 1], np.zeros((2, E + 1), np.float32)),
                 lambda: store.add(list(range(6)), feats), lambda: store.add([0, 1], feats, det_index=[0]), lambda: store.add([0, 1], feats, new=[True]),
                 lambda: tracking.GhostGallery(4, 0, E, ctx=ctx), lambda: tracking.GhostGallery(-1, 4, E, ctx=ctx)):
        with pytest.raises(ValueError):
            call()
    for t, h in zip((store.gallery, store.count, store.newest, store.mv_seen), held):
        assert same(t.cpu().numpy(), h)                                           # refused calls launched nothing
    empty = tracking.GhostGallery(0, 1, E, ctx=ctx)
    empty.add([], feats[:0])
    assert tuple(empty.gallery.shape) == (0, 1, E)


def ema_scenario():
    """5 targets x 6 rounds at E = 512 -> [(features [k,E], targets, active_targets)]: target 3 first seen in round 3, target 1 fed twice in round 2,
    target 4 dropped through active_targets in round 3 and fed again in round 4."""
    from busca_amd import synth
    rounds = []
    for r in range(6):
        targets = [t for t in range(5) if not (t == 3 and r < 3) and not (t == 4 and r == 3)]
        if r == 2:
            targets.insert(3, 1)
        active = [t for t in range(5) if not (t == 4 and r == 3)]
        rounds.append((synth.normal(900 + r, "ema", (len(targets), 512)) + np.float32(0.25), targets, active))
    return rounds


def ema_numpy(rounds, alpha, dtype):
    """deep_sort/track.py:244-248 and :85-87 per target, in `dtype`."""
    gal = {}
    for feats, targets, active in rounds:
        for f, t in zip(feats.astype(dtype), targets):
            feature = f / np.linalg.norm(f)
            if t in gal:
                smooth = dtype(alpha) * gal[t] + dtype(1 - alpha) * feature
                smooth /= np.linalg.norm(smooth)
                gal[t] = smooth
            else:
                gal[t] = feature
        gal = {t: v for t, v in gal.items() if t in active}
        yield dict(gal)


@gpu
def test_strongsort_ema_on_the_device(ctx):
    from busca_amd import tracking
    alpha, rounds = 0.9, ema_scenario()
    want32, want64 = list(ema_numpy(rounds, alpha, np.float32)), list(ema_numpy(rounds, alpha, np.float64))
    assert all(v.dtype == np.float32 for w in want32 for v in w.values())
    bar = 4 * max(np.abs(w32[t].astype(np.float64) - w64[t]).max() for w32, w64 in zip(want32, want64) for t in w32)
    assert 0 < bar < 1e-6
    metric = tracking.NearestNeighborDistanceMetric("cosine", 0.4, budget=3, ctx=ctx)
    plain = tracking.NearestNeighborDistanceMetric("cosine", 0.4, budget=3, ctx=ctx)
    worst = 0.0
    for r, (feats, targets, active) in enumerate(rounds):
        metric.partial_fit(_dev(feats) if r % 2 else feats, targets, active, ema_alpha=alpha)      # the device tensor appearance_round was given, or host rows
        got = metric.samples
        assert sorted(got) == sorted(want32[r])
        for t, rows in got.items():
            assert rows.shape == (1, 512) and rows.dtype == np.float32                # one row per target, whatever the budget
            worst = max(worst, float(np.abs(rows[0].astype(np.float64) - want32[r][t]).max()))
        ids = sorted(got) + [77]
        dist = metric.distance(feats, ids)
        rows = np.stack([got[t][0] for t in ids[:-1]])
        assert same(dist[:-1], tracking.appearance_cost(rows, feats, "min", ctx=ctx).cpu().numpy()) and np.isposinf(dist[-1]).all()
        plain.partial_fit(feats, targets, active, ema_alpha=None)
    print("EMA: max |device - float32 restatement| %.3g, bar %.3g" % (worst, bar))
    assert worst <= bar
    twice = [k for k, t in enumerate(rounds[2][1]) if t == 1]
    swapped = rounds[2][0].copy()
    swapped[twice] = swapped[twice[::-1]]
    other = list(ema_numpy(rounds[:2] + [(swapped, rounds[2][1], rounds[2][2])], alpha, np.float32))[2][1]
    assert len(twice) == 2 and np.abs(other - want32[2][1]).max() > 100 * bar          # the scenario tells call order from its reverse
    # ema_alpha=None is the code path as it was: the last `budget` normalised samples per target, oldest first
    hist = {}
    for feats, targets, active in rounds:
        for f, t in zip(feats.astype(np.float64), targets):
            hist.setdefault(t, []).append((f / np.sqrt((f * f).sum())).astype(np.float32))
        hist = {t: v[-3:] for t, v in hist.items() if t in active}
    got = plain.samples
    assert sorted(got) == sorted(hist) and all(same(got[t], np.stack(hist[t])) for t in hist)
