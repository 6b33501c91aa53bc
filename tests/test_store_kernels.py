"""The appearance state's own kernels and C interface: libbusca_store.so (include/busca_store.h), its binding busca_amd._store_lib, and the Python
surface routed through it (GhostGallery.add / release, ghost_round's 'mv_avg' blend, NearestNeighborDistanceMetric.partial_fit(ema_alpha=)).

References, none of them the device's output:
  * tests/golden/ghost_store.npz and `NpStore` of tests/test_ghost_store.py, which reproduces that fixture bit for bit: ring bookkeeping, stored rows,
    the mv_avg table, flags and returned rows are compared exactly.  The blend is two float32 products and one float32 sum; a contracted
    multiply-add differs from that in the last bit of some of the 12 x 512-odd values checked, so it does not survive.
  * `ema_numpy` of the same module (deep_sort/track.py:244-248 restated) in float32, at the bar that module derives: 4 x the largest elementwise
    distance between the restatement in float32 and in float64, computed here for the shapes used here (at E = 1 both are exactly +-1 and the bar
    is 0: x / |x| is exact with a correctly rounded square root and quotient).
Every state array of the edge-shape test has S + 1 rows and the kernels are told S: row S holds a sentinel that must survive every call."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests.test_ghost_store import A_ACT, A_INACT, BUDGET, CAPACITY, E, FRAMES, NpStore, ema_numpy, ema_scenario, frame, gold, replay_numpy, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
SENTINEL = 7.5


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_store.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_store_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _store_lib.STORE_API.items()}
    assert sorted(declared) == ["busca_store_ema_fit", "busca_store_last_error", "busca_store_mv_avg", "busca_store_release", "busca_store_ring_add",
                                "busca_store_version"]

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert {n for n in exported(_store_lib.STORE_LIB_PATH) if not n.startswith("_")} == set(_store_lib.STORE_API)
    assert os.path.basename(hip_lib) == "libbusca_hip.so"
    for other in (hip_lib, _track_lib.TRACK_LIB_PATH):
        assert not [n for n in exported(other) if n.startswith("busca_store")], other
    ours = exported(_store_lib.STORE_LIB_PATH)
    assert not [n for n in ours if n in {k for t in _lib.HEADERS.values() for k in t} or n in _track_lib.TRACK_API]
    assert "busca_store.h" not in _lib.HEADERS and "_store_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _store_lib.load()
    assert lib.busca_store_version() == 1000 and _store_lib.ABI_MAJOR == 1 and lib.busca_store_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _store_lib
    lib = _store_lib.load()
    P, ODD, S, k, m = 0x10000, 0x10002, 8, 3, 5           # an aligned address, one that is not 4-byte aligned

    def calls(gallery=P, count=P, newest=P, avg=P, seen=P, S=S, rows=4, E=32, slot=P, k=k, feats=P, m=m, det=P, new=P, na=2, a=0.9, b=0.5, out=P,
              gslot=P, gold_row=P, gstart=P, src=P, nsrc=4, alpha=0.9, dev=0):
        return {
            "busca_store_ring_add": lambda: lib.busca_store_ring_add(gallery, count, newest, seen, S, rows, E, slot, k, feats, m, det, new, dev, None),
            "busca_store_release": lambda: lib.busca_store_release(count, seen, S, slot, k, dev, None),
            "busca_store_mv_avg": lambda: lib.busca_store_mv_avg(gallery, count, newest, avg, seen, S, rows, E, slot, k, min(na, max(k, 0)), a, b, out, dev, None),
            "busca_store_ema_fit": lambda: lib.busca_store_ema_fit(gallery, S, rows, E, feats, m, gslot, gold_row, gstart, src, k, nsrc, alpha, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_store_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    every = list(calls())
    nulls = dict(gallery=None, count=None, newest=None, avg=None, seen=None, slot=None, feats=None, det=None, new=None, out=None, gslot=None,
                 gold_row=None, gstart=None, src=None)
    for name in every:
        assert calls(k=0)[name]() == 0, name                                       # the no-op: k = 0, n = 0, g = 0
        assert calls(k=0, **nulls)[name]() == 0, name
        refused(name, "negative size", k=-1)
        refused(name, "negative size", S=-1)
        refused(name, "negative device", dev=-1)
    for name in ("busca_store_ring_add", "busca_store_mv_avg", "busca_store_ema_fit"):
        refused(name, "null pointer", gallery=None)
        refused(name, "misaligned", gallery=ODD)
        refused(name, "at least 1 row", rows=0)
        refused(name, "at least 1 row", E=0)
    for name in ("busca_store_ring_add", "busca_store_release", "busca_store_mv_avg"):
        refused(name, "null pointer", slot=None)
        refused(name, "null pointer", seen=None)
        refused(name, "misaligned", slot=ODD)
    for name in ("busca_store_ring_add", "busca_store_release"):
        refused(name, "null pointer", count=None)
        refused(name, "misaligned", count=ODD)
    name = "busca_store_ring_add"
    refused(name, "null pointer", newest=None)
    refused(name, "null pointer (feats)", feats=None)
    refused(name, "negative size", m=-1)
    refused(name, "misaligned", newest=ODD)
    refused(name, "misaligned", feats=ODD)
    refused(name, "misaligned", det=ODD)
    refused(name, "no det_index", det=None, k=6)
    assert calls(det=None, k=0)[name]() == 0
    name = "busca_store_mv_avg"
    assert calls(count=None, newest=None, k=0)[name]() == 0
    refused(name, "null pointer", avg=None)
    refused(name, "null pointer", out=None)
    refused(name, "misaligned", count=ODD)
    refused(name, "misaligned", newest=ODD)
    refused(name, "misaligned", avg=ODD)
    refused(name, "misaligned", out=ODD)
    refused(name, "is NaN", a=float("nan"))
    refused(name, "is NaN", b=float("nan"))
    rc = lib.busca_store_mv_avg(P, P, P, P, P, S, 4, 32, P, k, k + 1, 0.9, 0.5, P, 0, None)
    assert rc == -1 and "num_active 4 outside 0 .. 3" in lib.busca_store_last_error().decode()
    rc = lib.busca_store_mv_avg(P, P, P, P, P, S, 4, 32, P, k, -1, 0.9, 0.5, P, 0, None)
    assert rc == -1 and "num_active -1 outside" in lib.busca_store_last_error().decode()
    name = "busca_store_ema_fit"
    refused(name, "negative size", m=-1)
    refused(name, "negative size", nsrc=-1)
    refused(name, "alpha is NaN", alpha=float("nan"))
    for arg in ("gslot", "gold_row", "gstart"):
        refused(name, "null pointer", **{arg: None})
        refused(name, "misaligned", **{arg: ODD})
    refused(name, "null pointer (feats, src)", feats=None)
    refused(name, "null pointer (feats, src)", src=None)
    refused(name, "misaligned", feats=ODD)
    refused(name, "misaligned", src=ODD)
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_store_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_store_last_error() != b""


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


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32).reshape(-1))


def _p(t):
    return None if t is None else t.data_ptr()


class Raw:
    """The state arrays of one store on the device with `pad` rows behind the last slot, and the four calls made directly."""

    def __init__(self, S, budget, e, pad=0):
        import torch
        from busca_amd import _store_lib
        self.lib, self.check = _store_lib.load(), _store_lib.check
        self.S, self.budget, self.e = S, budget, e
        dev = torch.device("cuda", 0)
        self.gallery = torch.zeros(S + pad, budget, e, dtype=torch.float32, device=dev)
        self.count, self.newest = (torch.zeros(S + pad, dtype=torch.int32, device=dev) for _ in range(2))
        self.mv_avg = torch.zeros(S + pad, e, dtype=torch.float32, device=dev)
        self.mv_seen = torch.zeros(S + pad, dtype=torch.uint8, device=dev)
        if pad:
            self.gallery[S:], self.mv_avg[S:] = SENTINEL, SENTINEL
            self.count[S:], self.newest[S:], self.mv_seen[S:] = 77, 77, 77

    def spare_is_untouched(self):
        S = self.S
        return (bool((self.gallery[S:] == SENTINEL).all()) and bool((self.mv_avg[S:] == SENTINEL).all()) and bool((self.count[S:] == 77).all())
                and bool((self.newest[S:] == 77).all()) and bool((self.mv_seen[S:] == 77).all()))

    def release(self, slots, stream=None):
        s = _i32(slots)
        self.check(self.lib.busca_store_release(self.count.data_ptr(), self.mv_seen.data_ptr(), self.S, s.data_ptr(), s.numel(), 0, stream))

    def add(self, slots, feats, det_index=None, new=None, stream=None):
        s, f = _i32(slots), _dev(feats)
        d = None if det_index is None else _i32(det_index)
        w = None if new is None else _dev(np.asarray(new).astype(np.uint8))
        self.check(self.lib.busca_store_ring_add(self.gallery.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(), self.mv_seen.data_ptr(), self.S,
                                                 self.budget, self.e, s.data_ptr(), s.numel(), _p(f), f.shape[0], _p(d), _p(w), 0, stream))

    def mv(self, slots, num_active, a_act, a_inact, count=True, newest=True, stream=None):
        import torch
        s = _i32(slots)
        out = torch.full((s.numel(), self.e), -3.0, dtype=torch.float32, device=s.device)
        self.check(self.lib.busca_store_mv_avg(self.gallery.data_ptr(), self.count.data_ptr() if count else None, self.newest.data_ptr() if newest else None,
                                               self.mv_avg.data_ptr(), self.mv_seen.data_ptr(), self.S, self.budget, self.e, s.data_ptr(), s.numel(),
                                               num_active, a_act, a_inact, out.data_ptr(), 0, stream))
        return out.cpu().numpy()

    def host(self):
        S = self.S
        return {k: getattr(self, k)[:S].cpu().numpy() for k in ("gallery", "count", "newest", "mv_avg", "mv_seen")}


@gpu
def test_raw_abi_replays_the_fixture():
    g, ref, raw = gold(), NpStore(CAPACITY, BUDGET, E), Raw(CAPACITY, BUDGET, E)
    for f in range(FRAMES):
        fr = frame(g, f)
        ref.release(fr["release"])
        ref.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        raw.release(fr["release"])
        raw.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        h = raw.host()
        live = ref.count > 0
        assert same(h["count"], ref.count) and same(h["newest"][live], ref.newest[live]), f
        for s in np.nonzero(live)[0]:
            assert same(h["gallery"][s, :ref.count[s]], ref.gallery[s, :ref.count[s]]), (f, s)
        slots = np.concatenate([fr["active"], fr["inactive"]])
        px = raw.mv(slots, len(fr["active"]), A_ACT, A_INACT)
        h = raw.host()
        assert same(px, g["mv_px_%d" % f]), f
        assert same(h["mv_avg"][slots], g["mv_tab_%d" % f][slots]) and same(h["mv_seen"], g["mv_seen_%d" % f]), f


def _np_add(ref, S, slots, feats, det_index, new):
    """NpStore.add with the skipping rule of the C interface: a slot outside 0 .. S-1 or a feature row outside 0 .. m-1 drops the pair."""
    keep = [i for i, s in enumerate(slots) if 0 <= s < S and 0 <= (i if det_index is None else det_index[i]) < len(feats)]
    ref.add([slots[i] for i in keep], feats, [(i if det_index is None else det_index[i]) for i in keep], None if new is None else [new[i] for i in keep])


def _np_mv(ref, S, slots, num_active, a_act, a_inact, count=True, newest=True):
    """busca_store_mv_avg on an NpStore: its header's rules for count NULL / newest NULL, NpStore.mv's arithmetic."""
    out = np.full((len(slots), ref.gallery.shape[2]), np.nan, dtype=np.float32)
    for i, s in enumerate(slots):
        cnt = 0 if not 0 <= s < S else int(ref.count[s]) if count else ref.budget
        if cnt == 0:
            continue
        nw = int(ref.newest[s]) if newest else cnt - 1
        last, a = ref.gallery[s, nw], (a_act if i < num_active else a_inact)
        f = ref.mv_avg[s] * np.float32(a) + last * np.float32(1 - a) if ref.mv_seen[s] else last
        ref.mv_avg[s], ref.mv_seen[s] = f, 1
        out[i] = f
    return out


@gpu
@pytest.mark.parametrize("k", [1, CAPACITY])
@pytest.mark.parametrize("budget", [1, 3])
@pytest.mark.parametrize("e", [1, 63, 64, 65, 257])
def test_edge_shapes_against_numpy(e, budget, k):
    from busca_amd import synth
    S, m = CAPACITY, CAPACITY + 2
    ref, raw = NpStore(S, budget, e), Raw(S, budget, e, pad=1)

    def agree(what):
        h = raw.host()
        live = ref.count > 0
        assert raw.spare_is_untouched(), what
        assert same(h["count"], ref.count) and same(h["newest"][live], ref.newest[live]) and same(h["mv_seen"], ref.mv_seen), what
        assert same(h["gallery"][live], ref.gallery[live]) and same(h["mv_avg"][ref.mv_seen > 0], ref.mv_avg[ref.mv_seen > 0]), what

    for step in range(budget + 2):                          # every ring wraps at least once
        feats = synth.normal(300 + step, "edge", (m, e))
        if k == 1:                                          # one pair per call: slot 0 again (its ring wraps), then each kind of skipped pair
            lists = [([0], [m - 1 - step], [0]), ([-1], [0], [1]), ([S], [1], [1]), ([1 + step % 2], [m], [1])]
        else:                                               # CAPACITY pairs in one call, three of them skipped
            order = [int(s) for s in np.roll(np.arange(S), step)]
            slots = order[:S - 3] + [-1, S, order[S - 3]]
            det = [int(j) for j in (np.arange(S) * 3 + step) % m]
            det[S - 1] = m
            new = [int(step == 2 and i == 2) for i in range(S)]         # `is_new` on slot 0, live since step 0
            lists = [(slots, det, new)]
        for slots, det, new in lists:
            _np_add(ref, S, slots, feats, det, new)
            raw.add(slots, feats, det, new)
            agree(("add", step, slots))
        if step == 0 and k == 1:                            # without det_index and without is_new: pair i takes feature row i
            _np_add(ref, S, [3, -1], feats, None, None)
            raw.add([3, -1], feats)
            agree(("add, identity", step))
        # the blend: seen and unseen slots, an empty one (slot S-1 is never added to when k == 1; released below otherwise), skipped ones
        if k != 1 and step == 1:
            ref.release([order[0]])
            raw.release([order[0], -1, S])
            agree(("release", step))
        rows = [0, -1, S - 1, 1, S, 3, 2]
        for na, cnt, nw in ((0, True, True), (len(rows), True, True), (3, True, False), (3, False, True), (2, False, False)):
            want = _np_mv(ref, S, rows, na, A_ACT, A_INACT, cnt, nw)
            got = raw.mv(rows, na, A_ACT, A_INACT, cnt, nw)
            assert same(got, want), ("mv_avg", step, na, cnt, nw)
            agree(("mv_avg", step, na, cnt, nw))
    assert ref.count.max() == budget


def _ema_rounds(e):
    """ema_scenario() cut to its first `e` columns, with target 2 fed three times in round 4 (rows 2, then the two appended ones)."""
    from busca_amd import synth
    rounds = [(f[:, :e].copy(), list(t), list(a)) for f, t, a in ema_scenario()]
    f, t, a = rounds[4]
    extra = (synth.normal(950, "ema3", (2, 512)) + np.float32(0.25))[:, :e]
    rounds[4] = (np.concatenate([f, extra]), t + [2, 2], a)
    return rounds


@gpu
@pytest.mark.parametrize("e", [512, 1, 65])
def test_ema_fit_against_numpy(ctx, e):
    from busca_amd import tracking
    alpha, rounds = 0.9, _ema_rounds(e)
    want32, want64 = list(ema_numpy(rounds, alpha, np.float32)), list(ema_numpy(rounds, alpha, np.float64))
    bar = 4 * max(np.abs(w32[t].astype(np.float64) - w64[t]).max() for w32, w64 in zip(want32, want64) for t in w32)
    assert 0 <= bar < 1e-6 and (bar > 0 or e == 1)
    runs = []
    for _ in range(2):
        metric = tracking.NearestNeighborDistanceMetric("cosine", 0.4, budget=3, ctx=ctx)
        worst, got = 0.0, []
        for r, (feats, targets, active) in enumerate(rounds):
            metric.partial_fit(_dev(feats) if r % 2 else feats, targets, active, ema_alpha=alpha)
            got.append(metric.samples)
            assert sorted(got[-1]) == sorted(want32[r])
            for t, rows in got[-1].items():
                assert rows.shape == (1, e) and rows.dtype == np.float32
                worst = max(worst, float(np.abs(rows[0].astype(np.float64) - want32[r][t]).max()))
        print("EMA E = %d: max |device - float32 restatement| %.3g, bar %.3g" % (e, worst, bar))
        assert worst <= bar
        runs.append(got)
    for ra, rb in zip(*runs):                               # two runs, the same bits
        assert sorted(ra) == sorted(rb) and all(same(ra[t], rb[t]) for t in ra)
    if e > 1:                                               # the three feedings of target 2 in round 4 are told from their reverse
        thrice = [i for i, t in enumerate(rounds[4][1]) if t == 2]
        swapped = rounds[4][0].copy()
        swapped[thrice] = swapped[thrice[::-1]]
        other = list(ema_numpy(rounds[:4] + [(swapped, rounds[4][1], rounds[4][2])], alpha, np.float32))[4][2]
        assert len(thrice) == 3 and np.abs(other - want32[4][2]).max() > 100 * bar


@gpu
def test_ema_fit_groups_zero_rows_and_skips():
    """The raw call: a group's bits do not depend on the other groups of the call; a zero feature row gives NaN; skipped groups and rows touch nothing."""
    import torch
    from busca_amd import _store_lib, synth
    lib = _store_lib.load()
    S, e, m = 6, 65, 7
    feats = synth.normal(77, "ema_raw", (m, e)) + np.float32(0.25)
    feats[5] = 0
    start = synth.normal(78, "ema_raw0", (S + 1, 2, e))
    assert start.dtype == feats.dtype == np.float32
    start[:S] /= np.linalg.norm(start[:S], axis=2, keepdims=True)
    start[S] = SENTINEL

    def fit(gslot, gold_row, gstart, src):
        gal = _dev(start)
        table = _i32(np.concatenate([gslot, gold_row, gstart, src]))
        g, k = len(gslot), len(src)
        _store_lib.check(lib.busca_store_ema_fit(gal.data_ptr(), S, 2, e, _dev(feats).data_ptr(), m, table.data_ptr(), table[g:].data_ptr(),
                                                 table[2 * g:].data_ptr(), table[3 * g + 1:].data_ptr(), g, k, 0.9, 0, None))
        torch.cuda.synchronize()
        return gal.cpu().numpy()
    # slot 2 (has a sample in ring row 1) is fed rows 3, 0, 4; slot 0 has none and is fed row 1; slot 4 is fed the zero row; then three skipped groups
    # (slot -1, slot S, a ring row beyond the ring) and, in slot 5's list, a feature row beyond m
    many = fit([2, 0, 4, -1, S, 1, 5], [1, -1, 0, 0, 0, 2, -1], [0, 3, 4, 5, 6, 7, 8, 10], [3, 0, 4, 1, 5, 2, 2, 2, m, 6])
    one = fit([2], [1], [0, 3], [3, 0, 4])
    assert same(many[2, 0], one[2, 0]) and not same(many[2, 0], start[2, 0])
    def chain(dt):                                          # slot 2 from its stored sample through rows 3, 0, 4: the restatement's lines, `gal[t]` given
        old = start[2, 1].astype(dt)
        for j in (3, 0, 4):
            f = feats[j].astype(dt)
            old = dt(0.9) * old + dt(1 - 0.9) * (f / np.linalg.norm(f))
            old = old / np.linalg.norm(old)
        return old

    def first(j, dt):                                       # a target without a sample stores f / ||f||
        return feats[j].astype(dt) / np.linalg.norm(feats[j].astype(dt))
    pairs = [(chain(np.float32), chain(np.float64), many[2, 0]), (first(1, np.float32), first(1, np.float64), many[0, 0]),
             (first(6, np.float32), first(6, np.float64), many[5, 0])]          # slot 5: the row beyond m is skipped, row 6 stored
    bar = 4 * max(np.abs(w32.astype(np.float64) - w64).max() for w32, w64, _ in pairs)
    assert 0 < bar < 1e-6 and all(w32.dtype == np.float32 and np.abs(got.astype(np.float64) - w32).max() <= bar for w32, _, got in pairs)
    assert np.isnan(many[4, 0]).all()                       # the zero row: 0 / 0, and the blend of a NaN
    untouched = [(1, 0), (1, 1), (3, 0), (3, 1), (2, 1), (0, 1), (4, 1), (5, 1), (S, 0), (S, 1)]
    assert all(same(many[s, r], start[s, r]) for s, r in untouched)


class Spy:
    """A library handle that counts the calls of the entry points whose name starts with `prefix`."""

    def __init__(self, lib, prefix):
        self._lib, self._prefix, self.calls = lib, prefix, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(self._prefix) or name.endswith(("_last_error", "_version")):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def _recorder():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))
    return Recorder()


@gpu
def test_one_launch_per_call(ctx, monkeypatch):
    import torch
    from busca_amd import _store_lib, tracking
    g = gold()
    spy = Spy(_store_lib.load(), "busca_store_")
    monkeypatch.setattr(_store_lib, "_lib", spy)
    hip = Spy(ctx.lib, "busca_ghost_proxies")
    monkeypatch.setattr(ctx, "lib", hip)
    store, ref = tracking.GhostGallery(CAPACITY, BUDGET, E, ctx=ctx), NpStore(CAPACITY, BUDGET, E)
    cfg = dict(avg_act={"do": True, "proxy": "mv_avg", "num": A_ACT}, avg_inact={"do": True, "proxy": "mv_avg", "num": A_INACT})
    for f in range(8):
        fr = frame(g, f)
        ops = [_i32(fr["release"]), _i32(fr["slots"]), _dev(fr["det"]), _i32(fr["det_index"]), _dev(fr["new"].astype(np.uint8))]
        if f == 5:
            ops[4] = ops[4].bool()                          # a bool flag vector is read in place as well
        torch.cuda.synchronize()
        del spy.calls[:]
        with _recorder() as rec:
            if len(fr["release"]):
                store.release(ops[0])
            store.add(*ops[1:])
        assert spy.calls == ["busca_store_release"] * bool(len(fr["release"])) + ["busca_store_ring_add"] and rec.ops == [], (f, spy.calls, rec.ops)
        ref.release(fr["release"])
        ref.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
        del spy.calls[:], hip.calls[:]
        tracking.ghost_round(store.state(fr["active"], fr["inactive"]), ops[2], cfg=cfg, ctx=ctx)
        assert spy.calls == ["busca_store_mv_avg"] and hip.calls == [], (f, spy.calls, hip.calls)
        slots = list(fr["active"]) + list(fr["inactive"])
        assert same(store.mv_avg.cpu().numpy()[slots], g["mv_tab_%d" % f][slots]) and same(store.count.cpu().numpy(), ref.count), f
    assert any(len(frame(g, f)["release"]) for f in range(8))
    # one weight for both groups, and 'mv_avg' beside another proxy: still one blend launch (the other group's proxy is a busca_ghost_proxies call)
    fr = frame(g, 7)
    for inact, proxies in (({"do": True, "proxy": "mv_avg", "num": A_ACT}, 0), ({"do": True, "proxy": "mean", "num": 3}, 1)):
        del spy.calls[:], hip.calls[:]
        tracking.ghost_round(store.state(fr["active"], fr["inactive"]), fr["det"], cfg=dict(cfg, avg_inact=inact), ctx=ctx)
        assert spy.calls == ["busca_store_mv_avg"] and len(hip.calls) == proxies, (inact, spy.calls, hip.calls)
    # other dtypes are converted with one tensor op each; host lists travel in one upload
    fr = frame(g, 8)
    ops = [_dev(fr["slots"].astype(np.int64)), _dev(fr["det"]), _i32(fr["det_index"]), _dev(fr["new"].astype(np.uint8))]
    del spy.calls[:]
    with _recorder() as rec:
        store.add(*ops)
    assert spy.calls == ["busca_store_ring_add"] and len(rec.ops) == 1, rec.ops
    # the EMA fit: a target three times in one call, one launch
    metric = tracking.NearestNeighborDistanceMetric("cosine", 0.4, ctx=ctx)
    feats, targets, active = _ema_rounds(64)[4]
    assert targets.count(2) == 3
    for _ in range(2):                                      # targets without a sample, then with one
        del spy.calls[:]
        metric.partial_fit(feats, targets, active, ema_alpha=0.9)
        assert spy.calls == ["busca_store_ema_fit"]


def _frame8():
    """The store after frame 7 and frame 8's operands, as the stream-order test of tests/test_ghost_store.py takes them."""
    g, ref = gold(), replay_numpy(8)
    return g, ref, frame(g, 8)


@gpu
def test_stream_order_ring_add_and_release(busy):
    import torch
    from busca_amd import _store_lib
    from tests.test_streams_gpu import _nan, behind
    lib = _store_lib.load()
    g, ref, fr = _frame8()
    true = [_dev(ref.gallery), _dev(ref.count), _dev(ref.newest), _dev(ref.mv_seen), _dev(fr["det"]), _i32(fr["slots"]), _i32(fr["det_index"]),
            _dev(fr["new"].astype(np.uint8))]
    poison = [_nan(true[0]), torch.zeros_like(true[1]), torch.full_like(true[2], 3), torch.ones_like(true[3]), _nan(true[4]), true[5].flip(0).contiguous(),
              torch.zeros_like(true[6]), 1 - true[7]]
    k, m = len(fr["slots"]), fr["det"].shape[0]
    want, _ = behind(busy, "busca_store_ring_add", lambda x, o, st: _store_lib.check(lib.busca_store_ring_add(
        x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr(), CAPACITY, BUDGET, E, x[5].data_ptr(), k, x[4].data_ptr(), m, x[6].data_ptr(),
        x[7].data_ptr(), 0, st)), true, poison)
    ref.release(fr["release"])
    ref.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
    assert same(want[1], ref.count) and same(want[0][ref.count > 0], ref.gallery[ref.count > 0])
    live = np.nonzero(ref.count)[0].astype(np.int32)
    gone, kept = live[::2].copy(), live[1::2].copy()
    true = [_dev(ref.count), _dev(np.ones(CAPACITY, dtype=np.uint8)), _i32(gone)]
    poison = [torch.full_like(true[0], 2), torch.zeros_like(true[1]), _i32(np.resize(kept, len(gone)))]
    want, _ = behind(busy, "busca_store_release", lambda x, o, st: _store_lib.check(lib.busca_store_release(
        x[0].data_ptr(), x[1].data_ptr(), CAPACITY, x[2].data_ptr(), len(gone), 0, st)), true, poison)
    assert (want[0][gone] == 0).all() and same(want[0][kept], ref.count[kept]) and (want[1][gone] == 0).all() and (want[1][kept] == 1).all()


@gpu
def test_stream_order_mv_avg(busy):
    import torch
    from busca_amd import _store_lib
    from tests.test_streams_gpu import _nan, behind
    lib = _store_lib.load()
    g, ref, fr = _frame8()
    ref.release(fr["release"])
    ref.add(fr["slots"], fr["det"], fr["det_index"], fr["new"])
    slots = np.concatenate([fr["active"], fr["inactive"]]).astype(np.int32)
    true = [_dev(ref.gallery), _dev(ref.count), _dev(ref.newest), _dev(ref.mv_avg), _dev(ref.mv_seen), _i32(slots)]
    poison = [_nan(true[0]), torch.full_like(true[1], 1), torch.zeros_like(true[2]), _nan(true[3]), 1 - true[4], true[5].flip(0).contiguous()]
    out = torch.empty(len(slots), E, dtype=torch.float32, device=true[0].device)
    want, _ = behind(busy, "busca_store_mv_avg", lambda x, o, st: _store_lib.check(lib.busca_store_mv_avg(
        x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr(), x[4].data_ptr(), CAPACITY, BUDGET, E, x[5].data_ptr(), len(slots),
        len(fr["active"]), A_ACT, A_INACT, o[0].data_ptr(), 0, st)), true, poison, lambda: [out.fill_(-7.0)])
    assert same(want[6], g["mv_px_8"]) and same(want[3][slots], g["mv_tab_8"][slots]) and same(want[4], g["mv_seen_8"])


@gpu
def test_stream_order_ema_fit(busy):
    from busca_amd import _store_lib, synth
    from tests.test_streams_gpu import _nan, behind
    lib = _store_lib.load()
    S, e, m = 5, 65, 6
    feats = synth.normal(81, "ema_stream", (m, e)) + np.float32(0.25)
    start = synth.normal(82, "ema_stream0", (S, 1, e))
    start /= np.linalg.norm(start, axis=2, keepdims=True)
    gslot, gold_row, gstart, src = [3, 0, 1], [0, -1, 0], [0, 3, 4, 6], [2, 5, 0, 1, 4, 3]
    true = [_dev(start), _dev(feats), _i32(np.concatenate([gslot, gold_row, gstart, src]))]
    poison = [_nan(true[0]), _nan(true[1]), _i32(np.concatenate([[1, 3, 0], [-1, 0, -1], [0, 1, 2, 6], src[::-1]]))]
    g, k = len(gslot), len(src)
    want, _ = behind(busy, "busca_store_ema_fit", lambda x, o, st: _store_lib.check(lib.busca_store_ema_fit(
        x[0].data_ptr(), S, 1, e, x[1].data_ptr(), m, x[2].data_ptr(), x[2][g:].data_ptr(), x[2][2 * g:].data_ptr(), x[2][3 * g + 1:].data_ptr(), g, k,
        0.9, 0, st)), true, poison)
    assert np.isfinite(want[0]).all() and same(want[0][[2, 4]], start[[2, 4]]) and not same(want[0][[3, 0, 1]], start[[3, 0, 1]])
    assert np.abs(np.linalg.norm(want[0][:, 0].astype(np.float64), axis=1) - 1).max() < 1e-6
