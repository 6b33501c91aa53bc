"""A whole ByteTrack frame on resident Kalman state: libbusca_frame.so (include/busca_frame.h), its binding busca_amd._frame_lib and
KalmanStore.frame - predict, the cost slab of the three rounds, busca_assign_stages, update and initiation as one chain on the stream.

The reference is the route this repository had before: KalmanStore.round three times with the lists compacted on the host between the calls
exactly as BYTETracker.update does it (adapters/ByteTrack/yolox/tracker/byte_tracker.py:244-249, 312-425), then KalmanStore.update and
KalmanStore.initiate (`_composed` below).  Everything is compared with np.array_equal - match lists, unmatched lists, new tracks, and the means and
covariances of the whole store: the kernels of the frame run the per-track bodies of the kernels behind those calls.  The 16-frame script of
tests/golden/kalman_store.npz is replayed as well: its detections sit on their tracks (IoU >= 0.6 with the own track, <= 0.13 with any other), so
the association finds the script's pairs, and the states must land where the existing replay (tests/test_kalman_store.py, which pins its predictions
and initiations to the fixture bit for bit) lands them: equal in every bit after every frame."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kalman_filter import _detections, gold
from tests.test_kalman_store import CAP, PERM, _dev, _near, _state_of, _store, _untouched, phase, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_THRESH, MATCH_THRESH, DET_THRESH = 0.6, 0.8, 0.7
SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (96, 40)]            # the edges of the 16 x 64 tile
# scores by detection (or by group of duplicates), cycled: the three classes, scores equal to track_thresh and to low_thresh (class 2 both), and
# first-round scores on either side of det_thresh
SCORES = np.array([0.95, 0.4, 0.8, 0.05, 0.65, 0.6, 0.2, 0.9, 0.1, 0.75])
# the scores of the 1st .. 4th detection that sits on a track, by track number modulo 5: first-round detections only; second-round and below; a
# first-round one below det_thresh first; none of either round (0.6 is track_thresh itself); first and second round mixed
BY_TRACK = np.array([[0.95, 0.8, 0.9, 0.75], [0.4, 0.2, 0.05, 0.1], [0.65, 0.6, 0.9, 0.3], [0.6, 0.05, 0.1, 0.6], [0.9, 0.4, 0.8, 0.3]])


def _classes(scores):
    """byte_tracker.py:244-249, restated for the tests."""
    scores = np.asarray(scores)
    cls = np.full(len(scores), 2, dtype=np.uint8)
    cls[np.logical_and(scores > 0.1, scores < TRACK_THRESH)] = 1
    cls[scores > TRACK_THRESH] = 0
    return cls


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _frame_lib, _lib, _rounds_lib, _sort_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_frame.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_frame_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _frame_lib.FRAME_API.items()}
    assert sorted(declared) == ["busca_frame_apply", "busca_frame_cost", "busca_frame_last_error", "busca_frame_version"]
    assert declared["busca_frame_cost"] == 13 and declared["busca_frame_apply"] == 18

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_frame_lib.FRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_frame_lib.FRAME_API)
    others = [hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH, _rounds_lib.ROUNDS_LIB_PATH, _sort_lib.SORT_LIB_PATH]
    assert os.path.basename(hip_lib) == "libbusca_hip.so" and len({os.path.basename(p) for p in others}) == 5
    for other in others:
        theirs = {n for n in exported(other) if not n.startswith("_")}
        assert not [n for n in theirs if n.startswith("busca_frame")], other
        assert not (theirs & ours), other
    assert "busca_frame.h" not in _lib.HEADERS and "_frame_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _frame_lib.load()
    assert lib.busca_frame_version() == 1000 and _frame_lib.ABI_MAJOR == 1 and lib.busca_frame_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _frame_lib
    lib = _frame_lib.load()
    P, ODD, S, n, m = 0x10000, 0x10004, 8, 3, 5          # an aligned address, one that is 4- but not 8-byte aligned

    def calls(mean=P, cov=P, S=S, slot=P, n=n, tlbr=P, xyah=P, score=P, cls=P + 1, m=m, out=P, status=P, r2c=P, c2r=P, thresh=0.7, free=P, n_free=2,
              new=P, dev=0):
        return {
            "busca_frame_cost": lambda: lib.busca_frame_cost(mean, cov, S, slot, n, tlbr, score, cls, m, out, status, dev, None),
            "busca_frame_apply": lambda: lib.busca_frame_apply(mean, cov, S, slot, n, r2c, c2r, xyah, score, cls, m, thresh, free, n_free, new, status,
                                                               dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_frame_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    for name in calls():
        assert calls(n=0, m=0)[name]() == 0, name                                  # the no-op
        assert calls(n=0, m=0, mean=None, cov=None, slot=None, out=None, r2c=None, c2r=None, xyah=None, tlbr=None, cls=None, new=None, free=None)[name]() == 0
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", slot=None)
        refused(name, "null pointer", cls=None)
        refused(name, "negative size", n=-1)
        refused(name, "negative size", m=-1)
        refused(name, "negative size", S=-1)
        refused(name, "negative device", dev=-1)
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", cov=ODD)
        refused(name, "misaligned", score=ODD)
        refused(name, "misaligned", slot=0x10002)
        refused(name, "misaligned", status=0x10002)
    name = "busca_frame_cost"
    assert calls(n=0)[name]() == 0 and calls(m=0)[name]() == 0
    refused(name, "null pointer", tlbr=None)
    refused(name, "null pointer", out=None)
    refused(name, "misaligned", tlbr=ODD)
    refused(name, "misaligned", out=ODD)
    refused(name, "more workgroups than a grid holds", n=16 * 65535 + 1)
    name = "busca_frame_apply"
    refused(name, "negative size (n_free", n_free=-1)
    refused(name, "det_thresh is NaN", thresh=float("nan"))
    refused(name, "one call takes 2048", m=2049)
    refused(name, "null pointer", cov=None)
    refused(name, "null pointer", r2c=None)
    refused(name, "null pointer", c2r=None)
    refused(name, "null pointer", xyah=None)
    refused(name, "null pointer", new=None)
    refused(name, "null pointer", free=None)
    refused(name, "misaligned", xyah=ODD)
    refused(name, "misaligned", r2c=0x10002)
    refused(name, "misaligned", c2r=0x10002)
    refused(name, "misaligned", free=0x10002)
    refused(name, "misaligned", new=0x10002)
    # the message is the calling thread's own
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_frame_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_frame_last_error() != b""


def test_python_level_checks():
    import sys
    from busca_amd import tracking
    from busca_amd.kalman_store import ByteFrame, KalmanStore, _frame_classes, _frame_row_tables
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    import busca.tracking as alias
    assert tracking.ByteFrame is ByteFrame is alias.ByteFrame
    assert ByteFrame._fields == ("first", "second", "unconfirmed", "unmatched_pool", "unmatched_unconfirmed", "new_tracks", "overflow", "det_class")
    # classes from scores, by the comparisons of the reference: a score equal to a threshold belongs to neither round
    scores = [0.9, 0.6, 0.59, 0.1, 0.100001, 0.0, 0.61, float("nan")]
    assert _frame_classes(scores, 0.6).tolist() == [0, 2, 1, 2, 1, 2, 0, 2]
    assert _frame_classes(scores, 0.6).dtype == np.uint8 and _frame_classes([], 0.6).shape == (0,)
    assert _frame_classes(np.float32(scores), np.float32(0.6)).tolist() == [0, 2, 1, 2, 1, 2, 0, 2]      # on the array as given: float32 against float32
    assert _frame_classes([0.3, 0.2, 0.25], 0.3, low_thresh=0.2).tolist() == [2, 2, 1]
    assert np.array_equal(_frame_classes(SCORES, TRACK_THRESH), _classes(SCORES)) and _classes(SCORES).tolist() == [0, 1, 0, 2, 0, 2, 1, 0, 2, 0]
    # the row tables of a mixed pool
    first, again, lost = _frame_row_tables([False, True, True, False], 4, 2)
    assert first.tolist() == [0, 0, 0, 0, 2, 2] and again.tolist() == [1, -1, -1, 1, -1, -1] and lost.tolist() == [False, True, True, False]
    assert first.dtype == again.dtype == np.int32
    assert [t.tolist() for t in _frame_row_tables([], 0, 0)[:2]] == [[], []]
    # refused before anything is allocated
    st = KalmanStore(CAP)
    dets = _detections(np.array([[100.0, 100.0, 0.5, 80.0]] * 3))
    sc = [0.9, 0.3, 0.9]
    ok = dict(track_thresh=0.6, match_thresh=0.8, det_thresh=0.7)
    for kw, words in ((dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[3], free_slots=[4, 2]), "also listed"),
                      (dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[3], free_slots=[3]), "also listed"),
                      (dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[3], free_slots=[4, 5, 4]), "distinct"),
                      (dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[2], free_slots=[4]), "distinct"),
                      (dict(pool_slots=[1, 1], lost=[0, 0], unconfirmed_slots=[], free_slots=[4]), "distinct"),
                      (dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[], free_slots=[-1]), "negative"),
                      (dict(pool_slots=[1, CAP], lost=[0, 0], unconfirmed_slots=[], free_slots=[]), "beyond the capacity"),
                      (dict(pool_slots=[1, 2], lost=[0, 0], unconfirmed_slots=[], free_slots=[CAP]), "beyond the capacity"),
                      (dict(pool_slots=[1, 2], lost=[0], unconfirmed_slots=[3], free_slots=[4]), "`lost` flags"),
                      (dict(pool_slots=[1, 2], lost=[0, 0, 1], unconfirmed_slots=[3], free_slots=[4]), "`lost` flags")):
        with pytest.raises(ValueError, match=words):
            st.frame(detections=dets, det_scores=sc, **kw, **ok)
    with pytest.raises(ValueError, match="2 scores for 3 detections"):
        st.frame([1, 2], [0, 0], [3], dets, sc[:2], **ok)
    import torch
    with pytest.raises(ValueError, match="detection objects"):
        st.frame([1, 2], [0, 0], [3], torch.ones(3, 4), sc, **ok)
    assert st.mean is None                                                         # nothing was allocated


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


class Scene:
    """n tracks on a grid of overlapping boxes - the pool (Tracked and lost rows mixed), then n // 4 unconfirmed ones - in scattered slots of a
    store of 128, and m detections sitting on tracks, with the scores of SCORES.  `tie`: everything on integer coordinates, no velocities, every
    detection box two or three times with one score - whole columns of the cost matrices are equal."""

    def __init__(self, n, m, seed, tie=False, n_unconfirmed=None, scores=None):
        rs = np.random.RandomState(seed)
        g = gold()
        nn = n if n else 8                                       # without tracks the detections sit where 8 tracks would be
        i = np.arange(nn)
        mean = np.zeros((nn, 8))
        mean[:, 0], mean[:, 1], mean[:, 2], mean[:, 3] = 200 + 30 * (i % 8), 150 + 60 * (i // 8), 0.5, 80
        if not tie:
            mean[:, :2] += rs.uniform(-5, 5, (nn, 2))
            mean[:, 3] *= rs.uniform(0.9, 1.1, nn)
            mean[:, 4:6] = rs.uniform(-2, 2, (nn, 2))
            mean[:, 7] = rs.uniform(-0.5, 0.5, nn)
        self.mean, self.cov = mean[:n], g["cov"][i % 96][:n].copy()
        self.n, self.m = n, m
        self.n_unc = n // 4 if n_unconfirmed is None else n_unconfirmed
        self.n_pool = n - self.n_unc
        self.lost = np.arange(self.n_pool) % 3 == 1
        self.slots = PERM[:n].astype(np.int64)
        self.pool, self.unc = self.slots[:self.n_pool], self.slots[self.n_pool:]
        self.free = PERM[n:].astype(np.int64)
        if tie:
            group = np.cumsum(np.arange(m) % 5 % 3 == 0) - 1          # groups of 3, 2, 3, 2 ... detections
            on = (group * 5) % nn
            xyah = mean[on, :4].copy()
            xyah[:, 0] += (group % 3 - 1) * 4
            xyah[:, 1] += (group % 2) * 6
            score = SCORES[group % len(SCORES)]
        else:
            j = np.arange(m)
            on = (j * 7) % nn
            xyah = mean[on, :4] + mean[on, 4:]                            # where the prediction puts the track
            xyah[:, :2] += rs.uniform(-6, 6, (m, 2))
            xyah[:, 3] *= rs.uniform(0.92, 1.08, m)
            score = BY_TRACK[on % 5, (j // nn) % 4]                       # what a track is offered depends on the track
            far = j % 9 == 4                                              # newcomers, far from every track: on either side of det_thresh
            xyah[far] = np.stack([2000.0 + 50 * j[far], 300.0 + 0 * j[far], 0.5 + 0 * j[far], 80.0 + 0 * j[far]], 1)
            score[far] = np.where((j[far] // 9) % 2 == 0, 0.9, 0.65)
        from busca_amd.kalman import _measurements
        self.dets = _detections(xyah)
        self.xyah = _measurements(self.dets)                     # what every route reads from the objects
        self.scores = score if scores is None else np.broadcast_to(np.asarray(scores, dtype=np.float64), (m,)).copy()

    def store(self):
        return _store(128, self.mean, self.cov, self.slots)


def _composed(st, sc, free, mot20=False, det_thresh=DET_THRESH):
    """The frame on the route this repository had before: three rounds, the lists compacted on the host between them as byte_tracker.py:312-425
    compacts them, then update and initiate.  -> what ByteFrame holds, as plain lists."""
    scores, dets, lost = sc.scores, sc.dets, sc.lost
    hi = np.nonzero(scores > TRACK_THRESH)[0]
    lo = np.nonzero(np.logical_and(scores > 0.1, scores < TRACK_THRESH))[0]
    m1, ut, ud = st.round(sc.pool, [dets[j] for j in hi], MATCH_THRESH, det_scores=None if mot20 else scores[hi], not_tracked=lost)
    first = [(int(r), int(hi[c])) for r, c in m1]
    r_tracked = [int(i) for i in ut if not lost[i]]
    r_lost = [int(i) for i in ut if lost[i]]
    m2, ut2, _ = st.round(sc.pool[r_tracked], [dets[j] for j in lo], 0.5, predict=False)
    second = [(r_tracked[r], int(lo[c])) for r, c in m2]
    unmatched_pool = [r_tracked[i] for i in ut2] + r_lost
    left = [int(hi[c]) for c in ud]
    m3, uu, ud3 = st.round(sc.unc, [dets[j] for j in left], 0.7, det_scores=None if mot20 else scores[left], predict=False)
    unconfirmed = [(int(r), left[c]) for r, c in m3]
    starts = [left[c] for c in ud3 if not scores[left[c]] < det_thresh]
    pairs = [(sc.pool[r], j) for r, j in first + second] + [(sc.unc[r], j) for r, j in unconfirmed]
    status = st.update([s for s, _ in pairs], sc.xyah, [j for _, j in pairs]).cpu().numpy()
    k = min(len(starts), len(free))
    st.initiate(free[:k], sc.xyah, starts[:k])
    return dict(first=first, second=second, unconfirmed=unconfirmed, unmatched_pool=unmatched_pool, unmatched_unconfirmed=[int(r) for r in uu],
                new_tracks=[(j, int(s)) for j, s in zip(starts[:k], free[:k])], overflow=starts[k:], status=status)


def _frame(st, sc, free, **kw):
    return st.frame(sc.pool, sc.lost, sc.unc, sc.dets, sc.scores, TRACK_THRESH, MATCH_THRESH, kw.pop("det_thresh", DET_THRESH), free_slots=free, **kw)


def _agree(sc, free, what, **kw):
    """frame() on one store, the composed route on a copy: the same lists, the same bits in every slot."""
    a, b = sc.store(), sc.store()
    before = _state_of(a)
    got = _frame(a, sc, free, **kw)
    want = _composed(b, sc, free, **{k: v for k, v in kw.items() if k in ("mot20", "det_thresh")})
    assert not want["status"].any(), what
    for field in ("first", "second", "unconfirmed", "unmatched_pool", "unmatched_unconfirmed", "new_tracks", "overflow"):
        assert [tuple(x) if isinstance(x, tuple) else int(x) for x in getattr(got, field)] == want[field], (what, field, getattr(got, field), want[field])
    assert np.array_equal(got.det_class, _classes(sc.scores)), what
    after, ref = _state_of(a), _state_of(b)
    assert np.array_equal(after[0], ref[0]) and np.array_equal(after[1], ref[1]), what
    touched = list(sc.pool) + [sc.unc[r] for r, _ in want["unconfirmed"]] + [s for _, s in want["new_tracks"]]
    _untouched(before, after, touched, what)
    return got


def _raw_cost(st, slot, n, sc, cls, with_scores, guard=64, canary=777.25):
    """busca_frame_cost itself into a slab with a guard band on both sides -> (the slab [2, n, m], the status words)."""
    import torch
    from busca_amd import _frame_lib
    m = sc.m
    det = st.detections(sc.dets, sc.scores)
    buf = torch.full((2 * n * m + 2 * guard,), canary, dtype=torch.float64, device=st.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    d_cls = _dev(cls)
    _frame_lib.check(_frame_lib.load().busca_frame_cost(st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, slot.data_ptr(), n, det.tlbr.data_ptr(),
                                                        det.score.data_ptr() if with_scores else None, d_cls.data_ptr(), m,
                                                        buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *st._where()))
    buf, status = buf.cpu().numpy(), status.cpu().numpy()
    assert (buf[:guard] == canary).all() and (buf[guard + 2 * n * m:] == canary).all(), "written outside the slab"
    assert (status[:guard] == -7).all() and (status[guard + n:] == -7).all(), "written outside the status words"
    return buf[guard:guard + 2 * n * m].reshape(2, n, m), status[guard:guard + n]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", SHAPES)
def test_cost_planes(n, m):
    sc = Scene(n, m, 11 + n)
    st = sc.store()
    cls = _classes(sc.scores)
    if m > 2:
        cls[2] = 7                                           # any other byte: a detection of neither round
    for holes in (False, True):
        slots = sc.slots.astype(np.int32)
        if holes:                                            # skipped entries: negative, and beyond the capacity
            slots = np.insert(slots, [0, n // 2, n], [-1, 128, 2 ** 31 - 1]).astype(np.int32)
        slot = _dev(slots)
        rows = len(slots)
        with_sc, status0 = st.cost(slot, sc.dets, sc.scores)
        plain, _ = st.cost(slot, sc.dets)
        with_sc, plain = with_sc.cpu().numpy(), plain.cpu().numpy()
        for mot20 in (False, True):
            slab, status = _raw_cost(st, slot, rows, sc, cls, not mot20)
            want0 = np.where(cls == 0, plain if mot20 else with_sc, np.inf)
            want1 = np.where(cls == 1, plain, np.inf)
            assert np.array_equal(slab[0], want0) and np.array_equal(slab[1], want1), (n, m, holes, mot20)
            assert not status.any() and not status0.cpu().numpy().any()
            if holes:
                assert np.isposinf(slab[:, [0, n // 2 + 1, rows - 1]]).all()
        if (n, m) == (96, 40) and not holes:
            assert (with_sc[:, cls == 0] < 0.8).sum() >= 10 and (plain[:, cls == 1] < 0.5).sum() >= 3      # the planes are not all far apart


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(17, 65), (96, 40)])
@pytest.mark.parametrize("mot20", [False, True])
def test_frame_equals_the_composed_route(n, m, mot20):
    sc = Scene(n, m, 5 + n)
    got = _agree(sc, sc.free[:12], (n, m, mot20), mot20=mot20)
    print("frame %dx%d mot20=%s: %d first, %d second, %d unconfirmed, %d + %d left, %d new, %d overflow" % (
        n, m, mot20, len(got.first), len(got.second), len(got.unconfirmed), len(got.unmatched_pool), len(got.unmatched_unconfirmed),
        len(got.new_tracks), len(got.overflow)))
    assert got.first and got.second and got.unconfirmed and got.new_tracks and got.unmatched_pool      # every list of the frame is exercised
    assert all(not sc.lost[r] for r, _ in got.second)                                              # a lost track takes no second-round detection
    # apply=False: the same matches, and the state is only predicted
    a, b = sc.store(), sc.store()
    dry = _frame(a, sc, sc.free[:12], mot20=mot20, apply=False)
    assert (dry.first, dry.second, dry.unconfirmed, dry.unmatched_pool) == (got.first, got.second, got.unconfirmed, got.unmatched_pool)
    assert dry.new_tracks == [] and dry.overflow == []
    b.predict(sc.pool, sc.lost)
    assert all(np.array_equal(x, y) for x, y in zip(_state_of(a), _state_of(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(17, 65), (96, 40)])
def test_ties(n, m):
    sc = Scene(n, m, 3, tie=True)
    # the scene does tie: columns of the slab that are equal, bit for bit
    st = sc.store()
    cost = st.cost(sc.slots, sc.dets, sc.scores)[0].cpu().numpy()
    assert sum(np.array_equal(cost[:, j], cost[:, j + 1]) for j in range(m - 1)) >= m // 3
    got = _agree(sc, sc.free[:8], ("ties", n, m))
    assert len(got.first) + len(got.second) + len(got.unconfirmed) >= 4


def _raw_apply(st, slot, r2c, c2r, xyah, scores, cls, det_thresh, free, guard=16):
    import torch
    from busca_amd import _frame_lib
    n, m, n_free = len(slot), len(c2r), len(free)
    d = [_dev(np.asarray(x, dtype=np.int32)) if len(x) else None for x in (slot, r2c, c2r, free)]
    d_xyah, d_score, d_cls = _dev(np.asarray(xyah, dtype=np.float64)), None if scores is None else _dev(np.asarray(scores, dtype=np.float64)), _dev(cls)
    new = torch.full((m + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _frame_lib.check(_frame_lib.load().busca_frame_apply(st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, ptr(d[0]), n, ptr(d[1]), ptr(d[2]),
                                                         d_xyah.data_ptr(), ptr(d_score), d_cls.data_ptr(), m, det_thresh, ptr(d[3]), n_free,
                                                         new.data_ptr() + 4 * guard, status.data_ptr() + 4 * guard, *st._where()))
    new, status = new.cpu().numpy(), status.cpu().numpy()
    assert (new[:guard] == -7).all() and (new[guard + m:] == -7).all() and (status[:guard] == -7).all() and (status[guard + n:] == -7).all()
    return new[guard:guard + m], status[guard:guard + n]


@pytest.mark.gpu
def test_initiation_ranks():
    import torch
    from busca_amd.kalman_store import KalmanStore
    g = gold()
    S, GUARD, CANARY, m = 24, 6, 777.25, 150
    xyah = g["init_meas"][np.arange(m) % 64]
    scores = SCORES[np.arange(m) % 10]
    scores[::7] = 0.65                                       # first round, below det_thresh: starts nothing
    cls = _classes(scores)
    rs = np.random.RandomState(9)
    c2r = np.where(rs.uniform(size=m) < 0.4, 3, -1).astype(np.int32)             # matched columns scattered among the others
    eligible = [j for j in range(m) if c2r[j] < 0 and cls[j] == 0 and not scores[j] < DET_THRESH]
    assert len(eligible) > 20 and eligible[-1] > 128                             # ranks beyond one pass of the 64-lane loop
    free = np.array([5, 2, S + 3, 11, -4, 0, 7], dtype=np.int32)                 # one beyond the capacity, one negative: skipped, and reported
    assert len(eligible) > len(free)

    def run():
        mean_buf = torch.full((S + 1 + GUARD, 8), CANARY, dtype=torch.float64, device="cuda:0")
        cov_buf = torch.full((S + 1 + GUARD, 8, 8), CANARY, dtype=torch.float64, device="cuda:0")
        st = KalmanStore(S)
        st._state()
        st.mean, st.cov = mean_buf[:S + 1], cov_buf[:S + 1]
        new, _ = _raw_apply(st, [], [], c2r, xyah, scores, cls, DET_THRESH, free)
        return new, mean_buf.cpu().numpy(), cov_buf.cpu().numpy()
    new, mean, cov = run()
    want = np.full(m, -1, dtype=np.int32)
    want[eligible[:len(free)]] = free                        # slots are taken in ascending detection order
    want[eligible[len(free):]] = -2                          # the surplus: the store is full
    assert np.array_equal(new, want)
    ref = _store(S)
    live = [k for k, s in enumerate(free) if 0 <= s < S]
    ref.initiate(free[live], xyah, np.asarray(eligible)[live])
    rm, rc = _state_of(ref)
    taken = free[live]
    assert np.array_equal(mean[taken], rm[taken]) and np.array_equal(cov[taken], rc[taken])
    assert np.array_equal(mean[taken], g["init_mean"][np.asarray(eligible)[live] % 64])
    rest = np.ones(S + 1 + GUARD, dtype=bool)
    rest[taken] = False
    assert (mean[rest] == CANARY).all() and (cov[rest] == CANARY).all()          # nothing else of the store or behind it was written
    again = run()
    assert np.array_equal(again[0], new) and np.array_equal(again[1], mean) and np.array_equal(again[2], cov)
    # without scores every unmatched first-round column starts a track
    st = _store(S)
    new, _ = _raw_apply(st, [], [], c2r, xyah, None, cls, DET_THRESH, np.arange(S, dtype=np.int32))
    all_hi = [j for j in range(m) if c2r[j] < 0 and cls[j] == 0]
    assert np.array_equal(np.nonzero(new >= 0)[0], all_hi[:S]) and np.array_equal(np.nonzero(new == -2)[0], all_hi[S:])
    # through frame(): no tracks at all, fewer free slots than new tracks
    sc = Scene(0, 40, 2)
    got = _agree(sc, PERM[:3].astype(np.int64), "overflow")
    assert len(got.new_tracks) == 3 and len(got.overflow) >= 3 and [s for _, s in got.new_tracks] == PERM[:3].tolist()
    assert got.first == got.second == got.unconfirmed == got.unmatched_pool == got.unmatched_unconfirmed == []


@pytest.mark.gpu
def test_not_positive_definite():
    g = gold()
    idx = [4, 5, 6]
    mean, cov = g["mean"][idx].copy(), g["cov"][idx].copy()
    cov[1, :4, :4] = -np.eye(4)
    slots = [9, 2, 5]
    xyah = mean[:, :4] + mean[:, 4:]                         # every detection on its track's prediction; a host array: measurements as they are
    dets = xyah
    st, ref = _store(CAP, mean, cov, slots), _store(CAP, mean, cov, slots)
    ref.predict(slots, [False] * 3)
    kept = _state_of(ref)
    status = ref.update(slots, xyah).cpu().numpy()
    assert status.tolist() == [0, 1, 0]
    with pytest.raises(np.linalg.LinAlgError, match="KalmanStore.frame: the projected covariance of track 1"):
        st.frame(slots, [False] * 3, [], dets, [0.9] * 3, TRACK_THRESH, MATCH_THRESH, DET_THRESH)
    got, want = _state_of(st), _state_of(ref)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])                      # rows 0 and 2 are updated ...
    assert np.array_equal(got[0][2], kept[0][2]) and np.array_equal(got[1][2], kept[1][2])          # ... the flagged one keeps its predicted state
    assert not np.array_equal(got[1][9], kept[1][9]) and not np.array_equal(got[1][5], kept[1][5])      # (the innovation is zero: the means stay)
    # the raw call reports it as the update call does
    st = _store(CAP, mean, cov, slots)
    new, status = _raw_apply(st, slots, [2, 0, -1], [1, -1, 0], xyah, [0.9] * 3, np.zeros(3, dtype=np.uint8), DET_THRESH, [])
    assert status.tolist() == [0, 1, 0] and new.tolist() == [-1, -2, -1]


@pytest.mark.gpu
def test_degenerate_frames():
    free = PERM[100:104].astype(np.int64)
    # no detections: only the prediction happens
    sc = Scene(17, 0, 1)
    got = _agree(sc, free, "no detections")
    assert got.unmatched_pool == [i for i in range(sc.n_pool) if not sc.lost[i]] + [i for i in range(sc.n_pool) if sc.lost[i]]
    assert got.unmatched_unconfirmed == list(range(sc.n_unc)) and got.det_class.shape == (0,)
    # no tracks: only initiations happen
    sc = Scene(0, 9, 1)
    got = _agree(sc, free, "no tracks")
    starts = [j for j in range(9) if sc.scores[j] > TRACK_THRESH and not sc.scores[j] < DET_THRESH]
    assert [j for j, _ in got.new_tracks] + got.overflow == starts and 0 < len(starts) < int((sc.scores > TRACK_THRESH).sum())
    # only unconfirmed tracks
    got = _agree(Scene(5, 20, 1, n_unconfirmed=5), free, "only unconfirmed")
    assert got.unconfirmed and not got.first and not got.second
    # only low-score detections: the second round alone
    got = _agree(Scene(17, 30, 1, scores=0.3), free, "only low scores")
    assert got.second and not got.first and not got.unconfirmed and not got.new_tracks
    # every score equal to track_thresh: nothing matches, nothing starts
    got = _agree(Scene(17, 30, 1, scores=TRACK_THRESH), free, "scores equal to track_thresh")
    assert not (got.first or got.second or got.unconfirmed or got.new_tracks or got.overflow) and (got.det_class == 2).all()
    assert len(got.unmatched_pool) == 13 and len(got.unmatched_unconfirmed) == 4
    # no pool, no free slot
    got = _agree(Scene(4, 12, 1, n_unconfirmed=4), free[:0], "no free slot")
    assert not got.new_tracks


@pytest.mark.gpu
def test_a_frame_behind_a_busy_stream(busy):
    from busca_amd.kalman_store import KalmanStore
    from tests.test_streams_gpu import behind
    sc, other = Scene(17, 65, 5 + 17), Scene(17, 65, 99)
    full = lambda s: [_dev(x) for x in _state_of(s.store())]      # noqa: E731
    st = KalmanStore(128)
    st._state()

    def call(x, outs, stream):
        st.mean, st.cov = x
        got = _frame(st, sc, sc.free[:12])
        return [np.asarray(v, dtype=np.int64) for v in got]
    want, got = behind(busy, "KalmanStore.frame", call, true=full(sc), poison=full(other), form="current", host=True)
    assert len(got[2]) >= 4 and len(got[7]) >= 1                  # the frame matched in its first round and started tracks
    ref = sc.store()
    _composed(ref, sc, sc.free[:12])
    assert np.array_equal(got[0], _state_of(ref)[0]) and np.array_equal(got[1], _state_of(ref)[1])


@pytest.mark.gpu
def test_the_script_replays_through_frame():
    from tests.test_kalman_store import _run_frame
    s = script()
    st, ref = _store(CAP), _store(CAP)
    seen = set()
    for f in range(1, 17):
        meas = s["meas"][f - 1, :int(s["meas_m"][f - 1])]
        pool, lost = phase(f, "pred_slot", "pred_n", "pred_nt")
        upd, upd_det = phase(f, "upd_slot", "upd_n", "upd_det")
        ini, ini_det = phase(f, "ini_slot", "ini_n", "ini_det")
        unc = [int(x) for x in upd if x >= 0 and x not in pool]           # updated without having been predicted: unconfirmed
        scores = np.full(len(meas), 0.05)                                 # clutter: in neither round
        scores[[int(j) for x, j in zip(upd, upd_det) if x >= 0]] = 0.9
        scores[ini_det] = 0.9
        if f % 2 == 0 and 3 in upd and not lost[list(pool).index(3)]:     # track A (slot 3) where it is Tracked: through the second round
            scores[upd_det[list(upd).index(3)]] = 0.3
        order = np.argsort(ini_det)                                       # free slots are taken in ascending detection order
        got = st.frame(pool, lost, unc, meas, scores, TRACK_THRESH, MATCH_THRESH, DET_THRESH, free_slots=ini[order])
        _run_frame(ref, f)
        pairs = {(int(pool[r]), j) for r, j in got.first + got.second} | {(unc[r], j) for r, j in got.unconfirmed}
        assert pairs == {(int(x), int(j)) for x, j in zip(upd, upd_det) if x >= 0}, f
        assert got.new_tracks == [(int(ini_det[k]), int(ini[k])) for k in order] and got.overflow == [], f
        seen |= ({"second"} if got.second else set()) | ({"unconfirmed"} if got.unconfirmed else set()) | ({"lost"} if lost.any() else set())
        seen |= ({"skipped"} if (pool < 0).any() else set()) | ({"nothing"} if len(meas) == 0 else set())
        a, b = _state_of(st), _state_of(ref)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f               # where the existing replay lands them, bit for bit
        _near((a[0][:CAP], a[1][:CAP]), (s["mean"][f - 1, 2], s["cov"][f - 1, 2]), f)      # updates: inside the chain bars of the reference
        assert np.array_equal(a[0][ini], s["mean"][f - 1, 2][ini]) and np.array_equal(a[1][ini], s["cov"][f - 1, 2][ini]), f      # initiations: exact
    assert seen == {"second", "unconfirmed", "lost", "skipped", "nothing"}
