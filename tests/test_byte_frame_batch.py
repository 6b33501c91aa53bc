"""The ByteTrack frames of many sequences on one store as one chain: libbusca_mframe.so (include/busca_mframe.h), its binding
busca_amd._mframe_lib and KalmanStore.frame_batch - one prediction, busca_mframe_cost, busca_assign_stages over the batch, busca_mframe_apply and
one copy home, whatever the number of sequences.

The reference is KalmanStore.frame, once per problem, on a second store loaded alike (tests/test_byte_frame.py pins it to the composed route and
tests/test_byte_tracker_replay.py to the recorded tracker).  The scenes are tests/test_byte_frame.Scene, re-homed into disjoint ranges of a
scattered permutation of one store of 512 slots.  Everything is compared with np.array_equal - every field of every ByteFrame and the means and
covariances of the whole store: the kernels of the batch run the tile, row and column bodies of the kernels behind frame()."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests.test_byte_frame import DET_THRESH, MATCH_THRESH, SCORES, TRACK_THRESH, Scene, _classes, _raw_apply, _raw_cost
from tests.test_kalman_filter import gold
from tests.test_kalman_store import _dev, _state_of, _store, _untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 512
PERM = np.random.RandomState(17).permutation(CAP)
FIELDS = ("first", "second", "unconfirmed", "unmatched_pool", "unmatched_unconfirmed", "new_tracks", "overflow")
THRESH = dict(track_thresh=TRACK_THRESH, match_thresh=MATCH_THRESH, det_thresh=DET_THRESH)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _frame_lib, _lib, _mframe_lib, _rounds_lib, _sframe_lib, _sort_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_mframe.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_mframe_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _mframe_lib.MFRAME_API.items()}
    assert sorted(declared) == ["busca_mframe_apply", "busca_mframe_cost", "busca_mframe_last_error", "busca_mframe_version"]
    assert declared["busca_mframe_cost"] == 18 and declared["busca_mframe_apply"] == 22
    for name, val in (("BUSCA_MFRAME_MAX_DETS", _mframe_lib.MAX_DETS), ("BUSCA_MFRAME_MAX_BATCH", _mframe_lib.MAX_BATCH)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val
    assert _mframe_lib.MAX_DETS == _frame_lib.MAX_DETS and _mframe_lib.PROBLEM_WORDS == 6

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_mframe_lib.MFRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_mframe_lib.MFRAME_API)
    others = [hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH, _rounds_lib.ROUNDS_LIB_PATH, _sort_lib.SORT_LIB_PATH,
              _frame_lib.FRAME_LIB_PATH, _sframe_lib.SFRAME_LIB_PATH]
    assert os.path.basename(hip_lib) == "libbusca_hip.so" and len({os.path.basename(p) for p in others}) == 7
    for other in others:
        theirs = {n for n in exported(other) if not n.startswith("_")}
        assert not [n for n in theirs if n.startswith("busca_mframe")], other
        assert not (theirs & ours), other
    assert "busca_mframe.h" not in _lib.HEADERS and len(_lib.HEADERS) == 7 and "_mframe_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _mframe_lib.load()
    assert lib.busca_mframe_version() == 1000 and _mframe_lib.ABI_MAJOR == 1 and lib.busca_mframe_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _mframe_lib
    lib = _mframe_lib.load()
    P, ODD = 0x10000, 0x10004                            # an aligned address, one that is 4- but not 8-byte aligned

    def calls(mean=P, cov=P, S=8, slot=P, nt=7, tlbr=P, xyah=P, score=P, cls=P + 1, mt=9, ft=4, prob=P, batch=2, N=4, M=5, out=P, status=P, r2c=P,
              c2r=P, thresh=0.7, free=P, new=P, dev=0):
        return {
            "busca_mframe_cost": lambda: lib.busca_mframe_cost(mean, cov, S, slot, nt, tlbr, score, cls, mt, ft, prob, batch, N, M, out, status, dev, None),
            "busca_mframe_apply": lambda: lib.busca_mframe_apply(mean, cov, S, slot, nt, r2c, c2r, xyah, score, cls, mt, thresh, free, ft, prob, batch,
                                                                 N, M, new, status, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_mframe_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    nothing = dict(mean=None, cov=None, slot=None, out=None, r2c=None, c2r=None, xyah=None, tlbr=None, cls=None, new=None, free=None, prob=None,
                   status=None, score=None)
    for name in calls():
        for noop in (dict(batch=0), dict(N=0, M=0), dict(nt=0, mt=0)):             # the no-ops, with and without pointers
            assert calls(**noop)[name]() == 0, (name, noop)
            assert calls(**noop, **nothing)[name]() == 0, (name, noop)
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", slot=None)
        refused(name, "null pointer", cls=None)
        refused(name, "null pointer (problems)", prob=None)
        for size in ("S", "nt", "mt", "ft", "batch", "N", "M"):
            refused(name, "negative size", **{size: -1})
        refused(name, "negative device", dev=-1)
        refused(name, "65535 at most", batch=65536)
        assert calls(batch=65535, N=0, M=0)[name]() == 0
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", cov=ODD)
        refused(name, "misaligned", score=ODD)
        refused(name, "misaligned", slot=0x10002)
        refused(name, "misaligned", prob=0x10002)
        refused(name, "misaligned", status=0x10002)
    name = "busca_mframe_cost"
    for noop in (dict(N=0), dict(M=0), dict(nt=0), dict(mt=0)):
        assert calls(**noop)[name]() == 0 and calls(**noop, **nothing)[name]() == 0, noop
    refused(name, "null pointer", tlbr=None)
    refused(name, "null pointer", out=None)
    refused(name, "misaligned", tlbr=ODD)
    refused(name, "misaligned", out=ODD)
    refused(name, "more workgroups than a grid holds", N=16 * 65535 + 1)
    assert calls(cov=None, score=None, status=None, batch=0)[name]() == 0
    name = "busca_mframe_apply"
    refused(name, "det_thresh is NaN", thresh=float("nan"))
    refused(name, "one problem takes 2048", M=2049)
    refused(name, "more workgroups than a grid holds", N=2 ** 31 - 1)
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
    # without rows the row operands may be NULL and without columns the column operands - but the others are still judged
    refused(name, "misaligned", N=0, slot=None, r2c=None, mean=ODD)
    refused(name, "misaligned", M=0, c2r=None, xyah=None, cls=None, new=None, free=None, mean=ODD)
    refused(name, "null pointer", nt=0, slot=None, r2c=None, new=None)
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_mframe_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_mframe_last_error() != b""


def test_python_level_checks():
    import sys
    import torch
    from busca_amd import _lib, _mframe_lib, tracking
    from busca_amd.kalman_store import FrameProblem, KalmanStore
    from tests.test_kalman_filter import _detections
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    import busca.tracking as alias
    assert tracking.FrameProblem is FrameProblem is alias.FrameProblem
    assert FrameProblem._fields == ("pool_slots", "lost", "unconfirmed_slots", "detections", "det_scores", "free_slots")
    st = KalmanStore(64)
    dets = _detections(np.array([[100.0, 100.0, 0.5, 80.0]] * 3))
    sc = [0.9, 0.3, 0.9]
    good = FrameProblem([1, 2], [0, 0], [3], dets, sc, [4, 5])
    other = dict(pool_slots=[11, 12], lost=[0, 0], unconfirmed_slots=[13], detections=dets, det_scores=sc, free_slots=[14])
    # what frame() checks, per problem, naming the problem
    for kw, words in ((dict(free_slots=[14, 12]), "problem 1.*also listed"), (dict(free_slots=[13]), "problem 1.*also listed"),
                      (dict(free_slots=[14, 15, 14]), "problem 1.*distinct"), (dict(unconfirmed_slots=[12]), "problem 1.*distinct"),
                      (dict(pool_slots=[11, 11]), "problem 1.*distinct"), (dict(free_slots=[-1]), "problem 1.*negative"),
                      (dict(pool_slots=[11, 64]), "problem 1.*beyond the capacity"), (dict(free_slots=[64]), "problem 1.*beyond the capacity"),
                      (dict(lost=[0]), "problem 1.*`lost` flags"), (dict(lost=[0, 0, 1]), "problem 1.*`lost` flags"),
                      (dict(det_scores=sc[:2]), "problem 1.*2 scores for 3 detections"), (dict(detections=torch.ones(3, 4)), "problem 1.*detection objects"),
                      (dict(pool_slots=torch.ones(2, dtype=torch.int32)), "problem 1.*host slot lists"),
                      # tracks and free slots distinct across the batch
                      (dict(pool_slots=[11, 2]), "distinct across the whole batch.*slot 2 "), (dict(unconfirmed_slots=[1]), "distinct across the whole batch"),
                      (dict(free_slots=[5]), "distinct across the whole batch.*slot 5 "), (dict(free_slots=[3]), "distinct across the whole batch"),
                      (dict(pool_slots=[4, 12]), "distinct across the whole batch")):
        with pytest.raises(ValueError, match=words):
            st.frame_batch([good, FrameProblem(**dict(other, **kw))], **THRESH)
    with pytest.raises(ValueError, match="problem 0.*also listed"):
        st.frame_batch([([1, 2], [0, 0], [3], dets, sc, [2]), FrameProblem(**other)], **THRESH)      # plain tuples are taken
    # sizes: the batch, and the rows and columns of one problem
    empty = FrameProblem([], [], [], [], [], [])
    with pytest.raises(ValueError, match="65536 problems, one call takes 65535"):
        st.frame_batch([empty] * 65536, **THRESH)
    assert _mframe_lib.MAX_BATCH == 65535
    big = KalmanStore(_lib.ASSIGN_MAX + 8)
    with pytest.raises(ValueError, match="problem 1.*at most %d rows and columns" % _lib.ASSIGN_MAX):
        big.frame_batch([empty, FrameProblem(list(range(_lib.ASSIGN_MAX + 1)), [0] * (_lib.ASSIGN_MAX + 1), [], dets, sc, [])], **THRESH)
    many = np.tile([[100.0, 100.0, 0.5, 80.0]], (min(_lib.ASSIGN_MAX, _mframe_lib.MAX_DETS) + 1, 1))
    with pytest.raises(ValueError, match="problem 0.*at most"):
        st.frame_batch([FrameProblem([1], [0], [], many, np.full(len(many), 0.9), [])], **THRESH)
    assert st.frame_batch([], **THRESH) == []
    assert st.mean is None and big.mean is None                                    # nothing was allocated


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def busy():
    from tests.test_streams_gpu import Busy
    b = Busy()
    yield b
    b.report()


class Batch:
    """Scenes in one store of 512: scene k's tracks and its free slots live in a range of a scattered permutation that no other scene shares."""

    def __init__(self, scenes, n_free=12):
        self.scenes = scenes
        n_free = [n_free] * len(scenes) if np.isscalar(n_free) else list(n_free)
        at, self.slots, self.free = 0, [], []
        for sc, f in zip(scenes, n_free):
            self.slots.append(PERM[at:at + sc.n].astype(np.int64))
            self.free.append(PERM[at + sc.n:at + sc.n + f].astype(np.int64))
            at += sc.n + f
        assert at <= CAP
        self.listed = np.concatenate(self.slots + self.free)

    def store(self):
        return _store(CAP, np.concatenate([sc.mean for sc in self.scenes]), np.concatenate([sc.cov for sc in self.scenes]), np.concatenate(self.slots))

    def pool(self, k):
        return self.slots[k][:self.scenes[k].n_pool]

    def unc(self, k):
        return self.slots[k][self.scenes[k].n_pool:]

    def problems(self):
        from busca_amd.kalman_store import FrameProblem
        return [FrameProblem(self.pool(k), sc.lost, self.unc(k), sc.dets, sc.scores, self.free[k]) for k, sc in enumerate(self.scenes)]

    def frames(self, st, **kw):
        """The reference: frame() once per problem."""
        return [st.frame(self.pool(k), sc.lost, self.unc(k), sc.dets, sc.scores, TRACK_THRESH, MATCH_THRESH, kw.pop("det_thresh", DET_THRESH),
                         free_slots=self.free[k], **kw) for k, sc in enumerate(self.scenes)]


def _plain(fr):
    return {f: [tuple(int(v) for v in x) if isinstance(x, tuple) else int(x) for x in getattr(fr, f)] for f in FIELDS}


def _same_frames(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert type(a).__name__ == type(b).__name__ == "ByteFrame"
        assert _plain(a) == _plain(b), (what, k, _plain(a), _plain(b))
        assert a.det_class.dtype == b.det_class.dtype and np.array_equal(a.det_class, b.det_class), (what, k)


def _same_state(a, b, what):
    x, y = _state_of(a), _state_of(b)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), what


def _agree(batch, what, **kw):
    """frame_batch() on one store, frame() per problem on a copy: the same frames, the same bits in every slot, the unlisted slots untouched."""
    a, b = batch.store(), batch.store()
    before = _state_of(a)
    got = a.frame_batch(batch.problems(), **THRESH, **kw)
    want = batch.frames(b, **kw)
    _same_frames(got, want, what)
    _same_state(a, b, what)
    _untouched(before, _state_of(a), batch.listed, what)
    return got


BATCHES = {
    "mixed": ([(1, 1), (15, 63), (16, 64), (17, 65), (40, 30)], [12, 12, 12, 2, 12]),       # the edges of the 16 x 64 tile, each at a non-zero begin
    "with_empties": ([(17, 65), (0, 9), (17, 0), (0, 0), (5, 20)], [2, 3, 4, 0, 12]),
    "single": ([(17, 65)], [2]),
}


def _batch(name):
    shapes, n_free = BATCHES[name]
    return Batch([Scene(n, m, 5 + n + 3 * k, n_unconfirmed=5 if (n, m) == (5, 20) else None) for k, (n, m) in enumerate(shapes)], n_free)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mot20", [("mixed", False), ("with_empties", False), ("single", False), ("mixed", True)])
def test_ragged_batches_equal_the_list_of_frames(name, mot20):
    batch = _batch(name)
    got = _agree(batch, (name, mot20), mot20=mot20)
    for f in FIELDS:                                                               # every list of the frame is exercised somewhere in the batch
        assert any(len(getattr(fr, f)) for fr in got), (name, f)
        print("%s mot20=%s %s: %s" % (name, mot20, f, [len(getattr(fr, f)) for fr in got]))
    if name == "with_empties":                                                     # what frame() gives for a problem without rows or columns
        assert _plain(got[1])["first"] == [] and got[1].new_tracks and _plain(got[3]) == {f: [] for f in FIELDS} and got[3].det_class.shape == (0,)
        sc = batch.scenes[2]
        assert got[2].unmatched_pool == [i for i in range(sc.n_pool) if not sc.lost[i]] + [i for i in range(sc.n_pool) if sc.lost[i]]
        assert got[2].unmatched_unconfirmed == list(range(sc.n_unc)) and got[4].unconfirmed and not got[4].first
    # apply=False: the same matches, and the states are only predicted
    a, b = batch.store(), batch.store()
    dry = a.frame_batch(batch.problems(), **THRESH, mot20=mot20, apply=False)
    for d, g in zip(dry, got):
        assert (d.first, d.second, d.unconfirmed, d.unmatched_pool, d.unmatched_unconfirmed) == (g.first, g.second, g.unconfirmed, g.unmatched_pool,
                                                                                                 g.unmatched_unconfirmed)
        assert d.new_tracks == [] and d.overflow == [] and np.array_equal(d.det_class, g.det_class)
    for k, sc in enumerate(batch.scenes):
        b.predict(batch.pool(k), sc.lost)
    _same_state(a, b, (name, "apply=False"))


@pytest.mark.gpu
def test_every_detection_list_empty():
    """Without any detection only the prediction happens, and nothing is copied home."""
    import torch
    batch = Batch([Scene(17, 0, 1), Scene(0, 0, 2), Scene(5, 0, 3)])
    seen = []
    orig = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (seen.append(1), orig(self, *a, **k))[1]
    try:
        a = batch.store()
        got = a.frame_batch(batch.problems(), **THRESH)
    finally:
        torch.Tensor.cpu = orig
    assert seen == []
    b = batch.store()
    _same_frames(got, batch.frames(b), "no detections")
    _same_state(a, b, "no detections")
    assert len(got[0].unmatched_pool) == 13 and got[0].unmatched_unconfirmed == [0, 1, 2, 3]


@pytest.mark.gpu
def test_ties():
    batch = Batch([Scene(17, 65, 3, tie=True), Scene(17, 65, 5 + 17), Scene(96, 40, 3, tie=True)], 8)
    st = batch.store()
    for k in (0, 2):                                         # the scenes do tie: columns of the slab that are equal, bit for bit
        sc = batch.scenes[k]
        cost = st.cost(batch.slots[k], sc.dets, sc.scores)[0].cpu().numpy()
        assert sum(np.array_equal(cost[:, j], cost[:, j + 1]) for j in range(sc.m - 1)) >= sc.m // 3
    got = _agree(batch, "ties")                              # pairs by exact integer equality with the per-problem frames
    for k in (0, 2):
        assert len(got[k].first) + len(got[k].second) + len(got[k].unconfirmed) >= 4


class Raw:
    """The operands of the two raw calls for a Batch: one slot list, one detection table, one free list and the problem table, on the device."""

    def __init__(self, batch, st):
        self.batch, self.st = batch, st
        sc = batch.scenes
        self.B = len(sc)
        self.n, self.m, self.f = [s.n for s in sc], [s.m for s in sc], [len(f) for f in batch.free]
        self.N, self.M = max(self.n), max(self.m)
        self.table = np.zeros((self.B, 6), dtype=np.int32)
        self.table[:, 1], self.table[:, 3], self.table[:, 5] = self.n, self.m, self.f
        self.table[1:, 0::2] = np.cumsum(self.table[:-1, 1::2], axis=0)
        self.totals = [int(sum(x)) for x in (self.n, self.m, self.f)]
        self.cls = [_classes(s.scores) for s in sc]
        self.slot = _dev(np.concatenate(batch.slots).astype(np.int32))
        self.free = _dev(np.concatenate(batch.free).astype(np.int32))
        self.det = st.detections_batch([s.dets for s in sc], [s.scores for s in sc])[0]
        self.d_cls = _dev(np.concatenate(self.cls))

    def cost(self, table, with_scores, guard=64, canary=777.25):
        """busca_mframe_cost into a canary slab with a guard band on both sides -> (slab [B, 2, N, M], status [B, N]); the guards are checked here."""
        import torch
        from busca_amd import _mframe_lib
        st, B, N, M = self.st, self.B, self.N, self.M
        buf = torch.full((B * 2 * N * M + 2 * guard,), canary, dtype=torch.float64, device=st.dev)
        status = torch.full((B * N + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        d_table = _dev(np.asarray(table, dtype=np.int32))
        _mframe_lib.check(_mframe_lib.load().busca_mframe_cost(
            st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, self.slot.data_ptr(), self.totals[0], self.det.tlbr.data_ptr(),
            self.det.score.data_ptr() if with_scores else None, self.d_cls.data_ptr(), self.totals[1], self.totals[2], d_table.data_ptr(), B, N, M,
            buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *st._where()))
        buf, status = buf.cpu().numpy(), status.cpu().numpy()
        assert (buf[:guard] == canary).all() and (buf[-guard:] == canary).all(), "written outside the slab"
        assert (status[:guard] == -7).all() and (status[-guard:] == -7).all(), "written outside the status words"
        return buf[guard:-guard].reshape(B, 2, N, M), status[guard:-guard].reshape(B, N)

    def apply(self, st, table, r2c, c2r, det_thresh=DET_THRESH, guard=16):
        """busca_mframe_apply on `st` with canary-filled new_slot and status -> (new_slot [B, M], status [B, N])."""
        import torch
        from busca_amd import _mframe_lib
        B, N, M = self.B, self.N, self.M
        new = torch.full((B * M + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        status = torch.full((B * N + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        d_table, d_r2c, d_c2r = (_dev(np.ascontiguousarray(x, dtype=np.int32)) for x in (table, r2c, c2r))
        _mframe_lib.check(_mframe_lib.load().busca_mframe_apply(
            st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, self.slot.data_ptr(), self.totals[0], d_r2c.data_ptr() if N else None, d_c2r.data_ptr(),
            self.det.xyah.data_ptr(), self.det.score.data_ptr(), self.d_cls.data_ptr(), self.totals[1], det_thresh,
            self.free.data_ptr() if self.totals[2] else None, self.totals[2], d_table.data_ptr(), B, N, M, new.data_ptr() + 4 * guard,
            status.data_ptr() + 4 * guard if N else None, *st._where()))
        new, status = new.cpu().numpy(), status.cpu().numpy()
        assert (new[:guard] == -7).all() and (new[-guard:] == -7).all() and (status[:guard] == -7).all() and (status[-guard:] == -7).all()
        return new[guard:-guard].reshape(B, M), status[guard:-guard].reshape(B, N)

    def bad_tables(self, k):
        """Problem k's row made one the table should not hold, one kind at a time."""
        n_total, m_total, f_total = self.totals
        for col, value, kind in ((0, -1, "negative row_begin"), (4, -3, "negative free_begin"), (0, n_total - self.n[k] + 1, "rows past n_total"),
                                 (2, m_total - self.m[k] + 1, "detections past m_total"), (4, f_total - self.f[k] + 1, "free slots past f_total"),
                                 (1, self.N + 1, "n_k > N"), (3, self.M + 1, "m_k > M")):
            t = self.table.copy()
            t[k, col] = value
            if kind in ("n_k > N", "m_k > M"):               # inside its list all the same: only the slab is too small for it
                t[k, col - 1] = 0
            yield kind, t


def _guarded(batch, guard=6, canary=777.25):
    """batch.store() with its tensors inside canary-filled buffers: guard rows behind the spare slot -> (store, mean buffer, cov buffer)."""
    import torch
    from busca_amd.kalman_store import KalmanStore
    src = batch.store()
    mean_buf = torch.full((CAP + 1 + guard, 8), canary, dtype=torch.float64, device=src.dev)
    cov_buf = torch.full((CAP + 1 + guard, 8, 8), canary, dtype=torch.float64, device=src.dev)
    mean_buf[:CAP + 1], cov_buf[:CAP + 1] = src.mean, src.cov
    st = KalmanStore(CAP)
    st._state()
    st.mean, st.cov = mean_buf[:CAP + 1], cov_buf[:CAP + 1]
    return st, mean_buf, cov_buf


@pytest.mark.gpu
def test_raw_cost_writes_the_valid_corners_and_nothing_else():
    batch = _batch("mixed")
    st = batch.store()
    raw = Raw(batch, st)
    assert raw.table[1:, 0].all() and raw.table[1:, 2].all() and raw.table[1:, 4].all()            # every begin but the first is non-zero
    want = {}
    for with_scores in (True, False):
        slab, status = raw.cost(raw.table, with_scores)
        for k, sc in enumerate(batch.scenes):
            n, m = sc.n, sc.m
            alone, _ = _raw_cost(st, _dev(batch.slots[k].astype(np.int32)), n, sc, raw.cls[k], with_scores)
            want[k, with_scores] = alone
            assert np.array_equal(slab[k, :, :n, :m], alone), (k, with_scores)
            assert (slab[k, :, n:, :] == 777.25).all() and (slab[k, :, :, m:] == 777.25).all(), (k, "padding written")
            assert (status[k, :n] == 0).all() and (status[k, n:] == -7).all(), k
    for k in (1, 4):
        for kind, table in raw.bad_tables(k):
            slab, status = raw.cost(table, True)
            assert (slab[k] == 777.25).all() and (status[k] == -7).all(), (kind, "the skipped problem was written")
            for o, sc in enumerate(batch.scenes):
                if o != k:
                    assert np.array_equal(slab[o, :, :sc.n, :sc.m], want[o, True]) and (status[o, :sc.n] == 0).all(), (kind, o)
                    assert (slab[o, :, sc.n:, :] == 777.25).all() and (slab[o, :, :, sc.m:] == 777.25).all() and (status[o, sc.n:] == -7).all()
    # a problem without rows or without detections has no tile: nothing of it is written
    batch = _batch("with_empties")
    st = batch.store()
    raw = Raw(batch, st)
    slab, status = raw.cost(raw.table, True)
    for k in (1, 2, 3):
        assert (slab[k] == 777.25).all() and (status[k] == -7).all(), k
    for k in (0, 4):
        sc = batch.scenes[k]
        assert np.array_equal(slab[k, :, :sc.n, :sc.m], _raw_cost(st, _dev(batch.slots[k].astype(np.int32)), sc.n, sc, raw.cls[k], True)[0])
        assert (status[k, :sc.n] == 0).all() and (status[k, sc.n:] == -7).all()


def _match_vectors(raw):
    """Match vectors the solver could have given: every third row of a problem matched, to scattered columns of its own problem."""
    r2c, c2r = np.full((raw.B, raw.N), -1, dtype=np.int32), np.full((raw.B, raw.M), -1, dtype=np.int32)
    for k in range(raw.B):
        for i in range(0, min(raw.n[k], raw.m[k]), 3):
            j = (5 * i + 1) % raw.m[k]
            if c2r[k, j] < 0:
                r2c[k, i], c2r[k, j] = j, i
    return r2c, c2r


@pytest.mark.gpu
def test_raw_apply_writes_its_problems_and_nothing_else():
    batch = _batch("mixed")
    raw = Raw(batch, batch.store())
    r2c, c2r = _match_vectors(raw)
    assert (r2c >= 0).sum() >= 20

    def alone(st, skip=None):
        """busca_frame_apply, problem by problem -> (new_slot, status) in the padded layout, -7 where nothing is written."""
        new, status = np.full((raw.B, raw.M), -7, dtype=np.int32), np.full((raw.B, raw.N), -7, dtype=np.int32)
        for k, sc in enumerate(batch.scenes):
            if k != skip:
                new[k, :sc.m], status[k, :sc.n] = _raw_apply(st, batch.slots[k], r2c[k, :sc.n], c2r[k, :sc.m], sc.xyah, sc.scores, raw.cls[k], DET_THRESH,
                                                             batch.free[k])
        return new, status

    cases = [("as it is", raw.table, None)] + [(kind, t, k) for k in (1, 3) for kind, t in raw.bad_tables(k)]
    for kind, table, skipped in cases:
        st, mean_buf, cov_buf = _guarded(batch)
        before = _state_of(st)
        new, status = raw.apply(st, table, r2c, c2r)
        ref = batch.store()
        want_new, want_status = alone(ref, skipped)
        assert np.array_equal(new, want_new) and np.array_equal(status, want_status), kind
        _same_state(st, ref, kind)
        assert (mean_buf[CAP + 1:] == 777.25).all() and (cov_buf[CAP + 1:] == 777.25).all(), (kind, "written behind the store")
        if skipped is None:
            assert (new >= 0).sum() >= 8 and (new == -2).sum() >= 1 and not status[status != -7].any()
            touched = [batch.slots[k][i] for k in range(raw.B) for i in range(raw.n[k]) if r2c[k, i] >= 0] + list(new[new >= 0])
            _untouched(before, _state_of(st), touched, kind)
        else:
            mine = np.concatenate([batch.slots[skipped], batch.free[skipped]])
            assert np.array_equal(_state_of(st)[0][mine], before[0][mine]) and np.array_equal(_state_of(st)[1][mine], before[1][mine]), kind


@pytest.mark.gpu
def test_initiation_ranks_per_problem():
    import torch
    from busca_amd import _mframe_lib
    from busca_amd.kalman_store import KalmanStore
    g = gold()
    S, GUARD, CANARY = 40, 6, 777.25
    ms = [150, 70, 3]
    B, M = 3, max(ms)
    # per problem: one entry beyond the capacity and one negative (skipped, and reported as listed); fewer free slots than starters; none; plenty
    frees = [np.array([5, 2, S + 3, 11, -4, 0, 7], dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([21, S, 20, -1, 23, 22], dtype=np.int32)]
    xyah, scores, c2r, eligible = [], [], np.full((B, M), -1, dtype=np.int32), []
    rs = np.random.RandomState(9)
    for k, m in enumerate(ms):
        xyah.append(g["init_meas"][(np.arange(m) + 11 * k) % 64])
        s = SCORES[(np.arange(m) + k) % 10].copy()
        s[::7] = 0.65                                        # first round, below det_thresh: starts nothing
        c2r[k, :m] = np.where(rs.uniform(size=m) < 0.4, 3, -1)       # matched columns scattered among the others
        if m == 3:                                           # the small problem: two starters around a matched column
            s, c2r[k, :m] = np.array([0.9, 0.8, 0.95]), [-1, 3, -1]
        scores.append(s)
        eligible.append([j for j in range(m) if c2r[k, j] < 0 and _classes(s)[j] == 0 and not s[j] < DET_THRESH])
    assert len(eligible[0]) > len(frees[0]) and eligible[0][-1] > 128 and len(eligible[1]) > 3 and 0 < len(eligible[2]) <= 3
    table = np.zeros((B, 6), dtype=np.int32)
    table[:, 3], table[:, 5] = ms, [len(f) for f in frees]
    table[1:, 0::2] = np.cumsum(table[:-1, 1::2], axis=0)
    d = [_dev(x) for x in (table, c2r, np.concatenate(xyah), np.concatenate(scores), np.concatenate([_classes(s) for s in scores]), np.concatenate(frees))]

    def run():
        mean_buf = torch.full((S + 1 + GUARD, 8), CANARY, dtype=torch.float64, device="cuda:0")
        cov_buf = torch.full((S + 1 + GUARD, 8, 8), CANARY, dtype=torch.float64, device="cuda:0")
        st = KalmanStore(S)
        st._state()
        new = torch.full((B * M + 32,), -7, dtype=torch.int32, device="cuda:0")
        _mframe_lib.check(_mframe_lib.load().busca_mframe_apply(
            mean_buf.data_ptr(), cov_buf.data_ptr(), S, None, 0, None, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), sum(ms),
            DET_THRESH, d[5].data_ptr(), sum(len(f) for f in frees), d[0].data_ptr(), B, 0, M, new.data_ptr() + 64, None, *st._where()))
        new = new.cpu().numpy()
        assert (new[:16] == -7).all() and (new[-16:] == -7).all()
        return new[16:-16].reshape(B, M), mean_buf.cpu().numpy(), cov_buf.cpu().numpy()
    new, mean, cov = run()
    want = np.full((B, M), -7, dtype=np.int32)               # the padding is not written
    ref = _store(S)
    taken = []
    for k, m in enumerate(ms):
        want[k, :m] = -1
        f = frees[k]
        want[k, eligible[k][:len(f)]] = f[:len(eligible[k])]      # slots are taken in ascending detection order, from the problem's own range
        want[k, eligible[k][len(f):]] = -2                        # the surplus: that problem's range is used up
        live = [r for r, s in enumerate(f[:len(eligible[k])]) if 0 <= s < S]
        ref.initiate(f[live], xyah[k], np.asarray(eligible[k])[live])
        taken += f[live].tolist()
    assert np.array_equal(new, want), (new, want)
    assert (new[0] == -2).sum() == len(eligible[0]) - 7 and (new[1] == -2).sum() == len(eligible[1]) and (new[2] == -2).sum() == 0
    assert sorted(taken) == [0, 2, 5, 7, 11] + sorted(int(s) for s in frees[2][:len(eligible[2])] if 0 <= s < S)
    rm, rc = _state_of(ref)
    assert np.array_equal(mean[taken], rm[taken]) and np.array_equal(cov[taken], rc[taken])
    rest = np.ones(S + 1 + GUARD, dtype=bool)
    rest[taken] = False
    assert (mean[rest] == CANARY).all() and (cov[rest] == CANARY).all()          # nothing else of the store or behind it was written
    again = run()
    assert np.array_equal(again[0], new) and np.array_equal(again[1], mean) and np.array_equal(again[2], cov)


@pytest.mark.gpu
def test_not_positive_definite_in_one_problem_of_three():
    from busca_amd.kalman_store import FrameProblem
    g = gold()
    slots = [[9, 2, 5], [19, 12, 15], [29, 22, 25]]
    means, covs, problems = [], [], []
    for k in range(3):
        idx = [4, 5, 6]                                       # the states of tests/test_byte_frame.py::test_not_positive_definite, three times
        mean, cov = g["mean"][idx].copy(), g["cov"][idx].copy()
        if k == 1:
            cov[1, :4, :4] = -np.eye(4)
        means.append(mean)
        covs.append(cov)
        # every detection on its track's prediction; a host array: measurements as they are
        problems.append(FrameProblem(slots[k], [False] * 3, [], mean[:, :4] + mean[:, 4:], [0.9] * 3, []))
    load = lambda: _store(32, np.concatenate(means), np.concatenate(covs), np.concatenate(slots))      # noqa: E731
    st, ref, kept = load(), load(), load()
    for k in range(3):
        kept.predict(slots[k], [False] * 3)
    with pytest.raises(np.linalg.LinAlgError, match="KalmanStore.frame_batch: problem 1: the projected covariance of track 1"):
        st.frame_batch(problems, **THRESH)
    for k, p in enumerate(problems):                          # frame() applies before it raises, too
        if k == 1:
            with pytest.raises(np.linalg.LinAlgError, match="KalmanStore.frame: the projected covariance of track 1"):
                ref.frame(p.pool_slots, p.lost, [], p.detections, p.det_scores, **THRESH)
        else:
            ref.frame(p.pool_slots, p.lost, [], p.detections, p.det_scores, **THRESH)
    _same_state(st, ref, "every other track is updated exactly as by frame()")
    got, pred = _state_of(st), _state_of(kept)
    assert np.array_equal(got[0][12], pred[0][12]) and np.array_equal(got[1][12], pred[1][12])      # the flagged one keeps its predicted state
    for s in (9, 2, 5, 19, 15, 29, 22, 25):
        assert not np.array_equal(got[1][s], pred[1][s]), s


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5])
def test_one_copy_home_after_the_filter_is_enqueued(B, monkeypatch):
    """Every route from a device tensor to the host is counted as tests/test_sort_frame.py counts them: one frame_batch() takes exactly one, whatever
    the number of problems, none has happened when busca_mframe_apply is enqueued, and every library entry point is called once."""
    import torch
    from busca_amd import _mframe_lib, geometry
    batch = _batch("mixed" if B == 5 else "single")
    assert len(batch.scenes) == B
    st, ref = batch.store(), batch.store()
    want = batch.frames(ref)
    count = {"n": 0, "at_apply": None}
    calls = {}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            to_host = name != "to" or any(str(x).startswith("cpu") for x in list(a) + list(k.values()) if isinstance(x, (str, torch.device)))
            if self.is_cuda and to_host:
                count["n"] += 1
            return orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("cpu", "item", "tolist", "numpy", "to"):
        counted(name)

    def wrapped(lib, name):
        real = getattr(lib, name)

        def f(*a):
            calls[name] = calls.get(name, 0) + 1
            if name == "busca_mframe_apply":
                count["at_apply"] = count["n"]
            return real(*a)
        monkeypatch.setattr(lib, name, f)
    wrapped(_mframe_lib.load(), "busca_mframe_cost")
    wrapped(_mframe_lib.load(), "busca_mframe_apply")
    wrapped(st._lib, "busca_track_kalman_predict")
    wrapped(geometry.default_context(0).lib, "busca_assign_stages")
    got = st.frame_batch(batch.problems(), **THRESH)
    copies = count["n"]
    monkeypatch.undo()
    assert count["at_apply"] == 0 and copies == 1
    assert calls == {"busca_track_kalman_predict": 1, "busca_mframe_cost": 1, "busca_assign_stages": 1, "busca_mframe_apply": 1}
    _same_frames(got, want, B)
    _same_state(st, ref, B)


@pytest.mark.gpu
def test_a_batch_behind_a_busy_stream(busy):
    from busca_amd.kalman_store import KalmanStore
    from tests.test_streams_gpu import behind
    batch = Batch([Scene(17, 65, 5 + 17), Scene(16, 64, 8), Scene(0, 9, 1)])
    other = Batch([Scene(17, 65, 99), Scene(16, 64, 98), Scene(0, 9, 1)])
    full = lambda b: [_dev(x) for x in _state_of(b.store())]      # noqa: E731
    st = KalmanStore(CAP)
    st._state()

    def call(x, outs, stream):
        st.mean, st.cov = x
        got = st.frame_batch(batch.problems(), **THRESH)
        return [np.asarray(v, dtype=np.int64) for fr in got for v in fr]
    want, got = behind(busy, "KalmanStore.frame_batch", call, true=full(batch), poison=full(other), form="current", host=True)
    assert len(got[2]) >= 4 and len(got[7]) >= 1 and len(got[2 + 16 + 5]) >= 1      # first-round matches and new tracks; the third problem starts tracks
    ref = batch.store()
    batch.frames(ref)
    assert np.array_equal(got[0], _state_of(ref)[0]) and np.array_equal(got[1], _state_of(ref)[1])


# ---- the reference's tracker, several sequences in lock step on one store ------------------------------------------------------------
class Hub:
    """One KalmanStore for several Replays: every replay runs in a thread of its own and all of them meet at a barrier once per time step, where
    the problems of the replays that are live in that step go out as ONE frame_batch."""

    def __init__(self, capacity, parties):
        from busca_amd.kalman_store import KalmanStore
        self.store = KalmanStore(capacity)
        self.store._state()
        self.lock = threading.Lock()                             # the store's other calls, one thread at a time
        self.pending, self.results, self.sizes = {}, {}, []
        self.barrier = threading.Barrier(parties, action=self._issue)

    def _issue(self):
        who = sorted(self.pending)
        self.results = {}
        if who:
            assert len({self.pending[w][1] for w in who}) == 1, "the replays of a batch share their parameters"
            frames = self.store.frame_batch([self.pending[w][0] for w in who], **dict(self.pending[who[0]][1]))
            self.results = dict(zip(who, frames))
            self.sizes.append(len(who))
        self.pending = {}

    def wait(self):
        self.barrier.wait(timeout=120)


class BatchBackend:
    """tests/byte_replay's backend contract on a range [base, base + capacity) of the hub's store; frame() is a problem of the step's batch."""

    def __init__(self, hub, base, capacity):
        self.hub, self.base, self.capacity = hub, base, capacity

    def _at(self, slots):
        return np.asarray(slots, dtype=np.int64).reshape(-1) + self.base

    def frame(self, pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh, free_slots=(), mot20=False):
        from busca_amd.kalman_store import FrameProblem
        params = (("track_thresh", track_thresh), ("match_thresh", match_thresh), ("det_thresh", det_thresh), ("mot20", mot20))
        self.hub.pending[self.base] = (FrameProblem(self._at(pool_slots), lost, self._at(unconfirmed_slots), detections, det_scores,
                                                    self._at(free_slots)), params)
        self.hub.wait()
        fr = self.hub.results[self.base]
        return fr._replace(new_tracks=[(j, s - self.base) for j, s in fr.new_tracks])

    def boxes(self, slots, tlbr=True):
        with self.hub.lock:
            return self.hub.store.boxes(self._at(slots), tlbr).cpu().numpy()

    def states(self, slots):
        import torch
        with self.hub.lock:
            rows = torch.from_numpy(self._at(slots)).to(self.hub.store.dev)
            return self.hub.store.mean.index_select(0, rows).cpu().numpy(), self.hub.store.cov.index_select(0, rows).cpu().numpy()

    def remove_duplicates(self, a, b):
        from busca_amd import tracking
        with self.hub.lock:
            return tracking.remove_duplicate_stracks(a, b)


def _lockstep(plan):
    """plan: [(scene, first time step)] -> (the batch sizes of the steps, per replay the held states after every frame).  Every frame of every
    replay is held against the recording with the fixture's bars, as tests/test_byte_tracker_replay.py holds KalmanStore.frame."""
    from tests import byte_replay as br
    from tests.test_byte_tracker_replay import bars
    scenes = [br.load_scene(name) for name, _ in plan]
    bases = np.concatenate([[0], np.cumsum([p["capacity"] for p, _ in scenes])])
    steps = max(start + p["frames"] for (_, start), (p, _) in zip(plan, scenes))
    hub = Hub(int(bases[-1]), len(plan))
    held, failed = [[] for _ in plan], []

    def run(k):
        (name, start), (p, frames) = plan[k], scenes[k]
        try:
            rp = br.Replay(BatchBackend(hub, int(bases[k]), p["capacity"]), p["track_thresh"], p["track_buffer"], p["match_thresh"], p["mot20"])
            err = {"mean": 0.0, "cov": 0.0}
            for t in range(steps):
                if not start <= t < start + p["frames"]:
                    hub.wait()                                   # not live in this step: no problem in its batch
                    continue
                f = t - start
                rp.step(frames[f]["det"])
                bad = br.compare_frame(rp, frames[f], f, err, *bars(name)[:2])
                assert bad is None, "%s (replay %d): %s" % (name, k, bad)
                held[k].append(rp.held())
        except BaseException as e:                               # noqa: B902  (the others must not wait for this one)
            failed.append((k, e))
            hub.barrier.abort()
    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(plan))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    first = [e for _, e in failed if not isinstance(e, threading.BrokenBarrierError)] or [e for _, e in failed]
    if first:
        raise first[0]
    return hub.sizes, held


def _one_by_one(plan):
    from tests import byte_replay as br
    held = []
    for name, _ in plan:
        seen = []
        bad, _, _ = br.replay_scene(name, br.DeviceBackend, on_frame=lambda rp, want, f: seen.append(rp.held()))
        assert bad is None, bad
        held.append(seen)
    return held


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [[("small", 0), ("crowded", 0), ("small", 7)], [("small_mot20", 0), ("small_mot20", 5)]], ids=["three", "mot20"])
def test_lockstep_replay_of_the_reference_tracker(plan):
    sizes, held = _lockstep(plan)
    if len(plan) == 3:
        assert sizes == [2] * 7 + [3] * 5 + [2] * 28 + [1] * 7, sizes         # crowded ends after 12 steps, the first small after 40
    else:
        assert sizes == [1] * 5 + [2] * 35 + [1] * 5, sizes
    alone = _one_by_one(plan)
    for k, (a, b) in enumerate(zip(held, alone)):
        assert len(a) == len(b) > 0
        for f, (x, y) in enumerate(zip(a, b)):
            assert all(np.array_equal(u, v) for u, v in zip(x, y)), (plan[k], f)
