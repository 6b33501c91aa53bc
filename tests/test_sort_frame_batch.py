"""The StrongSORT frames of many sequences on one store as one chain: libbusca_msframe.so (include/busca_msframe.h), its binding
busca_amd._msframe_lib and SortStore.frame_batch - one advance, busca_msframe_cost (which forms the appearance entries of its tiles itself),
busca_assign_stages over the batch, busca_msframe_apply and one copy home, whatever the number of sequences.

The oracle is SortStore.frame, once per problem, on a second store loaded alike (tests/test_sort_frame.py pins it to the composed route), and for
the raw calls busca_sframe_advance, busca_appearance_cost + busca_sframe_cost and busca_sframe_apply, problem by problem.  Everything is compared
with np.array_equal - every field of every SortFrame and the whole of mean, cov and feat of both stores -, the raw cost slabs by their bit patterns
(they hold NaN on purpose): no tolerance anywhere."""
import os
import re
import subprocess
import threading
import types

import numpy as np
import pytest

from tests.test_kalman_filter import r_initiate
from tests.test_sort_frame import ALPHA, CONFS, MATCH_THRESH, MAX_IOU, _all_of, _fstore, _raw_apply, _raw_cost, _same, tracked_states
from tests.test_sort_store import _dev, _xyah_of, euclidean_warps, tlwh_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 256
PERM = np.random.RandomState(23).permutation(CAP)
E = 64
FIELDS = ("matches", "unmatched_tracks", "unmatched_detections", "new_tracks", "overflow")
KW = dict(max_iou_distance=MAX_IOU, matching_threshold=MATCH_THRESH, ema_alpha=ALPHA)
CANARY = 777.25


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    import importlib
    builder = importlib.import_module("busca_amd.build")
    hip_lib = builder.build()
    from busca_amd import _frame_lib, _lib, _mframe_lib, _msframe_lib, _rounds_lib, _sframe_lib, _sort_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_msframe.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_msframe_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _msframe_lib.MSFRAME_API.items()}
    assert sorted(declared) == ["busca_msframe_advance", "busca_msframe_apply", "busca_msframe_cost", "busca_msframe_last_error", "busca_msframe_version"]
    assert (declared["busca_msframe_advance"], declared["busca_msframe_cost"], declared["busca_msframe_apply"]) == (15, 30, 25)
    for name, val in (("BUSCA_MSFRAME_MAX_DETS", _msframe_lib.MAX_DETS), ("BUSCA_MSFRAME_MAX_BATCH", _msframe_lib.MAX_BATCH),
                      ("BUSCA_MSFRAME_MC", _msframe_lib.MC), ("BUSCA_MSFRAME_CLAMP", _msframe_lib.CLAMP), ("BUSCA_MSFRAME_E_MIN", _msframe_lib.E_MIN),
                      ("BUSCA_MSFRAME_E_MAX", _msframe_lib.E_MAX)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val
    assert _msframe_lib.MAX_DETS == _sframe_lib.MAX_DETS and _msframe_lib.PROBLEM_WORDS == 7

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_msframe_lib.MSFRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_msframe_lib.MSFRAME_API)
    others = [hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH, _rounds_lib.ROUNDS_LIB_PATH, _sort_lib.SORT_LIB_PATH,
              _frame_lib.FRAME_LIB_PATH, _sframe_lib.SFRAME_LIB_PATH, _mframe_lib.MFRAME_LIB_PATH]
    assert os.path.basename(hip_lib) == "libbusca_hip.so" and len({os.path.basename(p) for p in others}) == 8
    for other in others:                                                           # the build leaves all nine libraries, and no other exports ours
        assert os.path.exists(other), other
        theirs = {n for n in exported(other) if not n.startswith("_")}
        assert not [n for n in theirs if n.startswith("busca_msframe")], other
        assert not (theirs & ours), other
    assert {n for n in exported(_sframe_lib.SFRAME_LIB_PATH) if not n.startswith("_")} == set(_sframe_lib.SFRAME_API)      # it keeps its exports
    assert "busca_msframe.h" not in _lib.HEADERS and "_msframe_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    assert builder.MSFRAME_OUT == _msframe_lib.MSFRAME_LIB_PATH and os.path.exists(builder.MSFRAME_OUT + ".flags")
    lib = _msframe_lib.load()
    assert lib.busca_msframe_version() == 1001 and _msframe_lib.ABI_MAJOR == 1 and lib.busca_msframe_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _msframe_lib
    lib = _msframe_lib.load()
    P, ODD = 0x10000, 0x10004                            # an aligned address, one that is 4- but not 8-byte aligned

    def calls(mean=P, cov=P, S=8, slot=P, nt=7, xyah=P, tlwh=P, dfeat=P, mt=9, ft=4, nm=2, mats=P, stale=P + 1, feat=P, E=64, gated=1e5, flags=3, lam=0.98,
              maxd=0.3, maxiou=0.7, first=P, again=P, depth=3, prob=P, batch=2, N=4, M=5, out=P, status=P, r2c=P, c2r=P, conf=P, alpha=0.9, free=P, new=P,
              dev=0):
        return {
            "busca_msframe_advance": lambda: lib.busca_msframe_advance(mean, cov, S, slot, nt, mt, ft, mats, nm, prob, batch, N, M, dev, None),
            "busca_msframe_cost": lambda: lib.busca_msframe_cost(mean, cov, S, slot, nt, xyah, tlwh, dfeat, mt, ft, nm, stale, feat, E, gated, flags, lam, maxd,
                                                                 maxiou, first, again, depth, prob, batch, N, M, out, status, dev, None),
            "busca_msframe_apply": lambda: lib.busca_msframe_apply(mean, cov, S, slot, nt, r2c, c2r, xyah, conf, dfeat, mt, feat, E, alpha, free, ft, nm, prob,
                                                                   batch, N, M, new, status, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_msframe_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    nothing = dict(mean=None, cov=None, slot=None, out=None, r2c=None, c2r=None, xyah=None, tlwh=None, dfeat=None, feat=None, new=None, free=None, prob=None,
                   status=None, conf=None, mats=None, stale=None, first=None, again=None)
    for name in calls():
        for noop in (dict(batch=0), dict(N=0, M=0), dict(nt=0, mt=0)):             # the no-ops, with and without pointers
            assert calls(**noop)[name]() == 0, (name, noop)
            assert calls(**noop, **nothing)[name]() == 0, (name, noop)
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", cov=None)
        refused(name, "null pointer", slot=None)
        refused(name, "null pointer (problems)", prob=None)
        for size in ("S", "nt", "mt", "ft", "nm", "batch", "N", "M"):
            refused(name, "negative size", **{size: -1})
        refused(name, "negative device", dev=-1)
        refused(name, "65535 at most", batch=65536)
        assert calls(batch=65535, N=0, M=0)[name]() == 0
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", cov=ODD)
        refused(name, "misaligned", slot=0x10002)
        refused(name, "misaligned", prob=0x10002)
    name = "busca_msframe_advance"
    for noop in (dict(N=0), dict(nt=0)):
        assert calls(**noop)[name]() == 0 and calls(**noop, **nothing)[name]() == 0, noop
    refused(name, "null pointer (matrices", mats=None)
    refused(name, "misaligned", mats=ODD)
    assert calls(mats=None, nm=0, batch=0)[name]() == 0
    name = "busca_msframe_cost"
    for noop in (dict(N=0), dict(M=0), dict(nt=0), dict(mt=0)):
        assert calls(**noop)[name]() == 0 and calls(**noop, **nothing)[name]() == 0, noop
    for ptr in ("xyah", "tlwh", "dfeat", "feat", "first", "out"):
        refused(name, "null pointer", **{ptr: None})
    for ptr in ("xyah", "tlwh", "out"):
        refused(name, "misaligned", **{ptr: ODD})
    for ptr in ("first", "again", "status"):
        refused(name, "misaligned", **{ptr: 0x10002})
    refused(name, "16 bytes for feat and det_feat", feat=ODD)
    refused(name, "16 bytes for feat and det_feat", dfeat=0x10008)
    refused(name, "negative size (depth", depth=-1)
    refused(name, "unknown flag bits", flags=4)
    refused(name, "mc_lambda is NaN", lam=float("nan"))
    refused(name, "max_distance is NaN", maxd=float("nan"))
    refused(name, "max_iou_distance is NaN", maxiou=float("nan"))
    for bad_e in (0, 8, 24, 2064, -16):
        refused(name, "multiple of 16", E=bad_e)
    refused(name, "more workgroups than a grid holds", N=16 * 65535 + 1)
    assert calls(flags=0, lam=float("nan"), maxd=float("nan"), batch=0)[name]() == 0       # a NaN that no flag reads
    name = "busca_msframe_apply"
    for noop in (dict(M=0), dict(mt=0)):
        assert calls(**noop)[name]() == 0 and calls(**noop, **nothing)[name]() == 0, noop
    refused(name, "alpha is NaN", alpha=float("nan"))
    refused(name, "one problem takes 2048", M=2049)
    refused(name, "more workgroups than a grid holds", N=2 ** 31 - 1)
    refused(name, "at least 1 value", E=0)
    for ptr in ("feat", "r2c", "c2r", "xyah", "dfeat", "new", "free"):
        refused(name, "null pointer", **{ptr: None})
    refused(name, "misaligned", xyah=ODD)
    refused(name, "misaligned", conf=ODD)
    for ptr in ("r2c", "c2r", "free", "new", "status", "feat", "dfeat"):
        refused(name, "misaligned", **{ptr: 0x10002})
    # without rows the row operands may be NULL - but the others are still judged
    refused(name, "misaligned", N=0, slot=None, r2c=None, mean=ODD)
    refused(name, "null pointer", nt=0, slot=None, r2c=None, new=None)
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_msframe_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_msframe_last_error() != b""


def test_python_level_checks():
    import sys
    import torch
    from busca_amd import _lib, _msframe_lib, tracking
    from busca_amd.sort_store import SortFrameProblem, SortStore
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    import busca.tracking as alias
    assert tracking.SortFrameProblem is SortFrameProblem is alias.SortFrameProblem
    assert SortFrameProblem._fields == ("slots", "time_since_update", "confirmed", "det_tlwh", "det_confidence", "det_features", "free_slots", "camera_matrix")
    assert SortFrameProblem([], [], [], [], None, []).free_slots == () and SortFrameProblem([], [], [], [], None, []).camera_matrix is None
    st = SortStore(64, feature_dim=E)
    boxes = np.array([[100.0, 100.0, 40.0, 80.0]] * 3)
    feats = np.ones((3, E), dtype=np.float32)
    good = SortFrameProblem([1, 2], [1, 1], [True, False], boxes, None, feats, [4, 5])
    other = dict(slots=[11, 12], time_since_update=[1, 2], confirmed=[True, True], det_tlwh=boxes, det_confidence=[0.5] * 3, det_features=feats,
                 free_slots=[14], camera_matrix=None)
    for kw, words in ((dict(free_slots=[14, 12]), "problem 1.*also listed"), (dict(slots=[11, 11]), "problem 1.*distinct"),
                      (dict(free_slots=[-1]), "problem 1.*negative"), (dict(slots=[11, 64]), "problem 1"), (dict(confirmed=[True]), "problem 1.*confirmed flags"),
                      (dict(det_confidence=[0.5]), "problem 1.*1 confidences for 3 detections"), (dict(det_tlwh=torch.ones(3, 4)), "problem 1.*host"),
                      (dict(slots=torch.ones(2, dtype=torch.int32)), "problem 1.*host slot lists"),
                      (dict(det_features=np.ones((3, E + 16), dtype=np.float32)), "problem 1.*features for 3 detections"),        # the wrong feature shape
                      (dict(det_features=np.ones((2, E), dtype=np.float32)), "problem 1.*features for 3 detections"),
                      (dict(camera_matrix=np.eye(2)), "problem 1.*3 x 3"), (dict(camera_matrix=torch.eye(3)), "problem 1.*host 3 x 3"),
                      # tracks and free slots distinct across the batch
                      (dict(slots=[11, 2]), "distinct across the whole batch.*slot 2 "), (dict(free_slots=[5]), "distinct across the whole batch.*slot 5 "),
                      (dict(slots=[4, 12]), "distinct across the whole batch"), (dict(free_slots=[1]), "distinct across the whole batch"),
                      # one feature table: host arrays or device tensors
                      (dict(det_features=torch.ones(3, E)), "problem 1: host and device det_features")):
        with pytest.raises(ValueError, match="SortStore.frame_batch: " + words if words.startswith("problem") else words):
            st.frame_batch([good, SortFrameProblem(**dict(other, **kw))], **KW)
    with pytest.raises(ValueError, match="problem 0.*also listed"):
        st.frame_batch([([1, 2], [1, 1], [True, False], boxes, None, feats, [2]), SortFrameProblem(**other)], **KW)      # plain tuples are taken
    with pytest.raises(ValueError, match="problem 1.*the camera update precedes the prediction"):
        st.frame_batch([good, SortFrameProblem(**dict(other, camera_matrix=np.eye(3)))], predict=False, **KW)
    with pytest.raises(ValueError, match="problem 0.*ema_alpha"):
        st.frame_batch([good], MAX_IOU, MATCH_THRESH, None)
    with pytest.raises(ValueError, match="problem 0.*a cascade of depth"):
        st.frame_batch([good], cascade_depth=_lib.ASSIGN_STAGES_MAX, **KW)
    with pytest.raises(ValueError, match="problem 0.*needs the feature rows"):
        SortStore(64).frame_batch([good], **KW)                                    # feature_dim=None
    with pytest.raises(ValueError, match="problem 0.*multiple of 16"):
        SortStore(64, feature_dim=24).frame_batch([good._replace(det_features=np.ones((3, 24), dtype=np.float32))], **KW)
    # sizes: the batch, and the rows and columns of one problem
    empty = SortFrameProblem([], [], [], np.zeros((0, 4)), None, np.zeros((0, E), dtype=np.float32))
    with pytest.raises(ValueError, match="65536 problems, one call takes 65535"):
        st.frame_batch([empty] * 65536, **KW)
    assert _msframe_lib.MAX_BATCH == 65535
    big = SortStore(_lib.ASSIGN_MAX + 8, feature_dim=E)
    n = _lib.ASSIGN_MAX + 1
    with pytest.raises(ValueError, match="problem 1.*at most %d rows and columns" % _lib.ASSIGN_MAX):
        big.frame_batch([empty, SortFrameProblem(list(range(n)), [1] * n, [True] * n, boxes, None, feats)], **KW)
    m = min(_lib.ASSIGN_MAX, _msframe_lib.MAX_DETS) + 1
    with pytest.raises(ValueError, match="problem 0.*at most"):
        st.frame_batch([SortFrameProblem([1], [1], [True], np.tile(boxes[:1], (m, 1)), None, np.ones((m, E), dtype=np.float32))], **KW)
    assert st.frame_batch([], **KW) == []
    assert st.mean is None and st.feat is None and big.mean is None                # nothing was allocated


# ---- GPU: helpers -----------------------------------------------------------------------------------------------------------
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


class Scene:
    """tests/test_sort_frame.Scene at a feature width of its own and with ages 1 .. 5: n tracks (tracked_states) with unit feature rows and m
    detections - most on the prediction of a track with that track's feature, every 11th with the opposite feature (the cascade rejects it, the IoU
    stage may take it), every 9th a newcomer far from every track.  A third of the tracks have age 1, the others 1 .. 5, so that a cascade of depth 3
    leaves some confirmed tracks out (first = -1); every fifth track is unconfirmed; the rows of age > 1 are stale.  `tie`: integer boxes, one
    covariance, features from a few axis vectors, detections in duplicate - whole columns of both planes equal."""

    def __init__(self, n, m, seed, E=E, tie=False, conf=True, matrix=None):
        rs = np.random.RandomState(seed)
        nn = max(n, 8)
        i = np.arange(nn)
        if tie:
            z0 = np.stack([150.0 + 60 * (i % 8), 200.0 + 160 * (i // 8), np.full(nn, 0.5), np.full(nn, 128.0)], 1)
            mean, cov = r_initiate(z0)
            F = np.eye(E)[i % 4] + np.eye(E)[4 + i % 3]
        else:
            mean, cov = tracked_states(nn)
            F = rs.normal(size=(nn, E))
        F = (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)
        self.n, self.m, self.E, self.matrix = n, m, E, matrix
        self.mean, self.cov, self.F = mean[:n], cov[:n], F[:n].copy()
        self.tsu = np.where(i % 3 == 0, 1, 1 + (i * 7) % 5)[:n]
        self.confirmed = (i % 5 != 4)[:n]
        j = np.arange(m)
        if tie:
            group = j // 2
            on = (group * 3) % nn
            xyah = mean[on, :4].copy()
            xyah[:, 0] += (group % 3 - 1) * 8.0
            feats = (np.eye(E)[on % 4] + np.eye(E)[4 + (on + group) % 3]).astype(np.float32)
        else:
            on = (j * 7) % nn
            pm = mean[on, :4] + mean[on, 4:]                              # where the prediction puts the track
            xyah = pm + rs.uniform(-1, 1, (m, 4)) * np.stack([0.02 * pm[:, 3], 0.02 * pm[:, 3], np.full(m, 0.004), 0.02 * pm[:, 3]], 1)
            feats = F[on] + rs.normal(scale=0.02, size=(m, E))
            feats[j % 11 == 3] *= -1
            far = j % 9 == 4
            xyah[far] = np.stack([3000.0 + 100 * j[far], 300.0 + 0 * j[far], 0.5 + 0 * j[far], 120.0 + 0 * j[far]], 1)
            feats[far] = rs.normal(size=(int(far.sum()), E))
            feats = (feats * rs.uniform(0.5, 3.0, (m, 1))).astype(np.float32)      # not normalised
        self.tlwh = tlwh_of(xyah)
        self.xyah = _xyah_of(self.tlwh)                                   # what every route derives from the boxes
        self.feats = feats
        self.conf = CONFS[j % 4] if conf else None


class Batch:
    """Scenes in one store of 256: scene k's tracks and its free slots live in a range of a scattered permutation that no other scene shares."""

    def __init__(self, scenes, n_free=6):
        self.scenes = scenes
        n_free = [n_free] * len(scenes) if np.isscalar(n_free) else list(n_free)
        at, self.slots, self.free = 0, [], []
        for sc, f in zip(scenes, n_free):
            self.slots.append(PERM[at:at + sc.n].astype(np.int64))
            self.free.append(PERM[at + sc.n:at + sc.n + f].astype(np.int64))
            at += sc.n + f
        assert at <= CAP and len({sc.E for sc in scenes}) == 1
        self.E = scenes[0].E
        self.listed = np.concatenate(self.slots + self.free)

    def store(self):
        sc = self.scenes
        return _fstore(np.concatenate([s.mean for s in sc]), np.concatenate([s.cov for s in sc]), np.concatenate(self.slots),
                       np.concatenate([s.F for s in sc]), capacity=CAP, E=self.E)

    def problems(self, device_features=False):
        from busca_amd.sort_store import SortFrameProblem
        return [SortFrameProblem(self.slots[k], sc.tsu, sc.confirmed, sc.tlwh, sc.conf, _dev(sc.feats) if device_features else sc.feats, self.free[k],
                                 sc.matrix) for k, sc in enumerate(self.scenes)]

    def frames(self, st, depth=None, lam=None, **kw):
        """The oracle: frame() once per problem."""
        return [st.frame(self.slots[k], sc.tsu, sc.confirmed, sc.tlwh, sc.conf, sc.feats, MAX_IOU, MATCH_THRESH, ALPHA, free_slots=self.free[k],
                         cascade_depth=depth, mc_lambda=lam, camera_matrix=sc.matrix, **kw) for k, sc in enumerate(self.scenes)]


def _plain(fr):
    return {f: [tuple(int(v) for v in x) if isinstance(x, tuple) else int(x) for x in getattr(fr, f)] for f in FIELDS}


def _same_frames(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert type(a).__name__ == type(b).__name__ == "SortFrame"
        assert _plain(a) == _plain(b), (what, k, _plain(a), _plain(b))


def _agree(batch, what, depth=None, lam=None, device_features=False, **kw):
    """frame_batch() on one store, frame() per problem on a copy: the same frames, the same bits in every slot of mean, cov and feat."""
    a, b = batch.store(), batch.store()
    before = _all_of(a)
    got = a.frame_batch(batch.problems(device_features), cascade_depth=depth, mc_lambda=lam, **KW, **kw)
    want = batch.frames(b, depth, lam, **kw)
    _same_frames(got, want, what)
    after = _all_of(a)
    _same(after, _all_of(b), what)
    keep = np.ones(CAP + 1, dtype=bool)
    keep[batch.listed] = False
    for x, y in zip(before, after):
        assert np.array_equal(x[keep], y[keep]), (what, "an unlisted slot was written")
    return got


# n_k in {0, 1, 15, 16, 17, 33} and m_k in {0, 1, 63, 64, 65}: the edges of the 16 x 64 tile, each at a non-zero begin
BATCHES = {
    "six": ([(1, 65), (15, 63), (16, 64), (17, 1), (33, 65), (0, 64)], [6, 6, 2, 6, 6, 3]),
    "three": ([(17, 0), (33, 64), (0, 1)], [4, 40, 0]),
    "single": ([(17, 65)], [2]),
    "small": ([(17, 65), (16, 64), (1, 1)], [6, 6, 6]),
}


def _batch(name, E=E):
    shapes, n_free = BATCHES[name]
    warps = euclidean_warps()
    # confidences in every other problem, a camera matrix on two of three
    return Batch([Scene(n, m, 5 + n + 3 * k, E=E, conf=k % 2 == 0, matrix=None if k % 3 == 1 else warps[k % 8]) for k, (n, m) in enumerate(shapes)], n_free)


@pytest.mark.gpu
@pytest.mark.parametrize("lam", [None, 0.98])
@pytest.mark.parametrize("depth", [None, 3])
@pytest.mark.parametrize("name", ["six", "three", "single"])
def test_ragged_batches_equal_the_list_of_frames(name, depth, lam):
    batch = _batch(name)
    got = _agree(batch, (name, depth, lam), depth, lam)
    for f in FIELDS:
        print("%s depth=%s lam=%s %s: %s" % (name, depth, lam, f, [len(getattr(fr, f)) for fr in got]))
    if name == "six":
        for f in FIELDS:                                                           # every list of the frame is exercised somewhere in the batch
            assert any(len(getattr(fr, f)) for fr in got), (name, f)
        assert got[5].matches == [] and len(got[5].new_tracks) == 3 and len(got[5].overflow) == 61       # no tracks: a track per detection
        if depth == 3:                                                             # confirmed tracks older than the cascade took part in nothing
            sc = batch.scenes[4]
            out = [i for i in range(sc.n) if sc.confirmed[i] and sc.tsu[i] > 3]
            assert out and set(out) <= set(got[4].unmatched_tracks)
        assert sum(len(fr.matches) for fr in got) >= 30
    if name == "three":
        assert _plain(got[0]) == dict(matches=[], unmatched_tracks=list(range(17)), unmatched_detections=[], new_tracks=[], overflow=[])
        assert got[2].overflow == [0] and len(got[1].matches) >= 10
    # apply=False: the same matches, and the states are only advanced
    a, b = batch.store(), batch.store()
    dry = a.frame_batch(batch.problems(), cascade_depth=depth, mc_lambda=lam, apply=False, **KW)
    for d, g in zip(dry, got):
        assert (d.matches, d.unmatched_tracks, d.unmatched_detections) == (g.matches, g.unmatched_tracks, g.unmatched_detections)
        assert d.new_tracks == [] and d.overflow == []
    _same_frames(dry, batch.frames(b, depth, lam, apply=False), (name, "apply=False"))
    _same(_all_of(a), _all_of(b), (name, "apply=False"))


@pytest.mark.gpu
@pytest.mark.parametrize("width", [16, 512])
def test_other_feature_widths(width):
    got = _agree(_batch("small", E=width), ("width", width), 3, 0.98)
    assert len(got[0].matches) >= 6 and got[0].new_tracks


@pytest.mark.gpu
def test_device_features_and_confidence_zero_is_null():
    """Device tensors take one torch.cat and give the same bits; a batch whose problems all give no confidence (NULL in the kernel) equals the batch
    that spells the zeros out, and both equal frame() with det_confidence=None."""
    batch = _batch("small")
    _agree(batch, "device features", 3, None, device_features=True)
    for sc in batch.scenes:
        sc.conf = None
    a, b = batch.store(), batch.store()
    got = a.frame_batch(batch.problems(), cascade_depth=3, **KW)                    # no problem has confidences: det_conf = NULL
    want = batch.frames(b, 3)
    batch.scenes[1].conf = np.zeros(batch.scenes[1].m)                              # one does: the others contribute zeros
    c = batch.store()
    zeros = c.frame_batch(batch.problems(), cascade_depth=3, **KW)
    _same_frames(got, want, "NULL")
    _same_frames(zeros, want, "zeros")
    _same(_all_of(a), _all_of(b), "NULL")
    _same(_all_of(c), _all_of(b), "zeros")
    assert sum(len(fr.matches) for fr in got) >= 10


@pytest.mark.gpu
def test_a_feature_row_never_written_matches_nothing():
    batch = _batch("small")
    sc = batch.scenes[0]
    row = 1                                                                        # a confirmed track of age 2: the cascade is its only stage
    sc.tsu = sc.tsu.copy()
    sc.tsu[row] = 2
    assert sc.confirmed[row] and (7 * np.arange(sc.m) % 17 == row).any()           # and detections sit on it
    sc.F[row] = 0.0
    got = _agree(batch, "zero row", 3, None)
    assert row in got[0].unmatched_tracks
    sc.F[row] = Scene(17, 65, 5 + 17).F[row]                                       # with its feature it is matched
    assert row not in _agree(batch, "with its row", 3, None)[0].unmatched_tracks


@pytest.mark.gpu
def test_every_detection_list_empty():
    """Without any detection only the advance happens, and nothing is copied home."""
    import torch
    warps = euclidean_warps()
    batch = Batch([Scene(17, 0, 1, matrix=warps[0]), Scene(0, 0, 2), Scene(5, 0, 3)])
    seen = []
    orig = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (seen.append(1), orig(self, *a, **k))[1]
    try:
        a = batch.store()
        got = a.frame_batch(batch.problems(), cascade_depth=3, **KW)
    finally:
        torch.Tensor.cpu = orig
    assert seen == []
    b = batch.store()
    _same_frames(got, batch.frames(b, 3), "no detections")
    _same(_all_of(a), _all_of(b), "no detections")
    assert got[0].unmatched_tracks == list(range(17)) and got[1].unmatched_tracks == []
    c = batch.store()
    assert not np.array_equal(_all_of(c)[0][batch.slots[0]], _all_of(a)[0][batch.slots[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [3, None])
def test_ties(depth):
    batch = Batch([Scene(17, 40, 3, tie=True), Scene(17, 65, 5 + 17), Scene(33, 40, 3, tie=True)], 8)
    for k in (0, 2):                                         # the scenes do tie: detections and feature rows in duplicate
        sc = batch.scenes[k]
        assert sum(np.array_equal(sc.tlwh[j], sc.tlwh[j + 1]) and np.array_equal(sc.feats[j], sc.feats[j + 1]) for j in range(sc.m - 1)) >= sc.m // 3
        assert len(np.unique(sc.F, axis=0)) < sc.n
    got = _agree(batch, ("ties", depth), depth)              # pairs by exact integer equality with the per-problem frames
    for k in (0, 2):
        assert len(got[k].matches) >= 6 and got[k].new_tracks


# ---- GPU: the three raw calls -------------------------------------------------------------------------------------------------
class Raw:
    """The operands of the three raw calls for a Batch: one slot list, the detection tables, one free list, the matrices and the problem table."""
    DEPTH = 3

    def __init__(self, batch, st, shift=0):
        self.batch, self.st = batch, st
        sc = batch.scenes
        self.B = len(sc)
        self.n, self.m, self.f = [s.n for s in sc], [s.m for s in sc], [len(f) for f in batch.free]
        self.N, self.M = max(self.n), max(self.m)
        self.with_matrix = [k for k, s in enumerate(sc) if s.matrix is not None]
        self.table = np.zeros((self.B, 7), dtype=np.int32)
        self.table[:, 1], self.table[:, 3], self.table[:, 5], self.table[:, 6] = self.n, self.m, self.f, -1
        self.table[1:, 0:6:2] = np.cumsum(self.table[:-1, 1:6:2], axis=0)
        self.table[self.with_matrix, 6] = np.arange(len(self.with_matrix))
        self.totals = [int(sum(x)) for x in (self.n, self.m, self.f)]
        # rows in turn: plane 0 only (a cascade level), plane 1 only (unconfirmed), both (age 1), neither (older than the cascade)
        self.first, self.again, self.stale = [], [], []
        for k, n in enumerate(self.n):
            kind = (np.arange(n) + shift + k) % 4
            self.first.append(np.select([kind == 0, kind == 1, kind == 2], [np.arange(n) % self.DEPTH, self.DEPTH, 0], -1).astype(np.int32))
            self.again.append(np.where(kind == 2, self.DEPTH, -1).astype(np.int32))
            self.stale.append(np.arange(n) % 5 == 3)
        cat = lambda xs, dt: _dev(np.concatenate(xs).astype(dt))      # noqa: E731
        self.slot = cat(batch.slots, np.int32)
        self.free = cat(batch.free, np.int32) if self.totals[2] else None
        self.d_first, self.d_again, self.d_stale = cat(self.first, np.int32), cat(self.again, np.int32), cat(self.stale, np.uint8)
        self.xyah, self.tlwh = cat([s.xyah for s in sc], np.float64), cat([s.tlwh for s in sc], np.float64)
        self.conf = cat([np.zeros(s.m) if s.conf is None else s.conf for s in sc], np.float64)
        self.feats = cat([s.feats for s in sc], np.float32)
        self.mats = cat([sc[k].matrix.reshape(-1) for k in self.with_matrix], np.float64) if self.with_matrix else None

    def sizes(self):
        return self.totals[1], self.totals[2], len(self.with_matrix)

    def advance(self, st, table):
        from busca_amd import _msframe_lib
        d_table = _dev(np.asarray(table, dtype=np.int32))
        m_total, f_total, n_mat = self.sizes()
        _msframe_lib.check(_msframe_lib.load().busca_msframe_advance(st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, self.slot.data_ptr(), self.totals[0],
                                                                     m_total, f_total, None if self.mats is None else self.mats.data_ptr(), n_mat,
                                                                     d_table.data_ptr(), self.B, self.N, self.M, *st._where()))

    def cost(self, table, lam, gated=1e5, guard=64):
        """busca_msframe_cost into a canary slab with a guard band on both sides -> (slab [B, 2, N, M], status [B, N]); the guards are checked here."""
        import torch
        from busca_amd import _msframe_lib
        st, B, N, M = self.st, self.B, self.N, self.M
        buf = torch.full((B * 2 * N * M + 2 * guard,), CANARY, dtype=torch.float64, device=st.dev)
        status = torch.full((B * N + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        d_table = _dev(np.asarray(table, dtype=np.int32))
        m_total, f_total, n_mat = self.sizes()
        _msframe_lib.check(_msframe_lib.load().busca_msframe_cost(
            st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, self.slot.data_ptr(), self.totals[0], self.xyah.data_ptr(), self.tlwh.data_ptr(),
            self.feats.data_ptr(), m_total, f_total, n_mat, self.d_stale.data_ptr(), st.feat.data_ptr(), st.feature_dim, gated,
            (_msframe_lib.MC if lam is not None else 0) | _msframe_lib.CLAMP, 0.0 if lam is None else lam, MATCH_THRESH, MAX_IOU, self.d_first.data_ptr(),
            self.d_again.data_ptr(), self.DEPTH, d_table.data_ptr(), B, N, M, buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *st._where()))
        buf, status = buf.cpu().numpy(), status.cpu().numpy()
        assert (buf[:guard] == CANARY).all() and (buf[-guard:] == CANARY).all(), "written outside the slab"
        assert (status[:guard] == -7).all() and (status[-guard:] == -7).all(), "written outside the status words"
        return buf[guard:-guard].reshape(B, 2, N, M), status[guard:-guard].reshape(B, N)

    def alone(self, k, lam, ctx, gated=1e5):
        """busca_appearance_cost and busca_sframe_cost for problem k alone -> (slab [2, n_k, m_k], status [n_k])."""
        from busca_amd.appearance import appearance_cost
        st, sc = self.st, self.batch.scenes[k]
        slot = self.batch.slots[k].astype(np.int32)
        cost = appearance_cost(st.feat.view(st.capacity + 1, 1, -1), _dev(sc.feats), "min", slot=slot, ctx=ctx).cpu().numpy()
        return _raw_cost(st, _dev(slot), sc.xyah, sc.tlwh, self.stale[k], cost, sc.m, gated, lam, self.first[k], self.again[k], self.DEPTH)

    def apply(self, st, table, r2c, c2r, with_conf=True, guard=16):
        """busca_msframe_apply on `st` with canary-filled new_slot and status -> (new_slot [B, M], status [B, N])."""
        import torch
        from busca_amd import _msframe_lib
        B, N, M = self.B, self.N, self.M
        new = torch.full((B * M + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        status = torch.full((B * N + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
        d_table, d_r2c, d_c2r = (_dev(np.ascontiguousarray(x, dtype=np.int32)) for x in (table, r2c, c2r))
        m_total, f_total, n_mat = self.sizes()
        _msframe_lib.check(_msframe_lib.load().busca_msframe_apply(
            st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, self.slot.data_ptr(), self.totals[0], d_r2c.data_ptr(), d_c2r.data_ptr(),
            self.xyah.data_ptr(), self.conf.data_ptr() if with_conf else None, self.feats.data_ptr(), m_total, st.feat.data_ptr(), st.feature_dim, ALPHA,
            None if self.free is None else self.free.data_ptr(), f_total, n_mat, d_table.data_ptr(), B, N, M, new.data_ptr() + 4 * guard,
            status.data_ptr() + 4 * guard, *st._where()))
        new, status = new.cpu().numpy(), status.cpu().numpy()
        assert (new[:guard] == -7).all() and (new[-guard:] == -7).all() and (status[:guard] == -7).all() and (status[-guard:] == -7).all()
        return new[guard:-guard].reshape(B, M), status[guard:-guard].reshape(B, N)

    def bad_tables(self, k):
        """Problem k's row made one the table should not hold, one kind at a time."""
        n_total, m_total, f_total = self.totals
        for col, value, kind in ((0, -1, "negative row_begin"), (1, -2, "negative n_k"), (4, -3, "negative free_begin"),
                                 (0, n_total - self.n[k] + 1, "rows past n_total"), (2, m_total - self.m[k] + 1, "detections past m_total"),
                                 (4, f_total - self.f[k] + 1, "free slots past f_total"), (1, self.N + 1, "n_k > N"), (3, self.M + 1, "m_k > M"),
                                 (6, len(self.with_matrix), "matrix_k >= n_matrices"), (6, -2, "matrix_k < -1")):
            t = self.table.copy()
            t[k, col] = value
            if kind in ("n_k > N", "m_k > M"):               # inside its list all the same: only the slab is too small for it
                t[k, col - 1] = 0
            yield kind, t


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _guarded(batch, guard=6):
    """batch.store() with its tensors inside canary-filled buffers: guard rows behind the spare slot -> (store, the three buffers)."""
    import torch
    src = batch.store()
    bufs = [torch.full((CAP + 1 + guard,) + tuple(t.shape[1:]), CANARY, dtype=t.dtype, device=src.dev) for t in (src.mean, src.cov, src.feat)]
    for buf, t in zip(bufs, (src.mean, src.cov, src.feat)):
        buf[:CAP + 1] = t
    src.mean, src.cov, src.feat = (buf[:CAP + 1] for buf in bufs)
    return src, bufs


def _guards_intact(bufs, what):
    for buf in bufs:
        assert (buf[CAP + 1:] == CANARY).all(), (what, "written behind the store")


@pytest.mark.gpu
def test_raw_cost_writes_the_valid_corners_and_nothing_else(ctx):
    import torch
    batch = _batch("six")
    # a skipped slot, a slot beyond the capacity, a covariance that is not positive definite and a feature row never written, in rows of several kinds
    batch.slots[4][[2, 9]] = -1, CAP
    batch.scenes[4].cov = batch.scenes[4].cov.copy()
    batch.scenes[4].cov[[4, 8], :4, :4] = -np.eye(4)
    batch.scenes[4].F[[12, 16]] = 0.0
    st = batch.store()
    assert not st.feat[CAP].any()
    raw = Raw(batch, st)
    assert raw.table[1:, 0].all() and raw.table[1:, 2].all() and raw.table[1:, 4].all()            # every begin but the first is non-zero
    want = {}
    seen = {"nan": 0, "status": 0, "both": 0, "inf0": 0, "inf1": 0}
    for lam in (None, 0.98):
        for shift in (0, 1):
            raw = Raw(batch, st, shift)
            slab, status = raw.cost(raw.table, lam)
            for k, sc in enumerate(batch.scenes):
                n, m = sc.n, sc.m
                if n == 0 or m == 0:
                    assert (slab[k] == CANARY).all() and (status[k] == -7).all(), (k, "a problem without a tile was written")
                    continue
                alone, alone_status = raw.alone(k, lam, ctx)
                want[k, lam, shift] = alone, alone_status
                assert np.array_equal(_bits(slab[k, :, :n, :m]), _bits(alone)), (k, lam, shift)
                assert (slab[k, :, n:, :] == CANARY).all() and (slab[k, :, :, m:] == CANARY).all(), (k, "padding written")
                assert np.array_equal(status[k, :n], alone_status) and (status[k, n:] == -7).all(), k
                seen["nan"] += int(np.isnan(alone[0]).sum())
                seen["status"] += int(alone_status.sum())
                finite = np.isfinite(alone)
                seen["both"] += int((finite[0].any(1) & finite[1].any(1)).sum())
                seen["inf0"] += int(np.isposinf(alone[0]).all(1).sum())
                seen["inf1"] += int(np.isposinf(alone[1]).all(1).sum())
    assert all(seen.values()), seen            # NaN rows (the zero feature, the bad covariance), flagged rows, rows in both planes, in one, in neither
    raw = Raw(batch, st, 0)
    for k in (1, 4):
        for kind, table in raw.bad_tables(k):
            slab, status = raw.cost(table, 0.98)
            assert (slab[k] == CANARY).all() and (status[k] == -7).all(), (kind, "the skipped problem was written")
            for o, sc in enumerate(batch.scenes):
                if o != k and sc.n and sc.m:
                    assert np.array_equal(_bits(slab[o, :, :sc.n, :sc.m]), _bits(want[o, 0.98, 0][0])), (kind, o)
                    assert np.array_equal(status[o, :sc.n], want[o, 0.98, 0][1]) and (status[o, sc.n:] == -7).all(), (kind, o)
                    assert (slab[o, :, sc.n:, :] == CANARY).all() and (slab[o, :, :, sc.m:] == CANARY).all(), (kind, o)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_raw_advance_writes_its_problems_and_nothing_else():
    from busca_amd import _sframe_lib
    batch = _batch("six")
    batch.slots[4][[2, 9]] = -1, CAP
    raw = Raw(batch, batch.store())
    assert raw.with_matrix == [0, 2, 3, 5]
    cases = [("as it is", raw.table, None)] + [(kind, t, k) for k in (1, 4) for kind, t in raw.bad_tables(k)]
    for kind, table, skipped in cases:
        st, bufs = _guarded(batch)
        before = _all_of(st)
        raw.advance(st, table)
        ref = batch.store()
        for k, sc in enumerate(batch.scenes):
            if k != skipped and sc.n:
                mat = None if sc.matrix is None else _dev(sc.matrix)
                slot = _dev(batch.slots[k].astype(np.int32))
                _sframe_lib.check(_sframe_lib.load().busca_sframe_advance(ref.mean.data_ptr(), ref.cov.data_ptr(), CAP, slot.data_ptr(), sc.n,
                                                                          None if mat is None else mat.data_ptr(), *ref._where()))
        after = _all_of(st)
        _same(after, _all_of(ref), kind)
        _guards_intact(bufs, kind)
        moved = np.concatenate([batch.slots[k] for k in range(raw.B) if k != skipped])
        moved = moved[(moved >= 0) & (moved < CAP)]
        assert all(not np.array_equal(after[1][s], before[1][s]) for s in moved), kind
        keep = np.ones(CAP + 1, dtype=bool)
        keep[moved] = False
        assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(before, after)), kind
    # the warp did something: a problem with a matrix does not hold the plainly predicted means
    plain = batch.store()
    plain.predict(batch.slots[0])
    assert not np.array_equal(_all_of(plain)[0][batch.slots[0], :4], after[0][batch.slots[0], :4])


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
@pytest.mark.parametrize("with_conf", [True, False])
def test_raw_apply_writes_its_problems_and_nothing_else(with_conf):
    # free lists that hold skipped entries (a negative one, one beyond the capacity), that run short, that are empty, that are plentiful
    batch = _batch("six")
    batch = Batch(batch.scenes, [6, 6, 2, 6, 0, 70])
    batch.free[0][[1, 3]] = -4, CAP + 3
    batch.slots[4][[0, 9]] = -1, CAP
    raw = Raw(batch, batch.store())
    r2c, c2r = _match_vectors(raw)
    assert (r2c >= 0).sum() >= 20 and r2c[4, 0] >= 0 and r2c[4, 9] >= 0            # the skipped slots are matched rows

    def alone(st, skip=None):
        """busca_sframe_apply, problem by problem -> (new_slot, status) in the padded layout, -7 where nothing is written."""
        new, status = np.full((raw.B, raw.M), -7, dtype=np.int32), np.full((raw.B, raw.N), -7, dtype=np.int32)
        for k, sc in enumerate(batch.scenes):
            if k != skip and sc.m:
                conf = (np.zeros(sc.m) if sc.conf is None else sc.conf) if with_conf else None
                new[k, :sc.m], status[k, :sc.n] = _raw_apply(st, batch.slots[k], r2c[k, :sc.n], c2r[k, :sc.m], sc.xyah, conf, sc.feats, ALPHA, batch.free[k])
        return new, status

    cases = [("as it is", raw.table, None)] + [(kind, t, k) for k in (0, 4) for kind, t in raw.bad_tables(k)]
    for kind, table, skipped in cases:
        st, bufs = _guarded(batch)
        before = _all_of(st)
        new, status = raw.apply(st, table, r2c, c2r, with_conf)
        ref = batch.store()
        want_new, want_status = alone(ref, skipped)
        assert np.array_equal(new, want_new) and np.array_equal(status, want_status), kind
        after = _all_of(st)
        _same(after, _all_of(ref), kind)
        _guards_intact(bufs, kind)
        if skipped is None:
            # initiation ranks are per problem: each takes from its own range, in ascending detection order, -2 once the range is used up
            for k, sc in enumerate(batch.scenes):
                starters = [j for j in range(sc.m) if c2r[k, j] < 0]
                f = batch.free[k]
                assert list(new[k, starters[:len(f)]]) == list(f[:len(starters)]) and (new[k, starters[len(f):]] == -2).all(), k
                assert (new[k, [j for j in range(sc.m) if c2r[k, j] >= 0]] == -1).all(), k
            assert (new[2] == -2).sum() == 64 - int((c2r[2] >= 0).sum()) - 2 and (new[4] == -2).sum() == 65 - int((c2r[4] >= 0).sum()) >= 50
            assert (new[5, :64] >= 0).sum() == 64
            assert -4 in new[0] and CAP + 3 in new[0]                              # reported as listed, and skipped
            assert not status[status != -7].any()
            touched = [batch.slots[k][i] for k in range(raw.B) for i in range(raw.n[k]) if r2c[k, i] >= 0] + list(new[new >= 0])
            touched = [s for s in touched if 0 <= s < CAP]
            keep = np.ones(CAP + 1, dtype=bool)
            keep[touched] = False
            assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(before, after)), kind
            assert all(not np.array_equal(before[2][s], after[2][s]) for s in touched), kind
        else:
            mine = np.concatenate([batch.slots[skipped], batch.free[skipped]])
            mine = mine[(mine >= 0) & (mine < CAP)]
            assert all(np.array_equal(x[mine], y[mine]) for x, y in zip(before, after)), kind


# ---- GPU: the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_not_positive_definite_in_one_problem_of_three():
    import torch
    scenes = [Scene(17, 20, 2 + k) for k in range(3)]
    for sc in scenes:
        sc.tsu = np.ones(17, dtype=np.int64)
    batch = Batch(scenes, 4)
    bad_conf, bad_unc = 3, 4                                       # a confirmed row (gated) and an unconfirmed one (not gated)
    assert scenes[1].confirmed[bad_conf] and not scenes[1].confirmed[bad_unc]
    neg = lambda st, row: st.cov.__setitem__((int(batch.slots[1][row]), slice(0, 4), slice(0, 4)), -torch.eye(4, dtype=torch.float64, device=st.dev))      # noqa: E731

    def one_by_one(ref, words, **kw):
        for k, sc in enumerate(scenes):                            # frame() applies before it raises, too
            call = lambda: ref.frame(batch.slots[k], sc.tsu, sc.confirmed, sc.tlwh, sc.conf, sc.feats, MAX_IOU, MATCH_THRESH, ALPHA,       # noqa: E731
                                     free_slots=batch.free[k], cascade_depth=30, predict=False, **kw)
            if k == 1:
                with pytest.raises(np.linalg.LinAlgError, match=words):
                    call()
            else:
                call()
    # at a gated row: the gate never sees the unconfirmed track, but it does see the confirmed one
    st, ref = batch.store(), batch.store()
    neg(st, bad_unc)
    neg(ref, bad_unc)
    assert st.frame_batch(batch.problems(), cascade_depth=30, predict=False, apply=False, **KW)[1].matches
    neg(st, bad_conf)
    neg(ref, bad_conf)
    before = _all_of(st)
    with pytest.raises(np.linalg.LinAlgError, match="SortStore.frame_batch: problem 1: the projected covariance of track 3"):
        st.frame_batch(batch.problems(), cascade_depth=30, predict=False, **KW)
    one_by_one(ref, "SortStore.frame: the projected covariance of track 3")
    after = _all_of(st)
    _same(after, _all_of(ref), "a gated row")                      # the whole batch was applied, as the frames one by one
    for k in (0, 2):
        assert not np.array_equal(after[1][batch.slots[k][0]], before[1][batch.slots[k][0]])
    # at an update: the unconfirmed track is matched by the IoU stage (which reads only its mean), its update is flagged
    st, ref = batch.store(), batch.store()
    for s in (st, ref):
        for k in range(3):
            s.predict(batch.slots[k])
        neg(s, bad_unc)
    before = _all_of(st)
    with pytest.raises(np.linalg.LinAlgError, match="SortStore.frame_batch: problem 1: update: the projected covariance of track 4"):
        st.frame_batch(batch.problems(), cascade_depth=30, predict=False, **KW)
    one_by_one(ref, "SortStore.frame: update: the projected covariance of track 4")
    after = _all_of(st)
    _same(after, _all_of(ref), "an update")
    s = int(batch.slots[1][bad_unc])                               # that slot keeps its Kalman state, its feature row is smoothed all the same
    assert np.array_equal(after[0][s], before[0][s]) and np.array_equal(after[1][s], before[1][s]) and not np.array_equal(after[2][s], before[2][s])
    for k in range(3):                                             # the other two problems, and the other tracks of this one, were updated
        assert not np.array_equal(after[1][int(batch.slots[k][0])], before[1][int(batch.slots[k][0])]), k


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5])
def test_one_copy_home_after_the_filter_is_enqueued(B, monkeypatch):
    """Every route from a device tensor to the host is counted as tests/test_byte_frame_batch.py counts them: one frame_batch() takes exactly one,
    whatever the number of problems, none has happened when busca_msframe_apply is enqueued, and every library entry point is called once - the
    appearance cost not at all: the cost kernel forms its entries itself."""
    import torch
    from busca_amd import _msframe_lib, geometry
    batch = _batch("single") if B == 1 else Batch(_batch("six").scenes[:5], 6)
    assert len(batch.scenes) == B
    st, ref = batch.store(), batch.store()
    want = batch.frames(ref, 3, 0.98)
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
            if name == "busca_msframe_apply":
                count["at_apply"] = count["n"]
            return real(*a)
        monkeypatch.setattr(lib, name, f)
    for name in ("busca_msframe_advance", "busca_msframe_cost", "busca_msframe_apply"):
        wrapped(_msframe_lib.load(), name)
    for name in ("busca_assign_stages", "busca_appearance_cost"):
        wrapped(geometry.default_context(0).lib, name)
    got = st.frame_batch(batch.problems(), cascade_depth=3, mc_lambda=0.98, **KW)
    copies = count["n"]
    monkeypatch.undo()
    assert count["at_apply"] == 0 and copies == 1
    assert calls == {"busca_msframe_advance": 1, "busca_msframe_cost": 1, "busca_assign_stages": 1, "busca_msframe_apply": 1}
    _same_frames(got, want, B)
    _same(_all_of(st), _all_of(ref), B)


@pytest.mark.gpu
def test_a_batch_behind_a_busy_stream(busy):
    from tests.test_streams_gpu import behind
    warps = euclidean_warps()
    mk = lambda seeds: Batch([Scene(17, 65, seeds[0], matrix=warps[2]), Scene(16, 64, seeds[1]), Scene(0, 9, seeds[2])])      # noqa: E731
    batch, other = mk((22, 8, 1)), mk((99, 98, 97))
    full = lambda b: [_dev(x) for x in _all_of(b.store())]        # noqa: E731
    st = batch.store()

    def call(x, outs, stream):
        st.mean, st.cov, st.feat = x
        got = st.frame_batch(batch.problems(), cascade_depth=3, mc_lambda=0.98, **KW)
        return [np.asarray(v, dtype=np.int64) for fr in got for v in fr]
    want, got = behind(busy, "SortStore.frame_batch", call, true=full(batch), poison=full(other), form="current", host=True)
    assert len(got[3]) >= 6 and len(got[3 + 3]) >= 1 and len(got[3 + 10 + 3]) >= 1      # matches and new tracks; the third problem starts tracks
    ref = batch.store()
    batch.frames(ref, 3, 0.98)
    _same(got[:3], _all_of(ref), "behind a busy stream")


# ---- GPU: scripted sequences in lock step on one store --------------------------------------------------------------------------------
def _script(seed, frames, W=E):
    """A seeded scene of 6 targets over `frames` frames -> per frame (tlwh [m,4], confidences [m], features [m,W], camera matrix or None).  Targets are
    born at different frames, one goes missing for good, one for two frames; every target keeps a feature of its own, seen with a little noise;
    the detections of a frame come in an order that is not the tracks'; the camera moves at two frames."""
    rs = np.random.RandomState(seed)
    T = 6
    start = np.stack([120.0 + 260 * np.arange(T), 150.0 + 90 * (np.arange(T) % 3), rs.uniform(40, 60, T), rs.uniform(100, 150, T)], 1)
    vel = rs.uniform(-6, 6, (T, 2))
    born = [0, 0, 0, 0, 2, 5]
    gone = {1: range(4, frames), 3: range(6, 8)}
    F = rs.normal(size=(T, W))
    warps = euclidean_warps()
    out = []
    for f in range(frames):
        live = [t for t in range(T) if f >= born[t] and f not in gone.get(t, ())]
        live = [live[i] for i in rs.permutation(len(live))]
        boxes = np.array([np.concatenate([start[t, :2] + f * vel[t] + rs.uniform(-1, 1, 2), start[t, 2:] + rs.uniform(-1, 1, 2)]) for t in live]).reshape(-1, 4)
        feats = (F[live] + rs.normal(scale=0.05, size=(len(live), W))).astype(np.float32).reshape(-1, W)
        conf = np.array([[0.0, 0.4, 0.999, 0.7][(t + f) % 4] for t in live])
        out.append((boxes, conf if seed % 2 else None, feats, warps[(seed + f) % 8] if f in (3, 8) else None))
    return out


class Sequence:
    """StrongSORT's host bookkeeping for one sequence on its own range of slots: hits, confirmation after N_INIT hits, deletion of a tentative track
    at its first miss and of a confirmed one beyond MAX_AGE, the free slots handed out in the order they are popped."""
    N_INIT, MAX_AGE = 3, 2

    def __init__(self, script, slots, start):
        self.script, self.start = script, start
        self.free = list(slots)[::-1]
        self.tracks = []
        self.seen = {"births": 0, "confirmed": 0, "deleted": 0, "reused": False, "cascade": 0}
        self.freed = set()

    def active(self, t):
        return 0 <= t - self.start < len(self.script)

    def problem(self, t):
        from busca_amd.sort_store import SortFrameProblem
        boxes, conf, feats, mat = self.script[t - self.start]
        for tr in self.tracks:
            tr.time_since_update += 1
        return SortFrameProblem([tr.slot for tr in self.tracks], [tr.time_since_update for tr in self.tracks], [tr.confirmed for tr in self.tracks], boxes,
                                conf, feats, self.free[::-1][:len(boxes)], mat)

    def absorb(self, fr):
        for r, _ in fr.matches:
            tr = self.tracks[r]
            self.seen["cascade"] += int(tr.confirmed)
            tr.time_since_update, tr.hits = 0, tr.hits + 1
            if not tr.confirmed and tr.hits >= self.N_INIT:
                tr.confirmed = True
                self.seen["confirmed"] += 1
        assert fr.overflow == []
        born = []
        for _, s in fr.new_tracks:                                 # the slots the frame took are the ones the host pops, in that order
            assert self.free.pop() == s
            self.seen["reused"] |= s in self.freed
            born.append(types.SimpleNamespace(slot=s, time_since_update=0, hits=1, confirmed=False))
            self.seen["births"] += 1
        for r in fr.unmatched_tracks:
            tr = self.tracks[r]
            if not tr.confirmed or tr.time_since_update > self.MAX_AGE:
                self.free.append(tr.slot)
                self.freed.add(tr.slot)
                self.tracks[r] = None
                self.seen["deleted"] += 1
        self.tracks = [tr for tr in self.tracks if tr is not None] + born


@pytest.mark.gpu
def test_three_scripted_sequences_in_lock_step():
    """Three sequences of different lengths, staggered, through frame_batch() on one store - batches of 1, 2, 3, 2 and 1 problems over 14 time steps -
    and the same three through frame() on a second store: the same frames and the same bits in the whole store after every step."""
    plan = [(11, 14, 0), (12, 9, 2), (13, 4, 5)]                   # (seed, frames, first time step)
    mk = lambda: [Sequence(_script(seed, frames), PERM[16 * k:16 * k + 16].astype(int), start) for k, (seed, frames, start) in enumerate(plan)]      # noqa: E731
    a, b = _fstore(capacity=CAP, E=E), _fstore(capacity=CAP, E=E)
    lock, ones = mk(), mk()
    sizes = []
    for t in range(14):
        act = [k for k in range(3) if lock[k].active(t)]
        sizes.append(len(act))
        got = a.frame_batch([lock[k].problem(t) for k in act], cascade_depth=Sequence.MAX_AGE, mc_lambda=0.98, **KW)
        for k, fr in zip(act, got):
            p = ones[k].problem(t)
            want = b.frame(p.slots, p.time_since_update, p.confirmed, p.det_tlwh, p.det_confidence, p.det_features, MAX_IOU, MATCH_THRESH, ALPHA,
                           free_slots=p.free_slots, cascade_depth=Sequence.MAX_AGE, mc_lambda=0.98, camera_matrix=p.camera_matrix)
            _same_frames([fr], [want], (t, k))
            lock[k].absorb(fr)
            ones[k].absorb(want)
        _same(_all_of(a), _all_of(b), t)
    assert sizes == [1, 1, 2, 2, 2, 3, 3, 3, 3, 2, 2, 1, 1, 1]
    print([s.seen for s in lock])
    seen = lock[0].seen                                            # the script does what it is for: births, confirmations, a deletion, cascade matches
    assert seen["births"] >= 6 and seen["confirmed"] >= 3 and seen["deleted"] >= 1 and seen["cascade"] >= 6, seen
    assert lock[1].seen["confirmed"] >= 2 and lock[2].seen["births"] >= 4 and [s.seen for s in lock] == [s.seen for s in ones]
