"""A whole StrongSORT frame on resident state: libbusca_sframe.so (include/busca_sframe.h), its binding busca_amd._sframe_lib and SortStore.frame -
the camera update and the prediction, both planes of the cost slab, busca_assign_stages, the EMA feature rows, the NSA update and initiation as one chain.

The oracle is the set of calls this repository had before and pins elsewhere: SortStore.predict / camera_update / gate_cost / iou_cost / match /
update / initiate (tests/test_sort_store.py, tests/test_assign_stages.py) and busca_store_ema_fit (tests/test_store_kernels.py), composed on a
second store loaded alike (`_composed` below).  Every comparison is np.array_equal - match lists, new tracks, and the whole of mean, cov and feat;
no tolerance is introduced here.  (A row whose covariance is not positive definite is NaN in both routes: asserted with np.isnan.)  What the
composition itself must be - which call follows which, what the host does between them - is pinned to the reference's own tracker by
tests/test_sort_tracker_replay.py, which found the order of camera update and prediction used here until version 1001."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests.test_kalman_filter import gold, r_initiate
from tests.test_sort_store import (_dev, _scene, _untouched, _xyah_of, detections_near, euclidean_warps, r_predict, r_update_nsa, states,
                                    tlwh_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 128
PERM = np.random.RandomState(17).permutation(CAP)
E = 32
MATCH_THRESH, MAX_IOU, ALPHA = 0.3, 0.7, 0.9
CONFS = np.array([0.0, 0.3, 0.999, 0.6])
_CACHE = {}


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    from busca_amd.build import build
    hip_lib = build()
    from busca_amd import _frame_lib, _lib, _rounds_lib, _sframe_lib, _sort_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_sframe.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_sframe_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _sframe_lib.SFRAME_API.items()}
    assert sorted(declared) == ["busca_sframe_advance", "busca_sframe_apply", "busca_sframe_cost", "busca_sframe_last_error", "busca_sframe_version"]
    assert (declared["busca_sframe_advance"], declared["busca_sframe_cost"], declared["busca_sframe_apply"]) == (8, 23, 20)
    for name, val in (("BUSCA_SFRAME_MC", _sframe_lib.MC), ("BUSCA_SFRAME_CLAMP", _sframe_lib.CLAMP), ("BUSCA_SFRAME_MAX_DETS", _sframe_lib.MAX_DETS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert (_sframe_lib.MC, _sframe_lib.CLAMP) == (_sort_lib.MC, _sort_lib.CLAMP)

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_sframe_lib.SFRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_sframe_lib.SFRAME_API)
    others = [hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH, _rounds_lib.ROUNDS_LIB_PATH, _sort_lib.SORT_LIB_PATH, _frame_lib.FRAME_LIB_PATH]
    assert os.path.basename(hip_lib) == "libbusca_hip.so" and len({os.path.basename(p) for p in others}) == 6
    for other in others:
        theirs = {n for n in exported(other) if not n.startswith("_")}
        assert not [n for n in theirs if n.startswith("busca_sframe")], other
        assert not (theirs & ours), other
    assert "busca_sframe.h" not in _lib.HEADERS and "_sframe_lib" not in open(_lib.__file__.replace(".pyc", ".py")).read()
    lib = _sframe_lib.load()
    assert lib.busca_sframe_version() == 1001 and _sframe_lib.ABI_MAJOR == 1 and lib.busca_sframe_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _sframe_lib
    lib = _sframe_lib.load()
    P, Q, ODD, n, m = 0x10000, 0x20000, 0x10004, 3, 5     # two aligned addresses, one that is 4- but not 8-byte aligned
    nan = float("nan")

    def calls(mean=P, cov=P, S=8, slot=P, n=n, matrix=None, xyah=P, tlwh=P, m=m, stale=None, cost=P, ld=None, gated=1e5, flags=3, lam=0.98, maxd=0.3,
              maxiou=0.7, first=P, again=P, depth=3, out=Q, status=P, r2c=P, c2r=P, conf=P, dfeat=P, feat=P, E=16, alpha=0.9, free=P, n_free=2,
              new=P, dev=0):
        ld = m if ld is None else ld
        return {
            "busca_sframe_advance": lambda: lib.busca_sframe_advance(mean, cov, S, slot, n, matrix, dev, None),
            "busca_sframe_cost": lambda: lib.busca_sframe_cost(mean, cov, S, slot, n, xyah, tlwh, m, stale, cost, ld, gated, flags, lam, maxd, maxiou,
                                                               first, again, depth, out, status, dev, None),
            "busca_sframe_apply": lambda: lib.busca_sframe_apply(mean, cov, S, slot, n, r2c, c2r, xyah, conf, dfeat, m, feat, E, alpha, free, n_free,
                                                                 new, status, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_sframe_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    nothing = dict(mean=None, cov=None, slot=None, out=None, cost=None, r2c=None, c2r=None, xyah=None, tlwh=None, first=None, again=None, dfeat=None,
                   feat=None, new=None, free=None, conf=None, status=None)
    for name in calls():
        assert calls(n=0, m=0)[name]() == 0, name                                  # the no-op
        assert calls(n=0, m=0, **nothing)[name]() == 0, name
        refused(name, "null pointer", mean=None)
        refused(name, "null pointer", cov=None)
        refused(name, "null pointer", slot=None)
        refused(name, "negative size", n=-1)
        refused(name, "negative size", S=-1)
        refused(name, "negative device", dev=-1)
        refused(name, "misaligned", mean=ODD)
        refused(name, "misaligned", cov=ODD)
        refused(name, "misaligned", slot=0x10002)
    refused("busca_sframe_advance", "misaligned", matrix=ODD)
    for name in ("busca_sframe_cost", "busca_sframe_apply"):
        refused(name, "negative size", m=-1)
        refused(name, "null pointer", xyah=None)
        refused(name, "misaligned", xyah=ODD)
        refused(name, "misaligned", status=0x10002)
    name = "busca_sframe_cost"
    assert calls(n=0)[name]() == 0 and calls(m=0)[name]() == 0 and calls(m=0, **{k: None for k in ("xyah", "tlwh", "cost", "out", "first")})[name]() == 0
    refused(name, "negative size (depth", depth=-1)
    refused(name, "null pointer", tlwh=None)
    refused(name, "null pointer", cost=None)
    refused(name, "null pointer", first=None)
    refused(name, "null pointer", out=None)
    refused(name, "misaligned", tlwh=ODD)
    refused(name, "misaligned", cost=ODD)
    refused(name, "misaligned", out=ODD)
    refused(name, "misaligned", first=0x10002)
    refused(name, "misaligned", again=0x10002)
    refused(name, "max_distance is NaN", maxd=nan)
    refused(name, "max_iou_distance is NaN", maxiou=nan)
    refused(name, "mc_lambda is NaN", lam=nan)
    refused(name, "unknown flag bits", flags=4)
    refused(name, "unknown flag bits", flags=-1)
    refused(name, "ld_cost", ld=4)
    refused(name, "out must not be cost", out=P)
    refused(name, "more workgroups than a grid holds", n=16 * 65535 + 1)
    assert calls(lam=nan, maxd=nan, flags=0, n=0)[name]() == 0                    # NaN without its flag is no argument of the call
    assert calls(again=None, n=0)[name]() == 0
    name = "busca_sframe_apply"
    refused(name, "negative size (n_free", n_free=-1)
    refused(name, "alpha is NaN", alpha=nan)
    refused(name, "E 0", E=0)
    refused(name, "E -3", E=-3)
    refused(name, "one call takes 2048", m=2049)
    refused(name, "more workgroups than a grid holds", n=2 ** 31 - 1, m=1)
    refused(name, "null pointer", feat=None)
    refused(name, "null pointer", r2c=None)
    refused(name, "null pointer", c2r=None)
    refused(name, "null pointer", dfeat=None)
    refused(name, "null pointer", new=None)
    refused(name, "null pointer", free=None)
    refused(name, "misaligned", conf=ODD)
    refused(name, "misaligned", dfeat=0x10002)
    refused(name, "misaligned", feat=0x10002)
    refused(name, "misaligned", r2c=0x10002)
    refused(name, "misaligned", c2r=0x10002)
    refused(name, "misaligned", free=0x10002)
    refused(name, "misaligned", new=0x10002)
    # the message is the calling thread's own
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_sframe_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_sframe_last_error() != b""


def test_python_level_checks():
    import sys
    import torch
    from busca_amd import tracking
    from busca_amd.sort_store import SortFrame, SortStore
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    import busca.tracking as alias
    assert tracking.SortFrame is SortFrame is alias.SortFrame
    assert SortFrame._fields == ("matches", "unmatched_tracks", "unmatched_detections", "new_tracks", "overflow")
    boxes, feats = np.array([[100.0, 100.0, 40.0, 80.0]] * 3), np.ones((3, 16), dtype=np.float32)
    ok = dict(slots=[1, 2], time_since_update=[1, 1], confirmed=[True, False], det_tlwh=boxes, det_confidence=[0.5] * 3, det_features=feats,
              max_iou_distance=0.7, matching_threshold=0.3, ema_alpha=0.9, free_slots=[4, 5])
    # without feature_dim the store is what it was, and refuses frame
    plain = SortStore(CAP)
    assert plain.feature_dim is None and plain.feat is None and plain.mean is None
    with pytest.raises(ValueError, match="feature_dim"):
        plain.frame(**ok)
    for call in (lambda: plain.features([1]), lambda: plain.load_features([1], feats[:1])):
        with pytest.raises(ValueError, match="feature_dim"):
            call()
    with pytest.raises(ValueError):
        SortStore(CAP, feature_dim=0)
    st = SortStore(CAP, feature_dim=16)
    for kw, words in ((dict(slots=[1, 1]), "distinct"),
                      (dict(slots=[1, CAP]), "beyond the capacity"),
                      (dict(free_slots=[4, 4]), "distinct"),
                      (dict(free_slots=[CAP]), "beyond the capacity"),
                      (dict(free_slots=[-1]), "negative"),
                      (dict(free_slots=[4, 2]), "also listed"),
                      (dict(time_since_update=[1]), "time_since_update entries"),
                      (dict(confirmed=[True] * 3), "confirmed flags"),
                      (dict(det_confidence=[0.5] * 2), "2 confidences for 3 detections"),
                      (dict(det_features=feats[:2]), "features for 3 detections"),
                      (dict(det_features=np.ones((3, 32), dtype=np.float32)), "feature_dim 16"),
                      (dict(det_features=torch.ones(3, 8)), "feature_dim 16"),
                      (dict(ema_alpha=None), "ema_alpha"),
                      (dict(ema_alpha=float("nan")), "ema_alpha"),
                      (dict(cascade_depth=128), "stages"),
                      (dict(camera_matrix=np.eye(2)), "3 x 3"),
                      (dict(camera_matrix=np.eye(3), predict=False), "predict=False"),
                      (dict(det_tlwh=torch.ones(3, 4)), "host"),
                      (dict(slots=torch.tensor([1, 2])), "host slot lists"),
                      (dict(slots=list(range(2049)) if CAP > 2049 else [1, 2], det_tlwh=np.ones((2049, 4)), det_confidence=None,
                            det_features=np.ones((2049, 16), dtype=np.float32)), "at most 2048")):
        with pytest.raises(ValueError, match=words):
            st.frame(**{**ok, **kw})
    with pytest.raises(ValueError, match="multiple of 16"):
        SortStore(CAP, feature_dim=24).frame(**{**ok, "det_features": np.ones((3, 24), dtype=np.float32)})
    with pytest.raises(ValueError, match="rows for"):
        st.load_features([1, 2], feats)
    assert st.mean is None and st.feat is None                                     # nothing was allocated


# ---- GPU: helpers -----------------------------------------------------------------------------------------------------------
def _fstore(mean=None, cov=None, slots=None, feats=None, capacity=CAP, E=E):
    """A SortStore with feature rows; the states mean[i] / cov[i] and the raw feature rows feats[i] in slot slots[i] for the live entries."""
    from busca_amd.sort_store import SortStore
    st = SortStore(capacity, feature_dim=E)
    st._state()
    if mean is not None and len(mean):
        slots = np.asarray(slots)
        live = (slots >= 0) & (slots < capacity)
        idx = _dev(slots[live]).long()
        st.mean[idx] = _dev(np.asarray(mean)[live])
        st.cov[idx] = _dev(np.asarray(cov)[live])
        if feats is not None:
            st.feat[idx] = _dev(np.asarray(feats, dtype=np.float32)[live])
    return st


def _all_of(st):
    return st.mean.cpu().numpy(), st.cov.cpu().numpy(), st.feat.cpu().numpy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("mean", "cov", "feat")):
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:4].tolist())


def _ema_fit(st, pairs_old, pairs_new):
    """busca_store_ema_fit itself on the store's feature table seen as a [capacity + 1, 1, E] gallery, in place: (slot, detection) pairs that have a
    row (group_old_row 0) and pairs that start one (-1), one source each.  -> nothing; `feats` is read from st._det_feats."""
    from busca_amd import _store_lib
    pairs = [(s, 0, j) for s, j in pairs_old] + [(s, -1, j) for s, j in pairs_new]
    g = len(pairs)
    if g == 0:
        return
    table = _dev(np.concatenate([[s for s, _, _ in pairs], [o for _, o, _ in pairs], np.arange(g + 1), [j for _, _, j in pairs]]).astype(np.int32))
    f = st._det_feats
    _store_lib.check(_store_lib.load().busca_store_ema_fit(st.feat.data_ptr(), st.capacity + 1, 1, st.feature_dim, f.data_ptr(), f.shape[0],
                                                           table.data_ptr(), table[g:].data_ptr(), table[2 * g:].data_ptr(), table[3 * g + 1:].data_ptr(),
                                                           g, g, ALPHA, *st._where()))


def tracked_states(n):
    """n states on a grid of boxes that do not overlap, after two predict / update steps of the restated filter with mixed confidences (covariances
    that are not symmetric in their last bits, velocities that are not zero).  Built once per n, never written."""
    if ("tracked", n) not in _CACHE:
        i = np.arange(n)
        rs = np.random.RandomState(40 + n)
        z0 = np.stack([150.0 + 140 * (i % 8), 200.0 + 320 * (i // 8), rs.uniform(0.4, 0.6, n), rs.uniform(100, 140, n)], 1)
        mean, cov = r_initiate(z0)
        vel = rs.uniform(-3, 3, (n, 2))
        for s in range(2):
            new = []
            for k in range(n):
                m, c = r_predict(mean[k], cov[k])
                z = m[:4] + np.concatenate([vel[k] + rs.uniform(-0.5, 0.5, 2), [rs.uniform(-0.005, 0.005)], [rs.uniform(-1, 1)]])
                new.append(r_update_nsa(m, c, z, [0.0, 0.35, 0.8, 0.999][(k + s) % 4]))
            mean, cov = np.stack([a for a, _ in new]), np.stack([b for _, b in new])
        for a in (mean, cov):
            a.setflags(write=False)
        _CACHE[("tracked", n)] = (mean, cov)
    return _CACHE[("tracked", n)]


class Scene:
    """n tracks (tracked_states) in scattered slots of a store of 128 with unit feature rows, and m detections: most sit on the prediction of a track
    with that track's feature (some tracks are offered several), every 11th carries the opposite feature (the cascade rejects it, the IoU stage may
    take it), every 9th is a newcomer far from every track.  Ages: a third of the tracks at 1, the others spread over 1 .. 30, a few beyond; every
    fifth track is unconfirmed.  `tie`: integer boxes without velocities, one covariance, features from four axis vectors and detections in
    duplicate - costs on a coarse grid, whole columns equal."""

    def __init__(self, n, m, seed, tie=False):
        rs = np.random.RandomState(seed)
        nn = n if n else 8
        i = np.arange(nn)
        if tie:
            z0 = np.stack([150.0 + 60 * (i % 8), 200.0 + 160 * (i // 8), np.full(nn, 0.5), np.full(nn, 128.0)], 1)
            mean, cov = r_initiate(z0)
            F = np.eye(E)[i % 4] + np.eye(E)[4 + i % 3]
        else:
            mean, cov = tracked_states(nn)
            F = rs.normal(size=(nn, E))
        F = (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)
        self.n, self.m = n, m
        self.mean, self.cov, self.F = mean[:n], cov[:n], F[:n]
        self.slots = PERM[:n].astype(np.int64)
        self.free = PERM[n:].astype(np.int64)
        self.tsu = np.where(i % 3 == 0, 1, 1 + (i * 7) % 30)[:n]
        self.tsu = np.where(i[:n] % 13 == 5, 31 + i[:n], self.tsu)
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
        self.conf = CONFS[j % 4]

    def store(self):
        st = _fstore(self.mean, self.cov, self.slots, self.F)
        st._det_feats = _dev(self.feats) if self.m else None
        return st


class RowMetric:
    """What match() needs of a metric, over the feature rows of a store: track ids are slots, the gallery is `feat` seen as [capacity + 1, 1, E]."""

    def __init__(self, st, ctx):
        self.st, self.ctx, self.matching_threshold = st, ctx, MATCH_THRESH

    def distance(self, features, targets, device=False):
        from busca_amd.appearance import appearance_cost
        out = appearance_cost(self.st.feat.view(self.st.capacity + 1, 1, -1), features, "min", slot=np.asarray(targets, dtype=np.int32), ctx=self.ctx)
        return out if device else out.cpu().numpy()


def _composed(st, sc, free, depth, lam, mat, ctx, predict=True, apply=True):
    """The frame on the calls this repository had before: camera_update, predict (the reference's order, deep_sort_app.py:186-189), match with a metric over the same rows, update, initiate and
    busca_store_ema_fit for the rows -> what SortFrame holds, as plain lists, and the update's status words."""
    if predict:
        if mat is not None:
            st.camera_update(sc.slots, mat)
        st.predict(sc.slots)
    if sc.m == 0:
        return dict(matches=[], unmatched_tracks=list(range(sc.n)), unmatched_detections=[], new_tracks=[], overflow=[], status=np.zeros(0, dtype=np.int32))
    matches, ut, ud = st.match(RowMetric(st, ctx), sc.slots, [int(s) for s in sc.slots], sc.tsu, sc.confirmed, st._det_feats, sc.xyah, sc.tlwh, MAX_IOU,
                               cascade_depth=depth, mc_lambda=lam)
    status = np.zeros(0, dtype=np.int32)
    new, overflow = [], []
    if apply:
        rows, cols = [r for r, _ in matches], [c for _, c in matches]
        status = st.update(sc.slots[rows], sc.xyah, cols, confidence=sc.conf).cpu().numpy()
        k = min(len(ud), len(free))
        st.initiate(free[:k], sc.xyah, ud[:k])
        new, overflow = [(int(j), int(s)) for j, s in zip(ud[:k], free[:k])], [int(j) for j in ud[k:]]
        _ema_fit(st, [(int(sc.slots[r]), c) for r, c in matches], [(s, j) for j, s in new])
    return dict(matches=[(int(r), int(c)) for r, c in matches], unmatched_tracks=sorted(int(r) for r in ut), unmatched_detections=[int(j) for j in ud],
                new_tracks=new, overflow=overflow, status=status)


def _frame(st, sc, free, depth, lam, mat, **kw):
    return st.frame(sc.slots, sc.tsu, sc.confirmed, sc.tlwh, sc.conf, st._det_feats if sc.m else sc.feats, MAX_IOU, MATCH_THRESH, ALPHA, free_slots=free,
                    cascade_depth=depth, mc_lambda=lam, camera_matrix=mat, **kw)


def _agree(sc, free, depth, lam, mat, ctx, what, **kw):
    """frame() on one store, the composed route on a copy: the same lists, the same bits in every slot."""
    a, b = sc.store(), sc.store()
    before = _all_of(a)
    got = _frame(a, sc, free, depth, lam, mat, **kw)
    want = _composed(b, sc, free, depth, lam, mat, ctx, **kw)
    assert not want["status"].any(), what
    for field in ("matches", "unmatched_tracks", "unmatched_detections", "new_tracks", "overflow"):
        assert [tuple(x) if isinstance(x, tuple) else int(x) for x in getattr(got, field)] == want[field], (what, field, getattr(got, field), want[field])
    after = _all_of(a)
    _same(after, _all_of(b), what)
    touched = list(sc.slots) + [s for _, s in want["new_tracks"]]
    _untouched(before, after, touched, what)
    keep = np.ones(CAP + 1, dtype=bool)
    keep[touched] = False
    assert np.array_equal(before[2][keep], after[2][keep]), what
    return got


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


# ---- GPU: the three calls -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_matrix", [False, True])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_advance_is_camera_update_then_predict(n, with_matrix):
    from busca_amd import _sframe_lib
    mean, cov = states(5)
    k = np.arange(n) % 24
    slots = np.random.RandomState(5).permutation(80)[:n].astype(np.int32)
    a, b = _fstore(mean[k], cov[k], slots, capacity=80), _fstore(mean[k], cov[k], slots, capacity=80)
    listed = _dev(np.insert(slots, [0, n], [-1, 80]).astype(np.int32))             # one entry -1, one beyond the capacity: skipped
    mat = euclidean_warps()[1] if with_matrix else None
    before = _all_of(a)
    dmat = None if mat is None else _dev(mat)
    _sframe_lib.check(_sframe_lib.load().busca_sframe_advance(a.mean.data_ptr(), a.cov.data_ptr(), 80, listed.data_ptr(), n + 2,
                                                              None if dmat is None else dmat.data_ptr(), *a._where()))
    if mat is not None:
        b.camera_update(listed, mat)
    b.predict(listed)
    after = _all_of(a)
    _same(after, _all_of(b), (n, with_matrix))
    _untouched(before, after, slots, "advance")                                    # every unlisted slot and the spare one: unchanged in every bit
    assert not np.array_equal(after[0][slots], before[0][slots]) and not np.array_equal(after[1][slots], before[1][slots])
    if mat is not None:                                                            # the warp did something: not the predicted mean, and the
        c, d = _fstore(mean[k], cov[k], slots, capacity=80), _fstore(mean[k], cov[k], slots, capacity=80)      # order shows in mean and covariance
        c.predict(listed)
        assert not np.array_equal(_all_of(c)[0][slots, :4], after[0][slots, :4])
        d.predict(listed)
        d.camera_update(listed, mat)
        assert not np.array_equal(_all_of(d)[0][slots], after[0][slots]) and not np.array_equal(_all_of(d)[1][slots], after[1][slots])


def _raw_cost(st, slot, xyah, tlwh, stale, cost, ld, gated, lam, first, again, depth, guard=64, canary=777.25):
    """busca_sframe_cost itself into a slab with a guard band on both sides -> (the slab [2, n, m], the status words)."""
    import torch
    from busca_amd import _sframe_lib
    n, m = len(first), len(xyah)
    buf = torch.full((2 * n * m + 2 * guard,), canary, dtype=torch.float64, device=st.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    d = [_dev(np.ascontiguousarray(x)) for x in (xyah, tlwh, stale.astype(np.uint8), cost, first.astype(np.int32), again.astype(np.int32))]
    _sframe_lib.check(_sframe_lib.load().busca_sframe_cost(
        st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, slot.data_ptr(), n, d[0].data_ptr(), d[1].data_ptr(), m, d[2].data_ptr(), d[3].data_ptr(), ld,
        gated, (_sframe_lib.MC if lam is not None else 0) | _sframe_lib.CLAMP, 0.0 if lam is None else lam, MATCH_THRESH, MAX_IOU, d[4].data_ptr(),
        d[5].data_ptr(), depth, buf.data_ptr() + 8 * guard, status.data_ptr() + 4 * guard, *st._where()))
    buf, status = buf.cpu().numpy(), status.cpu().numpy()
    assert (buf[:guard] == canary).all() and (buf[guard + 2 * n * m:] == canary).all(), "written outside the slab"
    assert (status[:guard] == -7).all() and (status[guard + n:] == -7).all(), "written outside the status words"
    return buf[guard:guard + 2 * n * m].reshape(2, n, m), status[guard:guard + n]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (15, 63), (16, 64), (17, 65)])
def test_cost_planes(n, m):
    DEPTH = 3
    mean, cov = (a[:n].copy() for a in states(5))
    slots = PERM[:n].astype(np.int32)
    bad = np.zeros(n, dtype=bool)
    if n >= 15:
        slots[2], slots[9] = -1, CAP                               # skipped: negative, beyond the capacity
        cov[4, :4, :4] = -np.eye(4)                                # not positive definite
        bad[4] = True
    st = _fstore(mean, cov, slots)
    dslot = _dev(slots)
    xyah = detections_near(mean, m, 3 * n + m)
    tlwh = tlwh_of(xyah)
    stale = np.arange(n) % 5 == 3
    cost = np.random.RandomState(n * m).uniform(0.0, 0.6, (n, m + 3))      # a leading dimension beyond m
    seen_status = set()
    for lam in (None, 0.98):
        for gated in (1e5, 7.0):
            gate, gstatus = st.gate_cost(dslot, cost[:, :m], xyah, mc_lambda=lam, gated_cost=gated, max_distance=MATCH_THRESH)
            iou = st.iou_cost(dslot, tlwh, stale=stale, max_distance=MAX_IOU).cpu().numpy()
            gate, gstatus = gate.cpu().numpy(), gstatus.cpu().numpy()
            assert np.array_equal(gstatus != 0, bad)
            for shift in (0, 1):
                # rows in turn: plane 0 only (a cascade level), plane 1 only (unconfirmed), both (age 1), neither (older than the cascade)
                kind = (np.arange(n) + shift) % 4
                first = np.select([kind == 0, kind == 1, kind == 2], [np.arange(n) % DEPTH, DEPTH, 0], -1)
                again = np.where(kind == 2, DEPTH, -1)
                need0, need1 = (kind == 0) | (kind == 2), (kind == 1) | (kind == 2)
                slab, status = _raw_cost(st, dslot, xyah, tlwh, stale, cost, m + 3, gated, lam, first, again, DEPTH)
                what = (n, m, lam, gated, shift)
                ok0 = need0 & ~bad
                assert np.array_equal(slab[0][ok0], gate[ok0]) and np.isnan(slab[0][need0 & bad]).all(), what
                assert np.array_equal(slab[1][need1], iou[need1]), what
                assert np.isposinf(slab[0][~need0]).all() and np.isposinf(slab[1][~need1]).all(), what
                assert np.array_equal(status, (need0 & bad).astype(np.int32)), what      # a row that is not gated has status 0 whatever its covariance
                seen_status.add(int(status.sum()))
                if n >= 15:                                        # skipped and stale rows behave as the two kernels define
                    for r in (2, 9):
                        assert not need0[r] or (slab[0][r] == (gated if gated <= MATCH_THRESH else MATCH_THRESH + 1e-5)).all(), what
                        assert not need1[r] or (slab[1][r] == MAX_IOU + 1e-5).all(), what
                    assert all((slab[1][r] == MAX_IOU + 1e-5).all() for r in np.nonzero(stale & need1)[0]), what
    if n >= 15:
        assert seen_status == {0, 1}
    if n >= 16 and m >= 64:
        assert (gate[~bad] < MATCH_THRESH).any() and (gate[~bad] > MATCH_THRESH).any() and (iou < MAX_IOU).any()
    # again = NULL: never
    from busca_amd import _sframe_lib
    import torch
    first = np.where(np.arange(n) % 2 == 0, 0, DEPTH).astype(np.int32)
    out = torch.empty(2, n, m, dtype=torch.float64, device=st.dev)
    d = [_dev(np.ascontiguousarray(x)) for x in (xyah, tlwh, cost, first)]
    _sframe_lib.check(_sframe_lib.load().busca_sframe_cost(st.mean.data_ptr(), st.cov.data_ptr(), CAP, dslot.data_ptr(), n, d[0].data_ptr(), d[1].data_ptr(), m,
                                                           None, d[2].data_ptr(), m + 3, 1e5, 3, 0.98, MATCH_THRESH, MAX_IOU, d[3].data_ptr(), None, DEPTH,
                                                           out.data_ptr(), None, *st._where()))
    out = out.cpu().numpy()
    assert np.isposinf(out[0][first != 0]).all() and np.isposinf(out[1][first == 0]).all() and not np.isposinf(out[1][first != 0]).any()


def _raw_apply(st, slot, r2c, c2r, xyah, conf, dfeat, alpha, free, guard=16):
    import torch
    from busca_amd import _sframe_lib
    n, m, n_free = len(slot), len(c2r), len(free)
    d = [_dev(np.asarray(x, dtype=np.int32)) if len(x) else None for x in (slot, r2c, c2r, free)]
    d_xyah, d_conf, d_feat = _dev(np.asarray(xyah, dtype=np.float64)), None if conf is None else _dev(np.asarray(conf, dtype=np.float64)), _dev(dfeat)
    new = torch.full((m + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    status = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=st.dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _sframe_lib.check(_sframe_lib.load().busca_sframe_apply(st.mean.data_ptr(), st.cov.data_ptr(), st.capacity, ptr(d[0]), n, ptr(d[1]), ptr(d[2]),
                                                            d_xyah.data_ptr(), ptr(d_conf), d_feat.data_ptr(), m, st.feat.data_ptr(), st.feature_dim, alpha,
                                                            ptr(d[3]), n_free, new.data_ptr() + 4 * guard, status.data_ptr() + 4 * guard, *st._where()))
    new, status = new.cpu().numpy(), status.cpu().numpy()
    assert (new[:guard] == -7).all() and (new[guard + m:] == -7).all() and (status[:guard] == -7).all() and (status[guard + n:] == -7).all()
    return new[guard:guard + m], status[guard:guard + n]


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 63, 64, 65, 255, 256, 257, 512, 1000])
def test_apply_equals_update_initiate_and_ema_fit(width):
    import torch
    g = gold()
    S, GUARD, CANARY, n, m = 24, 6, 777.25, 12, 14
    rs = np.random.RandomState(width)
    slots = np.random.RandomState(3).permutation(S)[:n].astype(np.int32)
    slots[5] = -1                                                  # a skipped row that the solver matched all the same
    mean, cov = g["mean"][:n], g["cov"][:n]
    rows0 = rs.normal(size=(S + 1, width)).astype(np.float32)      # the table as it stands: raw rows, not normalised
    dfeat = (rs.normal(size=(m, width)) * rs.uniform(0.3, 4.0, (m, 1))).astype(np.float32)
    r2c = np.array([3, -1, 0, 7, -1, 9, 12, -1, 5, 1, -1, 13], dtype=np.int32)
    c2r = np.full(m, -1, dtype=np.int32)
    c2r[r2c[r2c >= 0]] = np.nonzero(r2c >= 0)[0]
    xyah = g["meas"][np.maximum(c2r, 0)]                           # a matched detection is its track's measurement of the fixture
    births = [j for j in range(m) if c2r[j] < 0]                   # 6 of them
    rest = [s for s in range(S) if s not in slots]
    free = np.array(rest[:2] + [S + 3] + rest[2:4], dtype=np.int32)        # one beyond the capacity: reported and skipped; 5 for 6 births
    assert len(births) == 6
    conf = np.array([0.0, 0.3, 0.999])[np.arange(m) % 3]

    def run(conf):
        mean_buf = torch.full((S + 1 + GUARD, 8), CANARY, dtype=torch.float64, device="cuda:0")
        cov_buf = torch.full((S + 1 + GUARD, 8, 8), CANARY, dtype=torch.float64, device="cuda:0")
        feat_buf = torch.full((S + 1 + GUARD, width), CANARY, dtype=torch.float32, device="cuda:0")
        st = _fstore(capacity=S, E=width)
        st.mean, st.cov, st.feat = mean_buf[:S + 1], cov_buf[:S + 1], feat_buf[:S + 1]
        live = slots >= 0
        st.mean[_dev(slots[live]).long()], st.cov[_dev(slots[live]).long()] = _dev(mean[live]), _dev(cov[live])
        st.feat[:] = _dev(rows0)
        new, status = _raw_apply(st, slots, r2c, c2r, xyah, conf, dfeat, ALPHA, free)
        return new, status, mean_buf.cpu().numpy(), cov_buf.cpu().numpy(), feat_buf.cpu().numpy()
    new, status, mean_a, cov_a, feat_a = run(conf)
    want_new = np.full(m, -1, dtype=np.int32)
    want_new[births[:5]] = free
    want_new[births[5:]] = -2                                      # the free list is used up: reported, nothing written
    assert np.array_equal(new, want_new) and not status.any()
    # the composed route on a store loaded alike
    ref = _fstore(mean, cov, slots, capacity=S, E=width)
    ref.feat[:] = _dev(rows0)
    ref._det_feats = _dev(dfeat)
    pairs = [(int(slots[r]), int(r2c[r])) for r in range(n) if r2c[r] >= 0 and slots[r] >= 0]
    ustatus = ref.update([s for s, _ in pairs], xyah, [j for _, j in pairs], confidence=conf).cpu().numpy()
    started = [(int(s), j) for s, j in zip(free, births[:5]) if 0 <= s < S]
    ref.initiate([s for s, _ in started], xyah, [j for _, j in started])
    _ema_fit(ref, pairs, started)
    assert not ustatus.any() and len(pairs) == 7 and len(started) == 4
    rm, rc, rf = _all_of(ref)
    touched = [s for s, _ in pairs + started]
    assert np.array_equal(mean_a[touched], rm[touched]) and np.array_equal(cov_a[touched], rc[touched]) and np.array_equal(feat_a[:S + 1], rf)
    # unmatched rows, unlisted slots, the spare slot and the guard rows behind it: unchanged in every bit
    live = slots >= 0
    mean_i, cov_i = np.full((S + 1 + GUARD, 8), CANARY), np.full((S + 1 + GUARD, 8, 8), CANARY)
    mean_i[slots[live]], cov_i[slots[live]] = mean[live], cov[live]
    rest_of = np.ones(S + 1 + GUARD, dtype=bool)
    rest_of[touched] = False
    assert np.array_equal(mean_a[rest_of], mean_i[rest_of]) and np.array_equal(cov_a[rest_of], cov_i[rest_of])
    assert np.array_equal(feat_a[:S + 1][rest_of[:S + 1]], rows0[rest_of[:S + 1]]) and (feat_a[S + 1:] == CANARY).all()
    assert all(abs(np.linalg.norm(feat_a[s].astype(np.float64)) - 1.0) < 1e-6 for s in touched)
    again = run(conf)
    assert all(np.array_equal(x, y) for x, y in zip(again, (new, status, mean_a, cov_a, feat_a)))   # new_slot and every bit: the same over two runs
    # det_conf NULL: confidence 0
    _, _, mean_0, cov_0, feat_0 = run(None)
    ref0 = _fstore(mean, cov, slots, capacity=S, E=width)
    ref0.update([s for s, _ in pairs], xyah, [j for _, j in pairs])
    rm0, rc0, _ = _all_of(ref0)
    sl = [s for s, _ in pairs]
    assert np.array_equal(mean_0[sl], rm0[sl]) and np.array_equal(cov_0[sl], rc0[sl]) and np.array_equal(feat_0, feat_a)
    assert not np.array_equal(cov_0[sl], cov_a[sl])


@pytest.mark.gpu
def test_apply_writes_the_feature_of_a_track_whose_update_fails():
    g = gold()
    mean, cov = g["mean"][4:7].copy(), g["cov"][4:7].copy()
    cov[1, :4, :4] = -np.eye(4)
    slots = np.array([9, 2, 5], dtype=np.int32)
    rs = np.random.RandomState(1)
    rows0, dfeat = rs.normal(size=(25, E)).astype(np.float32), rs.normal(size=(3, E)).astype(np.float32)
    a, b = _fstore(mean, cov, slots, capacity=24), _fstore(mean, cov, slots, capacity=24)
    for st in (a, b):
        st.feat[:] = _dev(rows0)
    new, status = _raw_apply(a, slots, [2, 0, -1], [1, -1, 0], g["meas"][4:7], [0.4] * 3, dfeat, ALPHA, [])
    assert status.tolist() == [0, 1, 0] and new.tolist() == [-1, -2, -1]
    b._det_feats = _dev(dfeat)
    assert b.update(slots[:2], g["meas"][4:7], [2, 0], confidence=0.4).cpu().numpy().tolist() == [0, 1]
    _ema_fit(b, [(9, 2), (2, 0)], [])
    _same(_all_of(a), _all_of(b), "failed update")
    assert np.array_equal(_all_of(a)[1][2], cov[1]) and not np.array_equal(_all_of(a)[2][2], rows0[2])      # the state kept, the feature smoothed


# ---- GPU: frame() against the composed route ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [30, None])
@pytest.mark.parametrize("n,m", [(1, 1), (17, 65), (96, 40)])
def test_frame_equals_the_composed_route(ctx, n, m, depth):
    sc = Scene(n, m, 5 + n)
    mat = euclidean_warps()[2]
    for lam, warp in ((None, None), (0.98, mat), (None, mat), (0.98, None)):
        got = _agree(sc, sc.free[:6], depth, lam, warp, ctx, (n, m, depth, lam, warp is not None))
        print("frame %dx%d depth=%s MC=%s warp=%s: %d matches, %d + %d left, %d new, %d overflow" % (
            n, m, depth, lam, warp is not None, len(got.matches), len(got.unmatched_tracks), len(got.unmatched_detections), len(got.new_tracks),
            len(got.overflow)))
        if n >= 17:
            assert len(got.matches) >= 6 and got.unmatched_tracks and got.new_tracks
            if depth:
                assert all(sc.tsu[r] <= 30 for r, _ in got.matches if sc.confirmed[r])    # a track older than the cascade takes part in nothing
        if m == 65:
            assert got.overflow                                                        # more births than the six free slots
    # apply=False: the same matches, and the state is only advanced
    a, b = sc.store(), sc.store()
    dry = _frame(a, sc, sc.free[:6], depth, 0.98, mat, apply=False)
    wet = _frame(sc.store(), sc, sc.free[:6], depth, 0.98, mat)
    assert dry[:3] == wet[:3] and dry.new_tracks == [] and dry.overflow == []
    b.camera_update(sc.slots, mat)
    b.predict(sc.slots)
    _same(_all_of(a), _all_of(b), "apply=False")
    # predict=False: on states that are advanced already
    a, b = sc.store(), sc.store()
    for st in (a, b):
        st.predict(sc.slots)
    got = _frame(a, sc, sc.free[:6], depth, None, None, predict=False)
    want = _composed(b, sc, sc.free[:6], depth, None, None, ctx, predict=False)
    assert got.matches == want["matches"] and got.new_tracks == want["new_tracks"]
    _same(_all_of(a), _all_of(b), "predict=False")


@pytest.mark.gpu
def test_degenerate_frames(ctx):
    mat = euclidean_warps()[0]
    # no detections: only the advance happens, nothing is copied
    sc = Scene(17, 0, 1)
    got = _agree(sc, sc.free[:4], 30, 0.98, mat, ctx, "no detections")
    assert got == ([], list(range(17)), [], [], [])
    # no tracks: every detection starts a track, until the free list is used up
    sc = Scene(0, 9, 1)
    got = _agree(sc, sc.free[:4], 30, 0.98, None, ctx, "no tracks")
    assert got.matches == [] and got.unmatched_detections == list(range(9))
    assert got.new_tracks == [(j, int(s)) for j, s in zip(range(4), sc.free[:4])] and got.overflow == [4, 5, 6, 7, 8]
    got = _agree(sc, sc.free[:0], None, None, None, ctx, "no tracks, no free slot")
    assert got.new_tracks == [] and got.overflow == list(range(9))
    # neither
    st = Scene(0, 0, 1).store()
    assert st.frame([], [], [], np.zeros((0, 4)), None, np.zeros((0, E), dtype=np.float32), MAX_IOU, MATCH_THRESH, ALPHA) == ([], [], [], [], [])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [3, None])
def test_ties(ctx, depth):
    n, m = 17, 40
    sc = Scene(n, m, 3, tie=True)
    sc.tsu = np.where(np.arange(n) % 2 == 0, 1, 1 + np.arange(n) % 3)
    # the scene does tie: columns of both planes that are equal, bit for bit
    st = sc.store()
    st.predict(sc.slots)
    cost = RowMetric(st, ctx).distance(st._det_feats, [int(s) for s in sc.slots], device=True)
    gate = st.gate_cost(sc.slots, cost, sc.xyah, max_distance=MATCH_THRESH)[0].cpu().numpy()
    iou = st.iou_cost(sc.slots, sc.tlwh, max_distance=MAX_IOU).cpu().numpy()
    assert sum(np.array_equal(gate[:, j], gate[:, j + 1]) and np.array_equal(iou[:, j], iou[:, j + 1]) for j in range(m - 1)) >= m // 3
    assert len(np.unique(gate)) <= 8                               # the appearance costs lie on a coarse grid
    got = _agree(sc, sc.free[:8], depth, None, None, ctx, ("ties", depth))
    assert len(got.matches) >= 6 and got.new_tracks


@pytest.mark.gpu
def test_not_positive_definite(ctx):
    import torch
    sc = Scene(17, 20, 2)
    sc.tsu = np.ones(17, dtype=np.int64)
    bad_conf, bad_unc = 3, 4                                       # a confirmed row (gated) and an unconfirmed one (not gated)
    assert sc.confirmed[bad_conf] and not sc.confirmed[bad_unc]
    st = sc.store()
    st.cov[int(sc.slots[bad_unc]), :4, :4] = -torch.eye(4, dtype=torch.float64, device=st.dev)
    got = _frame(st, sc, sc.free[:4], 30, None, None, predict=False, apply=False)      # the gate never sees the unconfirmed track
    assert got.matches
    st.cov[int(sc.slots[bad_conf]), :4, :4] = -torch.eye(4, dtype=torch.float64, device=st.dev)
    with pytest.raises(np.linalg.LinAlgError, match="SortStore.frame: the projected covariance of track 3"):
        _frame(st, sc, sc.free[:4], 30, None, None, predict=False, apply=False)
    # an update that fails: the unconfirmed track is matched by the IoU stage (which reads only its mean), its update is flagged
    st = sc.store()
    st.predict(sc.slots)
    st.cov[int(sc.slots[bad_unc]), :4, :4] = -torch.eye(4, dtype=torch.float64, device=st.dev)
    before = _all_of(st)
    with pytest.raises(np.linalg.LinAlgError, match="SortStore.frame: update: the projected covariance of track 4"):
        _frame(st, sc, sc.free[:4], 30, None, None, predict=False)
    after = _all_of(st)
    s = int(sc.slots[bad_unc])
    assert np.array_equal(after[0][s], before[0][s]) and np.array_equal(after[1][s], before[1][s]) and not np.array_equal(after[2][s], before[2][s])
    assert not np.array_equal(after[1][int(sc.slots[0])], before[1][int(sc.slots[0])])         # the others were updated


@pytest.mark.gpu
def test_the_scripted_scene_replays_through_frame(ctx):
    """The 12-frame scene of tests/test_sort_store.py (births, a miss, a deletion whose slot is reused, two camera updates, confidences 0 and 0.999)
    through frame() with the host bookkeeping between frames, and through the calls of that test's replay on a second store, with the camera update
    before the prediction as the reference's loop has it (deep_sort_app.py:186-189): the matches of that test
    (its iou_round on all tracks - the tracks here are tentative throughout, so the IoU stage is their only one), the same states and feature rows
    after every frame."""
    frames, warps = _scene()
    W = 16
    a, b = _fstore(capacity=8, E=W), _fstore(capacity=8, E=W)
    tracks, free = [], list(range(8))[::-1]                        # host objects: slot, time_since_update
    rs = np.random.RandomState(77)
    seen = {"births": 0, "miss": 0, "deleted": 0, "reused": False, "camera": 0}
    freed = set()
    for f, (det, conf) in enumerate(frames, start=1):
        slots = np.array([t.slot for t in tracks], dtype=np.int64)
        n, m = len(tracks), len(det)
        for t in tracks:
            t.time_since_update += 1
        tsu = [t.time_since_update for t in tracks]
        feats = rs.normal(size=(m, W)).astype(np.float32)
        offer = free[::-1][:m]                                     # the slots the host would hand out, in the order it pops them
        got = a.frame(slots, tsu, [False] * n, det, conf, feats, 0.7, MATCH_THRESH, ALPHA, free_slots=offer, cascade_depth=30, camera_matrix=warps.get(f))
        # the replay of tests/test_sort_store.py on the second store
        if f in warps:                                             # the reference's order: the warp, then the prediction
            b.camera_update(slots, warps[f])
            seen["camera"] += 1
        b.predict(slots)
        want = b.iou_round(slots, det, 0.7, stale=np.array([x > 1 for x in tsu], dtype=bool))
        z = _xyah_of(det)
        if want[0]:
            assert not b.update(slots[[r for r, _ in want[0]]], z, [c for _, c in want[0]], confidence=conf).cpu().numpy().any()
        new = [free.pop() for _ in want[2]]
        b.initiate(new, z, want[2])
        b._det_feats = _dev(feats)
        _ema_fit(b, [(int(slots[r]), c) for r, c in want[0]], list(zip(new, want[2])))
        assert sorted(got.matches) == sorted((int(r), int(c)) for r, c in want[0]), f
        assert got.unmatched_tracks == sorted(int(r) for r in want[1]) and got.unmatched_detections == [int(j) for j in want[2]], f
        assert got.new_tracks == list(zip([int(j) for j in want[2]], new)) and got.overflow == [], f
        _same(_all_of(a), _all_of(b), f)
        # the host bookkeeping: hits, misses, deletion at the second miss in a row, births
        for r, _ in got.matches:
            tracks[r].time_since_update = 0
        for r in got.unmatched_tracks:
            seen["miss"] += 1
            if tracks[r].time_since_update >= 2:
                free.append(tracks[r].slot)
                freed.add(tracks[r].slot)
                tracks[r] = None
                seen["deleted"] += 1
        tracks = [t for t in tracks if t is not None]
        seen["reused"] |= bool(freed & set(new))
        tracks += [types.SimpleNamespace(slot=s, time_since_update=0) for s in new]
        seen["births"] += len(new)
    assert seen == {"births": 7, "miss": 2, "deleted": 1, "reused": True, "camera": 2} and len(tracks) == 6


@pytest.mark.gpu
def test_frame_makes_one_copy_home_after_the_filter_is_enqueued(ctx, monkeypatch):
    """Every route from a device tensor to the host is counted as tests/test_assign_stages.py counts them for match(): one frame() takes exactly one,
    and none has happened when busca_sframe_apply is enqueued."""
    import torch
    from busca_amd import _sframe_lib
    sc = Scene(17, 65, 22)
    st = sc.store()
    want = _composed(sc.store(), sc, sc.free[:6], 30, 0.98, None, ctx)
    lib = _sframe_lib.load()
    count = {"n": 0, "at_apply": None}

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
    real_apply = lib.busca_sframe_apply

    def apply(*a):
        count["at_apply"] = count["n"]
        return real_apply(*a)
    monkeypatch.setattr(lib, "busca_sframe_apply", apply)
    got = _frame(st, sc, sc.free[:6], 30, 0.98, None)
    copies = count["n"]
    monkeypatch.undo()
    assert count["at_apply"] == 0 and copies == 1
    assert got.matches == want["matches"] and got.new_tracks == want["new_tracks"] and len(got.matches) >= 6


@pytest.mark.gpu
def test_a_frame_behind_a_busy_stream(ctx, busy):
    from tests.test_streams_gpu import behind
    sc, other = Scene(17, 65, 22), Scene(17, 65, 99)
    full = lambda s: [_dev(x) for x in _all_of(s.store())]      # noqa: E731
    st = sc.store()
    mat = euclidean_warps()[2]

    def call(x, outs, stream):
        st.mean, st.cov, st.feat = x
        got = _frame(st, sc, sc.free[:6], 30, 0.98, mat)
        return [np.asarray(v, dtype=np.int64) for v in got]
    want, got = behind(busy, "SortStore.frame", call, true=full(sc), poison=full(other), form="current", host=True)
    assert len(got[3]) >= 6 and len(got[6]) >= 1                  # the frame matched and started tracks
    ref = sc.store()
    _composed(ref, sc, sc.free[:6], 30, 0.98, mat, ctx)
    _same(got[:3], _all_of(ref), "behind a busy stream")
