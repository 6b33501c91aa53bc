"""GHOST's frame on resident state as one chain: libbusca_gframe.so (include/busca_gframe.h), its binding busca_amd._gframe_lib and
GhostStore.frame.

The oracle is the set of calls this repository already pins, composed on a second GhostGallery + GhostMotion loaded alike: GhostMotion.compensate /
step, ghost_round, the host restatement of assign_act_inact_same_time / assign_separatly below (pinned to the reference's own functions by
tests/golden/ghost_assign.npz), tracking.linear_assignment for the second stage, GhostGallery.add and GhostMotion.add.  Every comparison is exact:
np.array_equal, NaN patterns compared by np.isnan.  No tolerance anywhere."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, BUDGET, HIST, CAP = 32, 4, 4, 64
PERM = np.random.RandomState(31).permutation(CAP)
LIMIT = 8192.0
_CACHE = {}


def gold():
    if "gold" not in _CACHE:
        _CACHE["gold"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "ghost_assign.npz")))
    return _CACHE["gold"]


# ---- the host restatement of the reference's filter ---------------------------------------------------------------------
def host_same_time(row, col, dist, num_active, thr):
    """assign_act_inact_same_time (tracker.py:611-633) on `dist` [detections, tracks], active tracks first -> the kept (detection, track) pairs in
    the reference's order.  The comparison is strict; a NaN cost or threshold keeps nothing."""
    return [(int(r), int(c)) for r, c in zip(row, col) if dist[r, c] < thr[0 if c < num_active else 1]]


def host_assign(row, col, dist, num_active, thr, sep, solve=None):
    """assign_act_inact_same_time, or with `sep` assign_separatly (tracker.py:637-682): `dist` [detections, tracks] (sep: the pair [dist_act,
    dist_inact or None]), (row, col) the matching of the whole matrix (sep: of the active block), `solve` the second stage's solve_dense.
    -> dict: pairs [(detection, track column of the whole matrix)] in the order the reference calls add_detection, assigned (sorted), and what the
    second stage saw: compact (its matrix, or None), row2 / col2, and wrote (the (index into tr_ids, track column) pairs it wrote - the reference
    writes them at the COMPACTED detection index, tracker.py:633 with the list of :674)."""
    res = dict(compact=None, row2=None, col2=None, wrote=[])
    if not sep:
        pairs = host_same_time(row, col, dist, num_active, thr)
        res.update(pairs=pairs, assigned=sorted(r for r, _ in pairs))
        return res
    d_act, d_inact = dist
    pairs = host_same_time(row, col, d_act, d_act.shape[1], thr)
    assigned = {r for r, _ in pairs}
    if d_inact is not None:
        u = sorted(set(range(d_act.shape[0])) - assigned)
        if len(u) != 0:
            compact = d_inact[u, :]
            row2, col2 = solve(compact)
            second = host_same_time(row2, col2, compact, 0, thr)
            pairs = pairs + [(u[r], num_active + c) for r, c in second]
            assigned |= {u[r] for r, _ in second}
            res.update(compact=compact, row2=np.asarray(row2), col2=np.asarray(col2), wrote=[(r, num_active + c) for r, c in second])
    res.update(pairs=pairs, assigned=sorted(assigned))
    return res


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    import importlib
    builder = importlib.import_module("busca_amd.build")
    hip_lib = builder.build()
    from busca_amd import _frame_lib, _gframe_lib, _lib, _mframe_lib, _msframe_lib, _rounds_lib, _sframe_lib, _sort_lib, _store_lib, _track_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "busca_gframe.h")).read(), flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_gframe_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _gframe_lib.GFRAME_API.items()}
    assert sorted(declared) == ["busca_gframe_advance", "busca_gframe_apply", "busca_gframe_cost", "busca_gframe_keep", "busca_gframe_last_error",
                                "busca_gframe_version"]
    assert int(re.search(r"#define\s+BUSCA_GFRAME_MAX_DETS\s+(\d+)", hdr).group(1)) == _gframe_lib.MAX_DETS == _sframe_lib.MAX_DETS
    assert int(re.search(r"#define\s+BUSCA_GFRAME_EINVAL\s+\((-\d+)\)", hdr).group(1)) == _gframe_lib.EINVAL

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_gframe_lib.GFRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_gframe_lib.GFRAME_API)
    others = [hip_lib, _track_lib.TRACK_LIB_PATH, _store_lib.STORE_LIB_PATH, _rounds_lib.ROUNDS_LIB_PATH, _sort_lib.SORT_LIB_PATH,
              _frame_lib.FRAME_LIB_PATH, _sframe_lib.SFRAME_LIB_PATH, _mframe_lib.MFRAME_LIB_PATH, _msframe_lib.MSFRAME_LIB_PATH]
    assert len({os.path.basename(p) for p in others}) == 9
    for other in others:                                                           # the build leaves all ten libraries, and no other exports ours
        assert os.path.exists(other), other
        theirs = {n for n in exported(other) if not n.startswith("_")}
        assert not [n for n in theirs if n.startswith("busca_gframe")], other
    assert {n for n in exported(_store_lib.STORE_LIB_PATH) if not n.startswith("_")} == set(_store_lib.STORE_API)      # it keeps its exports
    assert "busca_gframe.h" not in _lib.HEADERS
    assert builder.GFRAME_OUT == _gframe_lib.GFRAME_LIB_PATH and os.path.exists(builder.GFRAME_OUT + ".flags")
    lib = _gframe_lib.load()
    assert lib.busca_gframe_version() == 1000 and _gframe_lib.ABI_MAJOR == 1 and lib.busca_gframe_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _gframe_lib
    lib = _gframe_lib.load()
    P, ODD = 0x10000, 0x10004                            # an aligned address, one that is 4- but not 8-byte aligned
    nan = float("nan")

    def calls(hist=P, frames=P, count=P, newest=P, pos=P, vel=P, S=8, H=4, slot=P, n=5, n_step=3, na=2, last_n=3, diff32=0, warp=P, pos_out=P, app=P,
              boxes=P, m=7, alpha=0.4, tl=P, dl=P, thr=P, out=P, lo=0, hi=5, r2c=P, c2r=P, track_det=P, det_track=P, merge=0, mask_from=-1, gallery=P,
              g_count=P, g_newest=P, seen=P, budget=3, E=16, feat=P, frame=9, may=P, free=P, n_free=2, det_slot=P, dev=0):
        return {
            "busca_gframe_advance": lambda: lib.busca_gframe_advance(hist, frames, count, newest, pos, vel, S, H, slot, n, n_step, na, last_n, diff32, warp,
                                                                     pos_out, dev, None),
            "busca_gframe_cost": lambda: lib.busca_gframe_cost(app, pos, boxes, n, m, alpha, tl, dl, na, thr, out, dev, None),
            "busca_gframe_keep": lambda: lib.busca_gframe_keep(app, n, m, lo, hi, na, r2c, c2r, thr, track_det, det_track, merge, mask_from, dev, None),
            "busca_gframe_apply": lambda: lib.busca_gframe_apply(hist, frames, count, newest, pos, vel, H, gallery, g_count, g_newest, seen, budget, E, S, slot,
                                                                 n, track_det, det_track, feat, boxes, m, frame, may, free, n_free, det_slot, dev, None),
        }

    def refused(name, words, **kw):
        rc = calls(**kw)[name]()
        msg = lib.busca_gframe_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and words in msg, (name, kw, rc, msg)

    nothing = dict(hist=None, frames=None, count=None, newest=None, pos=None, vel=None, slot=None, warp=None, pos_out=None, app=None, boxes=None, tl=None,
                   dl=None, thr=None, out=None, r2c=None, c2r=None, track_det=None, det_track=None, gallery=None, g_count=None, g_newest=None, seen=None,
                   feat=None, may=None, free=None, det_slot=None)
    for name in calls():
        refused(name, "negative size", n=-1, n_step=0, na=0, hi=0)
        refused(name, "negative device", dev=-1)
    name = "busca_gframe_advance"
    for noop in (dict(n=0, n_step=0, na=0), dict(warp=None, n_step=0, na=0)):
        assert calls(**noop)[name]() == 0 and calls(**{**nothing, **noop})[name]() == 0, noop
    for size in ("S", "H"):
        refused(name, "negative size", **{size: -1})
    refused(name, "at least 2 rows", H=1)
    refused(name, "n_step 6 outside", n_step=6)
    refused(name, "num_active 4 outside", na=4)
    refused(name, "last_n_frames = 1", last_n=1)
    for ptr in ("hist", "frames", "count", "newest", "pos", "vel", "slot", "pos_out"):
        refused(name, "null pointer", **{ptr: None})
    for ptr in ("hist", "pos", "vel", "pos_out"):
        refused(name, "misaligned", **{ptr: ODD})
    for ptr in ("frames", "count", "newest", "slot", "warp"):
        refused(name, "misaligned", **{ptr: 0x10002})
    assert calls(pos_out=None, n_step=0, na=0, n=0)[name]() == 0
    name = "busca_gframe_cost"
    for noop in (dict(n=0, na=0), dict(m=0)):
        assert calls(**noop)[name]() == 0 and calls(**{**nothing, **noop})[name]() == 0, noop
    refused(name, "negative size", m=-1)
    refused(name, "alpha is NaN", alpha=nan)
    refused(name, "go together", tl=None)
    refused(name, "go together", dl=None)
    refused(name, "more workgroups than a grid holds", n=16 * 65535 + 1)
    refused(name, "null pointer (app and out", app=None)
    refused(name, "null pointer (app and out", out=None)
    refused(name, "null pointer (det_boxes with pos)", boxes=None)
    assert calls(pos=None, boxes=None, n=0, na=0)[name]() == 0
    for ptr in ("app", "pos", "boxes", "thr", "out"):
        refused(name, "misaligned", **{ptr: ODD})
    for ptr in ("tl", "dl"):
        refused(name, "misaligned", **{ptr: 0x10002})
    name = "busca_gframe_keep"
    for noop in (dict(m=0), dict(hi=0, merge=1)):
        assert calls(**noop)[name]() == 0 and calls(**{**nothing, **noop})[name]() == 0, noop
    refused(name, "negative size", m=-1)
    refused(name, "rows -1 .. 5 outside", lo=-1)
    refused(name, "rows 3 .. 2 outside", lo=3, hi=2)
    refused(name, "rows 0 .. 6 outside", hi=6)
    refused(name, "num_active 6 outside", na=6)
    refused(name, "mask_from 2 outside", hi=3, mask_from=2)
    refused(name, "mask_from 6 outside", hi=3, mask_from=6)
    for ptr in ("c2r", "det_track", "app", "r2c", "thr", "track_det"):
        refused(name, "null pointer", **{ptr: None})
    for ptr in ("app", "thr"):
        refused(name, "misaligned", **{ptr: ODD})
    for ptr in ("r2c", "c2r", "track_det", "det_track"):
        refused(name, "misaligned", **{ptr: 0x10002})
    name = "busca_gframe_apply"
    for noop in (dict(m=0),):
        assert calls(**noop)[name]() == 0 and calls(**{**nothing, **noop})[name]() == 0, noop
    for size in ("S", "m", "n_free", "H"):
        refused(name, "negative size", **{size: -1})
    refused(name, "one call takes 2048", m=2049)
    refused(name, "more workgroups than a grid holds", n=2 ** 31 - 1)
    refused(name, "at least 2 rows", H=1)
    refused(name, "at least 1 row of at least 1 value", E=0)
    refused(name, "at least 1 row of at least 1 value", budget=0)
    for ptr in ("hist", "frames", "count", "newest", "pos", "vel", "gallery", "g_count", "g_newest", "seen", "slot", "track_det", "det_track", "feat",
                "boxes", "may", "free", "det_slot"):
        refused(name, "null pointer", **{ptr: None})
    for ptr in ("hist", "pos", "vel", "boxes"):
        refused(name, "misaligned", **{ptr: ODD})
    for ptr in ("frames", "count", "newest", "gallery", "g_count", "g_newest", "slot", "track_det", "det_track", "feat", "free", "det_slot"):
        refused(name, "misaligned", **{ptr: 0x10002})
    refused(name, "misaligned", n=0, slot=None, track_det=None, hist=ODD)          # without rows the row operands may be NULL - the others are still judged
    refused(name, "null pointer", n=0, slot=None, track_det=None, det_slot=None)
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_gframe_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_gframe_last_error() != b""


DEFAULT = dict(avg_act={"do": False, "num": 2, "proxy": "each_sample"}, avg_inact={"do": True, "num": 2, "proxy": "each_sample"}, act_reid_thresh=0.55,
               inact_reid_thresh=0.5, nan_first=False, assign_separately=False, new_track_conf=0.6,
               motion_config={"apply_motion_model": True, "combi": "sum_0.4", "last_n_frames": 3})
CONFIGS = {
    "default": DEFAULT,
    "mv_avg": dict(DEFAULT, avg_act={"do": True, "num": 0.9, "proxy": "mv_avg"}, avg_inact={"do": True, "num": 0.8, "proxy": "mv_avg"}),
    "nan_first": dict(DEFAULT, nan_first=True),
    "separate": dict(DEFAULT, assign_separately=True),
    "every": dict(DEFAULT, act_reid_thresh="every", inact_reid_thresh="every", motion_config={"apply_motion_model": False}),
}


def test_python_level_checks(monkeypatch):
    """Duplicate or overlapping slot lists, listed free slots, shape mismatches and refused configs raise before any device work: the store is a
    shell without tensors and the library is never loaded."""
    import types
    import torch
    from busca_amd import _gframe_lib, ghost_store, tracking
    monkeypatch.setattr(_gframe_lib, "load", lambda: pytest.fail("device work before the checks"))
    monkeypatch.setattr(ghost_store, "h2d_async", lambda *a, **k: pytest.fail("an upload before the checks"))
    st = object.__new__(tracking.GhostStore)
    st.capacity, st.budget, st.E, st.history = CAP, BUDGET, E, HIST
    st.motion = types.SimpleNamespace(box32=False)
    st.gallery = types.SimpleNamespace(mv_avg=object(), mv_seen=object())
    feats, boxes = np.zeros((3, E), np.float32), np.zeros((3, 4))

    def frame(active=(1, 2), inactive=(3,), cfg=DEFAULT, feats=feats, boxes=boxes, **kw):
        return st.frame(active, inactive, feats, boxes, 5, cfg, **kw)
    for kw, words in ((dict(active=(1, 1)), "distinct"), (dict(inactive=(2,)), "distinct"), (dict(idle=(3,)), "distinct"), (dict(idle=(9, 9)), "distinct"),
                      (dict(active=(CAP,)), "beyond the capacity"), (dict(active=(-1,)), "negative"), (dict(free_slots=(-2,)), "negative"),
                      (dict(free_slots=(7, 7)), "distinct"), (dict(free_slots=(3,)), "free slot 3 is also listed"),
                      (dict(idle=(8,), free_slots=(8,)), "free slot 8 is also listed"), (dict(free_slots=(CAP,)), "beyond the capacity"),
                      (dict(feats=np.zeros((2, E), np.float32)), "features for 3 detections"), (dict(feats=np.zeros((3, E + 16), np.float32)), "features for"),
                      (dict(boxes=np.zeros((3, 5))), "[m,4]"), (dict(det_conf=[0.5]), "1 confidences for 3"),
                      (dict(labels=([0, 1], [0, 0, 0])), "2 track labels"), (dict(labels=([0, 1, 0], [0, 0])), "2 detection labels"),
                      (dict(warp=np.zeros(5, np.float32)), "[2,3] warp"), (dict(thresholds=np.zeros(2)), "thresholds is a contiguous device"),
                      (dict(active=torch.zeros(2, dtype=torch.int32)), "host slot lists")):
        with pytest.raises(ValueError, match=re.escape(words)):
            frame(**kw)
    with pytest.raises(ValueError, match="use_bism"):
        frame(cfg=dict(DEFAULT, use_bism=True))
    with pytest.raises(ValueError, match="distance"):
        frame(cfg=dict(DEFAULT, distance="euclidean"))
    with pytest.raises(ValueError, match="Kalman"):
        frame(cfg=dict(DEFAULT, kalman=True))
    for bad in ("center_only", "approximate"):
        with pytest.raises(ValueError, match=bad):
            frame(cfg=dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], **{bad: True})))
    with pytest.raises(NotImplementedError, match="combi"):
        frame(cfg=dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], combi="mult")))
    with pytest.raises(NotImplementedError, match="'mode'"):
        frame(cfg=dict(DEFAULT, avg_inact={"do": True, "num": 3, "proxy": "mode"}))
    with pytest.raises(ValueError, match="'mv_avg' takes a number"):
        frame(cfg=dict(DEFAULT, avg_inact={"do": True, "num": "all", "proxy": "mv_avg"}))
    with pytest.raises(ValueError, match="must be a number"):
        frame(cfg=dict(DEFAULT, act_reid_thresh="sometimes"))
    with pytest.raises(ValueError, match="last_n_frames"):
        frame(cfg=dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], last_n_frames=1)))
    st.E = 24
    with pytest.raises(ValueError, match="multiple of 16"):
        frame(feats=np.zeros((3, 24), np.float32))
    assert tracking.GhostStore is ghost_store.GhostStore and tracking.GhostFrame._fields[:3] == ("matches", "new", "overflow")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        from busca import tracking as alias
        assert alias.GhostStore is tracking.GhostStore
    finally:
        sys.path.remove(os.path.join(ROOT, "busca_amd", "compat"))


def test_fixture_and_the_host_restatement():
    """The host restatement reproduces the reference's own assign_act_inact_same_time / assign_separatly on every recorded call: assigned, tr_ids,
    active_tracks, the add_detection calls and - separate mode - the compacted matrix handed to the second solve."""
    g = gold()
    params = g["params"]
    assert len(params) >= 24 and set(params[:, 0]) == {0, 1}
    seen = dict(equal=0, nan=0, second=0, none=0)
    for k, (sep, m, na, ni) in enumerate(params):
        dist, row, col, ids, thr = g["dist_%d" % k], g["row_%d" % k], g["col_%d" % k], g["ids_%d" % k], g["thr_%d" % k]
        assert dist.shape == (m, na + ni) and len(ids) == na + ni
        seen["nan"] += int(np.isnan(dist).any())
        seen["equal"] += int(any(dist[r, c] == thr[0 if c < na else 1] for r, c in zip(row, col)))
        if sep:
            recorded = (g["row2_%d" % k], g["col2_%d" % k]) if g["second_%d" % k][0] else None
            res = host_assign(row, col, [dist[:, :na], dist[:, na:] if na > 0 else None], na, thr, True, solve=lambda d: recorded)
            assert (res["compact"] is not None) == bool(g["second_%d" % k][0]), k
            if res["compact"] is not None:
                assert same(res["compact"], g["compact_%d" % k]), k
                seen["second"] += 1
            seen["none"] += int(na == 0)
        else:
            res = host_assign(row, col, dist, na, thr, False)
        assert np.array_equal(res["assigned"], g["assigned_%d" % k]), k
        assert np.array_equal([ids[c] for _, c in res["pairs"]], g["active_%d" % k]), k
        tr_ids = np.full(m, -1, dtype=np.int64)
        first = res["pairs"][:len(res["pairs"]) - len(res["wrote"])]
        for r, c in first + res["wrote"]:
            tr_ids[r] = ids[c]
        assert np.array_equal(tr_ids, g["tr_ids_%d" % k]), k
        # add_detection: (track id, the detection)
        added = [(ids[c], r) for r, c in res["pairs"]]              # the second stage hands over the right detection of its compacted list
        assert np.array_equal(np.array(added, dtype=np.int64).reshape(-1, 2), g["added_%d" % k]), k
    assert seen["equal"] >= 6 and seen["nan"] >= 12 and seen["second"] >= 8 and seen["none"] >= 1, seen


# ---- GPU: helpers -------------------------------------------------------------------------------------------------------
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
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy()


def _where():
    import torch
    return 0, torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


MOTION_KEYS = ("hist", "frames", "count", "newest", "pos", "vel")
GALLERY_KEYS = ("_gallery", "_count", "_newest", "_mv_avg", "_mv_seen")


def motion_state(gm):
    return [_host(getattr(gm, k)) for k in MOTION_KEYS]


def gallery_state(gg):
    return [_host(getattr(gg, k)) for k in GALLERY_KEYS]


def assert_same_states(a, b, what):
    for k, x, y in zip(MOTION_KEYS + GALLERY_KEYS, a, b):
        assert same(x, y), (what, k)


def random_motion(ctx, S, H, seed, box32=False):
    """A GhostMotion whose rings are empty, hold one sample, are partly filled and have wrapped, in turn."""
    from busca_amd import tracking
    rs = np.random.RandomState(seed)
    gm = tracking.GhostMotion(S, H, box_dtype=np.float32 if box32 else np.float64, ctx=ctx)
    hist = rs.uniform(0, 600, (S, H, 4)).astype(np.float32).astype(np.float64)
    hist[:, :, 2:] += hist[:, :, :2] + 20
    count = np.array([(0, 1, 2, H, H, H - 1)[s % 6] for s in range(S)], dtype=np.int32)
    newest = np.where(count == H, rs.randint(0, H, S), np.maximum(count - 1, 0)).astype(np.int32)
    frames = np.zeros((S, H), dtype=np.int32)
    for s in range(S):
        for back in range(H):
            frames[s, (newest[s] - back) % H] = 40 - 2 * back - (s % 3) * (back > 1)
    gm.hist.copy_(_dev(hist)), gm.frames.copy_(_dev(frames)), gm.count.copy_(_dev(count)), gm.newest.copy_(_dev(newest))
    gm.pos.copy_(_dev(rs.uniform(0, 600, (S, 4)))), gm.vel.copy_(_dev(rs.uniform(-3, 3, (S, 4))))
    return gm


def clone_motion(ctx, gm):
    from busca_amd import tracking
    other = tracking.GhostMotion(gm.capacity, gm.history, box_dtype=np.float32 if gm.box32 else np.float64, ctx=ctx)
    for k in MOTION_KEYS:
        getattr(other, k).copy_(getattr(gm, k))
    other.all_warped = gm.all_warped
    return other


def clone_gallery(ctx, gg):
    from busca_amd import tracking
    other = tracking.GhostGallery(gg.capacity, gg.budget, gg.E, ctx=ctx)
    for k in GALLERY_KEYS:
        getattr(other, k).copy_(getattr(gg, k))
    return other


WARP = np.array([[1.002, -0.013, 3.25], [0.011, 0.997, -2.5]], dtype=np.float32)


# ---- GPU: the four calls -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("diff32", [0, 1])
@pytest.mark.parametrize("warped", [False, True], ids=["still", "warp"])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_advance_equals_warp_then_step(ctx, n, warped, diff32):
    """busca_gframe_advance against busca_ghost_motion_warp on the listed slots followed by busca_ghost_motion_step on the first n_step: rings
    empty, with one sample, partly filled and wrapped; a window shorter than the ring; slots that are only warped; a skipped slot."""
    from busca_amd import _gframe_lib
    S, H = 80, HIST
    a = random_motion(ctx, S, H, 5 + n)
    b = clone_motion(ctx, a)
    slots = np.random.RandomState(n).permutation(S)[:n].astype(np.int32)
    if n >= 3:
        slots[1] = -1                                              # skipped: touches no memory, a row of NaN
    n_step = n - n // 3
    na = n_step // 2 if n > 1 else 1
    before = motion_state(a)
    d_slot, d_warp = _dev(slots), _dev(WARP.reshape(6))
    out = _dev(np.full((n_step + 1, 4), 777.25))
    _gframe_lib.check(_gframe_lib.load().busca_gframe_advance(
        a.hist.data_ptr(), a.frames.data_ptr(), a.count.data_ptr(), a.newest.data_ptr(), a.pos.data_ptr(), a.vel.data_ptr(), S, H, d_slot.data_ptr(), n,
        n_step, na, 3, diff32, d_warp.data_ptr() if warped else None, out.data_ptr(), *_where()))
    if warped:
        b.compensate(WARP, slots)
    b.box32, b.all_warped = bool(diff32), False
    want = _host(b.step(slots[:n_step], na, 3))
    got = _host(out)
    assert same(got[:n_step], want) and (got[n_step] == 777.25).all()
    for k, x, y, z in zip(MOTION_KEYS, motion_state(a), motion_state(b), before):
        assert same(x, y), k
        live = slots[slots >= 0]
        rest = np.setdiff1d(np.arange(S), live)
        assert same(x[rest], z[rest]), k                           # untouched slots bit-identical
    if n >= 3:
        assert np.isnan(got[1]).all()
    if n == 65:
        assert not same(motion_state(a)[4], before[4]) and (not warped or not same(motion_state(a)[0], before[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (15, 63), (16, 64), (17, 65)])
def test_cost_equals_pairwise_then_combine(ctx, n, m):
    import torch
    from busca_amd import _gframe_lib, _lib, geometry, tracking
    rs = np.random.RandomState(100 * n + m)
    app = rs.uniform(0, 1, (n, m))
    app[rs.uniform(size=(n, m)) < 0.1] = np.nan
    pos = rs.uniform(0, 300, (n, 4))
    pos[:, 2:] += pos[:, :2]
    boxes = pos[rs.randint(0, n, m)] + rs.uniform(-6, 6, (m, 4))
    if n > 1:
        pos[0] = np.nan
    tl, dl = rs.randint(0, 2, n).astype(np.int32), rs.randint(0, 2, m).astype(np.int32)
    na = n // 2
    thr = np.array([0.55, 0.45])
    d_app, d_pos, d_boxes, d_tl, d_dl, d_thr = _dev(app), _dev(pos), _dev(boxes), _dev(tl), _dev(dl), _dev(thr)
    motion = geometry.pairwise(ctx, d_pos, d_boxes, _lib.PAIR_IOU_COST)
    lib = _gframe_lib.load()
    seen_nan = 0
    for blend in (False, True):
        for labels in (False, True):
            for nan_first in (False, True):
                want = _host(tracking.ghost_cost(d_app, motion if blend else None, 0.4, d_tl if labels else None, d_dl if labels else None, na,
                                                 d_thr if nan_first else None, ctx=ctx))
                for alias in (False, True):
                    buf = torch.full((n * m + 16,), 777.25, dtype=torch.float64, device=d_app.device)
                    out = buf[8:8 + n * m]
                    if alias:
                        out.copy_(d_app.view(-1))
                    src = out if alias else d_app
                    _gframe_lib.check(lib.busca_gframe_cost(src.data_ptr(), d_pos.data_ptr() if blend else None, d_boxes.data_ptr(), n, m, 0.4,
                                                            d_tl.data_ptr() if labels else None, d_dl.data_ptr() if labels else None, na,
                                                            d_thr.data_ptr() if nan_first else None, out.data_ptr(), *_where()))
                    got = _host(buf)
                    assert same(got[8:8 + n * m].reshape(n, m), want), (blend, labels, nan_first, alias)
                    assert (got[:8] == 777.25).all() and (got[8 + n * m:] == 777.25).all()
                seen_nan += int(np.isnan(want).sum() > np.isnan(app).sum())
    assert seen_nan >= (4 if n > 1 else 0)
    assert same(_host(d_app), app)


def np_keep(cost, lo, hi, na, r2c, c2r, thr, track_det, det_track, merge, mask_from):
    cost, track_det, det_track = cost.copy(), track_det.copy(), det_track.copy()
    n, m = cost.shape
    kept = []
    for r in range(hi - lo):
        j, i = r2c[r], lo + r
        ok = 0 <= j < m and c2r[j] == r and cost[i, j] < thr[0 if i < na else 1]
        track_det[i] = j if ok else -1
        if ok:
            kept.append((i, j))
    if not merge:
        det_track[:] = -1
    for i, j in kept:
        det_track[j] = i
        if mask_from >= 0:
            cost[mask_from:, j] = np.nan
    return cost, track_det, det_track, kept


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (15, 63), (16, 64), (17, 65)])
def test_keep_is_the_strict_filter(ctx, n, m):
    from busca_amd import _gframe_lib
    lib = _gframe_lib.load()
    rs = np.random.RandomState(7 * n + m)
    thr = np.array([0.5, 0.4])
    total = 0
    for lo, hi, mask_from, merge in ((0, n, -1, 0), (0, n // 2, n // 2, 0), (n // 2, n, -1, 1), (0, n, n, 0), (0, 0, -1, 0)):
        rows = hi - lo
        cost = rs.uniform(0, 1, (n, m))
        r2c = np.full(rows, -1, dtype=np.int32)
        c2r = np.full(m, -1, dtype=np.int32)
        cols = rs.permutation(m)[:rows]
        for r, j in enumerate(cols):
            if r % 5 != 4:                                         # an unmatched row now and then
                r2c[r], c2r[j] = j, r
        na = n // 3
        for r in range(rows):                                      # a cost equal to its threshold, one just below, a NaN cost
            if r2c[r] >= 0:
                t = thr[0 if lo + r < na else 1]
                cost[lo + r, r2c[r]] = (t, np.nextafter(t, 0), np.nan, cost[lo + r, r2c[r]])[r % 4]
        track_det, det_track = np.full(n + 2, -7, dtype=np.int32), rs.randint(0, n, m + 2).astype(np.int32)
        w_cost, w_td, w_dt, kept = np_keep(cost, lo, hi, na, r2c, c2r, thr, track_det[1:-1], det_track[1:-1], merge, mask_from)
        total += len(kept)
        d_cost, d_r2c, d_c2r, d_thr, d_td, d_dt = _dev(cost), _dev(np.append(r2c, 0).astype(np.int32)), _dev(c2r), _dev(thr), _dev(track_det), _dev(det_track)
        _gframe_lib.check(lib.busca_gframe_keep(d_cost.data_ptr(), n, m, lo, hi, na, d_r2c.data_ptr(), d_c2r.data_ptr(), d_thr.data_ptr(),
                                                d_td.data_ptr() + 4, d_dt.data_ptr() + 4, merge, mask_from, *_where()))
        what = (lo, hi, mask_from, merge)
        g_td, g_dt = _host(d_td), _host(d_dt)
        assert same(_host(d_cost), w_cost), what                   # nothing but the masked block is written
        assert np.array_equal(g_td[1:-1], w_td) and g_td[0] == g_td[-1] == -7, what
        assert np.array_equal(g_dt[1:-1], w_dt) and g_dt[0] == det_track[0] and g_dt[-1] == det_track[-1], what
        if mask_from < 0:
            assert same(w_cost, cost)
        if (lo, hi) == (0, n):                                     # a NaN threshold keeps nothing
            d_nan = _dev(np.array([np.nan, np.nan]))
            _gframe_lib.check(lib.busca_gframe_keep(d_cost.data_ptr(), n, m, lo, hi, na, d_r2c.data_ptr(), d_c2r.data_ptr(), d_nan.data_ptr(),
                                                    d_td.data_ptr() + 4, d_dt.data_ptr() + 4, 0, -1, *_where()))
            assert (_host(d_td)[1:-1] == -1).all() and (_host(d_dt)[1:-1] == -1).all()
    assert (n == 1) or total >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 63, 64, 65, 257, 512])
def test_apply_equals_ring_add_and_append(ctx, width):
    """busca_gframe_apply against GhostGallery.add + GhostMotion.add (busca_store_ring_add, busca_ghost_motion_append): matched rows, new tracks
    ranked in detection order, a skipped slot, the free list running out (-2, nothing written), untouched slots bit-identical."""
    from busca_amd import _gframe_lib, tracking
    S, H, budget, n, m = 24, 3, 3, 7, 11
    rs = np.random.RandomState(width)
    am = random_motion(ctx, S, H, 3)
    ag = tracking.GhostGallery(S, budget, width, ctx=ctx)
    ag._gallery.copy_(_dev(rs.standard_normal((S + 1, budget, width)).astype(np.float32)))
    ag._count.copy_(_dev(np.array([(0, 1, 2, 3, 5)[s % 5] for s in range(S + 1)], dtype=np.int32)))
    ag._newest.copy_(_dev(rs.randint(0, budget, S + 1).astype(np.int32)))
    ag._mv_seen.copy_(_dev(rs.randint(0, 2, S + 1).astype(np.uint8)))
    bm, bg = clone_motion(ctx, am), clone_gallery(ctx, ag)
    before = motion_state(am) + gallery_state(ag)
    perm = rs.permutation(S)
    slots = perm[:n].astype(np.int32)
    slots[2] = -1                                                  # a skipped track
    free = perm[n:n + 2].astype(np.int32)
    track_det = np.array([4, -1, 7, 0, 9, -1, 2], dtype=np.int32)
    det_track = np.full(m, -1, dtype=np.int32)
    for i, j in enumerate(track_det):
        if j >= 0:
            det_track[j] = i
    may = np.ones(m, dtype=np.uint8)
    may[3] = 0                                                     # unassigned: 1, 3, 5, 6, 8, 10; 3 may not start: 1 and 5 get the slots, 6, 8, 10 overflow
    feats = rs.standard_normal((m, width)).astype(np.float32)
    feats[4, 0] = np.nan                                           # the bits are copied, whatever they encode
    boxes = rs.uniform(0, 500, (m, 4))
    d_slot, d_free, d_td, d_dt, d_may, d_feats, d_boxes = (_dev(x) for x in (slots, free, track_det, det_track, may, feats, boxes))
    d_ds = _dev(np.full(m + 2, -7, dtype=np.int32))
    _gframe_lib.check(_gframe_lib.load().busca_gframe_apply(
        am.hist.data_ptr(), am.frames.data_ptr(), am.count.data_ptr(), am.newest.data_ptr(), am.pos.data_ptr(), am.vel.data_ptr(), H,
        ag._gallery.data_ptr(), ag._count.data_ptr(), ag._newest.data_ptr(), ag._mv_seen.data_ptr(), budget, width, S, d_slot.data_ptr(), n,
        d_td.data_ptr(), d_dt.data_ptr(), d_feats.data_ptr(), d_boxes.data_ptr(), m, 51, d_may.data_ptr(), d_free.data_ptr(), 2, d_ds.data_ptr() + 4,
        *_where()))
    rows = [i for i in range(n) if track_det[i] >= 0]
    bg.add(slots[rows], d_feats, det_index=track_det[rows])
    bm.add(slots[rows], d_boxes, 51, det_index=track_det[rows])
    bg.add(free, d_feats, det_index=[1, 5], new=[1, 1])
    bm.add(free, d_boxes, 51, det_index=[1, 5], new=[1, 1])
    want_slot = np.array([slots[3], free[0], slots[6], -1, slots[0], free[1], -2, -1, -2, slots[4], -2], dtype=np.int32)
    assert want_slot[7] == -1 and slots[2] == -1                   # detection 7 belongs to the skipped track: its slot as listed
    got = _host(d_ds)
    assert np.array_equal(got[1:-1], want_slot) and got[0] == got[-1] == -7
    after = motion_state(am) + gallery_state(ag)
    assert_same_states(after, motion_state(bm) + gallery_state(bg), width)
    touched = np.concatenate([slots[rows], free])
    touched = touched[touched >= 0]
    rest = np.setdiff1d(np.arange(S + 1), touched)
    for k, x, z in zip(MOTION_KEYS + GALLERY_KEYS, after, before):
        idx = rest[rest < len(x)]
        assert same(x[idx], z[idx]), k
    assert not same(after[6], before[6]) and _host(ag._mv_seen)[free].tolist() == [0, 0] and _host(am.vel)[free].any() == 0


# ---- GPU: the frame ------------------------------------------------------------------------------------------------------
class Scene:
    """n_act active, n_inact in-patience inactive and n_idle idle tracks in scattered slots of a store of CAP, each with 1 .. 6 samples (rings of 4:
    some wrap), and m detections: most sit on a track - its newest feature with a little noise, its box moved a little -, every 7th is a newcomer
    far from every track, with confidences on both sides of new_track_conf.  `tie`: integer boxes, features from a few axis vectors, detections in
    duplicate - whole columns of the cost matrix equal."""

    def __init__(self, n, m, seed, tie=False, n_idle=2, capacity=CAP):
        rs = np.random.RandomState(seed)
        self.n, self.m, self.seed, self.capacity = n, m, seed, capacity
        self.na = (n + 1) // 2
        total = n + n_idle
        assert total + 8 <= capacity
        perm = PERM if capacity == CAP else np.random.RandomState(32).permutation(capacity)
        slots = perm[:total]
        self.active, self.inactive, self.idle = [int(s) for s in slots[:self.na]], [int(s) for s in slots[self.na:n]], [int(s) for s in slots[n:]]
        self.free = [int(s) for s in perm[total:]]
        self.samples = []                                          # per track: [(frame, feature, box)]
        for t in range(total):
            base = np.zeros(E) if tie else rs.standard_normal(E)
            if tie:
                base[t % 5] = 1.0
            x, y = (40.0 * (t % 12), 60.0 * (t // 12)) if tie else rs.uniform(0, 900, 2)
            vx, vy = (2.0, 1.0) if tie else rs.uniform(-4, 4, 2)
            k = 1 + (t * 5 + seed) % 6
            hist = []
            for q in range(k):
                f = (base + (0 if tie else 0.15) * rs.standard_normal(E)).astype(np.float32)
                frame = 20 - 2 * (k - 1 - q) - (q % 2)
                hist.append((frame, f, np.array([x + vx * frame, y + vy * frame, x + vx * frame + 30, y + vy * frame + 70])))
            self.samples.append(hist)
        feats, boxes = np.zeros((m, E), np.float32), np.zeros((m, 4))
        order = rs.permutation(max(n, 1))
        for j in range(m):
            t = order[(j // 2 if tie else j) % max(n, 1)]
            if n == 0 or (j % 7 == 6 and not tie):
                feats[j] = rs.standard_normal(E)
                boxes[j] = np.array([1500 + 40 * j, 900, 1530 + 40 * j, 970])
            else:
                _, f, b = self.samples[t][-1]
                feats[j] = f + (0 if tie else 0.05) * rs.standard_normal(E).astype(np.float32)
                boxes[j] = b + (np.array([2.0, 1, 2, 1]) if tie else rs.uniform(-3, 3, 4))
        self.feats, self.boxes = feats, np.round(boxes) if tie else boxes
        self.conf = np.where(np.arange(m) % 3 == 0, 0.5, 0.9)
        self.tlabels = (np.arange(n) % 4 == 3).astype(np.int32)
        self.dlabels = (np.arange(m) % 5 == 4).astype(np.int32)

    def store(self, ctx):
        from busca_amd import tracking
        st = tracking.GhostStore(self.capacity, BUDGET, E, HIST, ctx=ctx)
        slots = self.active + self.inactive + self.idle
        for q in range(6):
            who = [t for t in range(len(slots)) if q < len(self.samples[t])]
            if not who:
                break
            by_frame = {}
            for t in who:
                by_frame.setdefault(self.samples[t][q][0], []).append(t)
            for frame, ts in sorted(by_frame.items()):
                s = [slots[t] for t in ts]
                st.gallery.add(s, np.stack([self.samples[t][q][1] for t in ts]), new=[q == 0] * len(ts))
                st.motion.add(s, np.stack([self.samples[t][q][2] for t in ts]), frame, new=[q == 0] * len(ts))
        for t, s in enumerate(slots):                              # a stored velocity for the inactive tracks
            if t >= self.na:
                st.motion.vel[s] = _dev(np.array([1.5, -0.5, 1.5, -0.5]))
        return st


def clone_store(ctx, st):
    from busca_amd import tracking
    other = tracking.GhostStore(st.capacity, st.budget, st.E, st.history, ctx=ctx)
    for k in GALLERY_KEYS:
        getattr(other.gallery, k).copy_(getattr(st.gallery, k))
    for k in MOTION_KEYS:
        getattr(other.motion, k).copy_(getattr(st.motion, k))
    other.motion.all_warped = st.motion.all_warped
    return other


def store_state(st):
    return motion_state(st.motion) + gallery_state(st.gallery)


def composed(ctx, st, active, inactive, idle, feats, boxes, frame, cfg, conf, free, labels=None, warp=None):
    """Tracker._track on `st` by the calls this repository already pins, with the host between them -> the fields of a GhostFrame as a dict."""
    import torch
    from busca_amd import tracking
    active, inactive, idle, free = list(active), list(inactive), list(idle), list(free)
    na, n, m = len(active), len(active) + len(inactive), len(feats)
    listed = active + inactive + idle
    if warp is not None and listed:
        st.motion.compensate(warp, listed)
    if warp is not None:
        st.motion.all_warped = True                                # the listed slots are all the live ones
    res = dict(matches=[], new=[], overflow=[], unassigned_active=list(range(na)), unassigned_inactive=list(range(na, n)), thresholds=None)
    if m == 0:
        return res
    d_feats, sep = _dev(feats), bool(cfg.get("assign_separately", False))
    pairs = []
    if n > 0:
        mcfg = cfg.get("motion_config", {})
        state = st.gallery.state(active, inactive, motion=st.motion)
        thr_t = torch.full((2,), float("inf"), dtype=torch.float64, device=d_feats.device)
        dist, row, col = tracking.ghost_round(state, d_feats, labels=labels, cfg=cfg, thresholds=thr_t, det_boxes=boxes, ctx=ctx)
        if mcfg.get("apply_motion_model", False) and idle:
            st.motion.step(idle, 0, mcfg.get("last_n_frames", 100000000))       # motion_step of the inactive tracks beyond patience
        fixed = [float("inf") if isinstance(v, str) or v is None else float(v) for v in (cfg.get("act_reid_thresh"), cfg.get("inact_reid_thresh"))]
        thr = _host(thr_t) if any(isinstance(cfg.get(k), str) for k in ("act_reid_thresh", "inact_reid_thresh")) or cfg.get("nan_first") else np.array(fixed)
        res["thresholds"] = tuple(float(x) for x in thr)

        def solve(compact):                                        # [detections left, inactive tracks]
            mt, _, _ = tracking.linear_assignment(_dev(np.ascontiguousarray(compact.T)), LIMIT, ctx=ctx)
            mt = sorted((int(d), int(t)) for t, d in mt)
            return [d for d, _ in mt], [t for _, t in mt]
        host = [_host(dist[0]), None if dist[1] is None else _host(dist[1])] if sep else _host(dist)
        pairs = host_assign(row, col, host, na, thr, sep, solve)["pairs"]
        res["dist"] = host
    slots = active + inactive
    if pairs:
        s, d = [slots[c] for _, c in pairs], [r for r, _ in pairs]
        st.gallery.add(s, d_feats, det_index=d)
        st.motion.add(s, boxes, frame, det_index=d)
    assigned = {r for r, _ in pairs}
    may = np.ones(m, bool) if (n == 0 or conf is None) else np.asarray(conf) > cfg["new_track_conf"]
    starts = [j for j in range(m) if j not in assigned and may[j]]
    born, res["overflow"] = starts[:len(free)], starts[len(free):]
    if born:
        st.gallery.add(free[:len(born)], d_feats, det_index=born, new=[1] * len(born))
        st.motion.add(free[:len(born)], boxes, frame, det_index=born, new=[1] * len(born))
    res["matches"] = sorted((c, r) for r, c in pairs)
    res["new"] = list(zip(born, free[:len(born)]))
    taken = {c for _, c in pairs}
    res["unassigned_active"] = [i for i in range(na) if i not in taken]
    res["unassigned_inactive"] = [i for i in range(na, n) if i not in taken]
    return res


def assert_frame(got, want, what):
    for k in ("matches", "new", "overflow", "unassigned_active", "unassigned_inactive"):
        assert list(getattr(got, k)) == list(want[k]), (what, k, getattr(got, k), want[k])
    if want["thresholds"] is not None:
        assert same(np.array(got.thresholds), np.array(want["thresholds"])), (what, got.thresholds, want["thresholds"])


def both_routes(ctx, sc, cfg, warp=None, free=None, labels=True, what=None, sc_args=None):
    st = sc.store(ctx)
    ref = clone_store(ctx, st)
    free = sc.free[:6] if free is None else free
    lab = (sc.tlabels, sc.dlabels) if labels else None
    got = st.frame(sc.active, sc.inactive, sc.feats, sc.boxes, 23, cfg, det_conf=sc.conf, idle=sc.idle, free_slots=free, labels=lab, warp=warp)
    want = composed(ctx, ref, sc.active, sc.inactive, sc.idle, sc.feats, sc.boxes, 23, cfg, sc.conf, free, labels=lab, warp=warp)
    assert_frame(got, want, what)
    assert_same_states(store_state(st), store_state(ref), what)
    assert st.motion.all_warped == ref.motion.all_warped, what
    return got, want, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("n,m", [(1, 1), (17, 65), (96, 40)])
def test_frame_equals_the_composed_route(ctx, n, m, name):
    sc = Scene(n, m, 11 * n + m, capacity=128 if n > 50 else CAP)          # 96 tracks need more than the 64 slots of the other scenes
    if name == "every":                                            # a class-masked entry makes update_thresholds' mean NaN, in the reference too: nothing is kept
        got, _, _ = both_routes(ctx, sc, CONFIGS[name], warp=WARP, what=(n, m, name, "labels"))
        assert n == 1 or (got.matches == [] and np.isnan(got.thresholds).all())
    got, want, _ = both_routes(ctx, sc, CONFIGS[name], warp=WARP if name != "mv_avg" else None, labels=name != "every", what=(n, m, name))
    if n > 1:
        assert len(got.matches) >= min(n, m) // 3, (n, m, name)
        assert got.new and (m < 60 or got.overflow)
    if "dist" in want:                                             # the device matrix, in ghost_round's orientation
        gd = got.dist if isinstance(got.dist, list) else [got.dist]
        wd = want["dist"] if isinstance(want["dist"], list) else [want["dist"]]
        assert same(_host(gd[0]), wd[0]), (n, m, name)


@pytest.mark.gpu
def test_degenerate_frames(ctx):
    """No detections: the warp happens, no step, nothing is copied.  No track to match: every detection starts a track whatever its confidence, no
    step.  The separate mode without active tracks never matches an inactive track.  No free slot: every start overflows, nothing is written."""
    import torch
    sc = Scene(9, 12, 3)
    # m == 0
    st = sc.store(ctx)
    ref = clone_store(ctx, st)
    count = {"n": 0}
    orig = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (count.__setitem__("n", count["n"] + 1), orig(self, *a, **k))[1]
    try:
        got = st.frame(sc.active, sc.inactive, np.zeros((0, E), np.float32), np.zeros((0, 4)), 23, DEFAULT, idle=sc.idle, warp=WARP)
    finally:
        torch.Tensor.cpu = orig
    assert count["n"] == 0 and got.matches == [] and got.unassigned_active == list(range(sc.na)) and got.dist is None
    before = store_state(ref)
    ref.motion.compensate(WARP, sc.active + sc.inactive + sc.idle)
    assert_same_states(store_state(st), store_state(ref), "m == 0")
    assert st.motion.all_warped and same(store_state(st)[4], before[4]) and not same(store_state(st)[0], before[0])      # pos as it was: no step
    # n == 0: only idle tracks
    st = sc.store(ctx)
    ref = clone_store(ctx, st)
    everyone = sc.active + sc.inactive + sc.idle
    got = st.frame([], [], sc.feats, sc.boxes, 23, DEFAULT, det_conf=np.zeros(sc.m), idle=everyone, free_slots=sc.free[:20], warp=WARP)
    want = composed(ctx, ref, [], [], everyone, sc.feats, sc.boxes, 23, DEFAULT, np.zeros(sc.m), sc.free[:20], warp=WARP)
    assert_frame(got, want, "n == 0")
    assert [j for j, _ in got.new] == list(range(sc.m)) and got.dist is None
    assert_same_states(store_state(st), store_state(ref), "n == 0")
    # the separate mode without active tracks
    sep = CONFIGS["separate"]
    st = sc.store(ctx)
    ref = clone_store(ctx, st)
    inactive = sc.active + sc.inactive
    got = st.frame([], inactive, sc.feats, sc.boxes, 23, sep, det_conf=sc.conf, idle=sc.idle, free_slots=sc.free[:20])
    want = composed(ctx, ref, [], inactive, sc.idle, sc.feats, sc.boxes, 23, sep, sc.conf, sc.free[:20])
    assert_frame(got, want, "separate, no active")
    assert got.matches == [] and got.unassigned_inactive == list(range(sc.n)) and got.dist[1] is None and got.new
    assert_same_states(store_state(st), store_state(ref), "separate, no active")
    # no free slot
    got, want, st = both_routes(ctx, sc, DEFAULT, free=[], what="no free slot")
    assert got.new == [] and got.overflow and got.matches


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "separate"])
def test_ties_give_the_composed_route_s_pairs(ctx, name):
    sc = Scene(14, 24, 5, tie=True)
    got, want, _ = both_routes(ctx, sc, CONFIGS[name], labels=False, what=("ties", name))
    assert len(got.matches) >= 6
    cost = _host(got.dist[0] if name == "separate" else got.dist)
    assert any(same(cost[j], cost[j + 1]) for j in range(0, sc.m - 1, 2))          # duplicated detections: equal rows of [detections, tracks]


@pytest.mark.gpu
def test_a_cost_equal_to_its_threshold_in_the_separate_mode(ctx):
    """The filter is `<` while nan_first is `<=`: the active stage matches the pair but does not assign it, and the detection stays available to the
    inactive tracks - here a twin of the active track takes it."""
    sc = Scene(8, 6, 17, n_idle=0)
    t_act, t_in = 0, sc.na                                         # the first active and the first inactive track
    sc.samples[t_in] = [(f, feat.copy(), box.copy()) for f, feat, box in sc.samples[t_act]]
    j = next(j for j in range(sc.m) if np.abs(sc.boxes[j] - sc.samples[t_act][-1][2]).max() < 4)
    cfg = dict(CONFIGS["separate"], nan_first=True)
    probe = sc.store(ctx).frame(sc.active, sc.inactive, sc.feats, sc.boxes, 23, cfg, det_conf=sc.conf, free_slots=sc.free[:6], apply=False)
    assert (t_act, j) in probe.matches
    edge = float(_host(probe.dist[0])[j, t_act])
    cfg = dict(cfg, act_reid_thresh=edge)
    got, want, _ = both_routes(ctx, sc, cfg, labels=False, what="edge")
    assert float(_host(got.dist[0])[j, t_act]) == edge             # nan_first keeps it: <=
    assert (t_act, j) not in got.matches and (t_in, j) in got.matches and t_act in got.unassigned_active
    same_time = dict(cfg, assign_separately=False)
    got, want, _ = both_routes(ctx, sc, same_time, labels=False, what="edge, same time")
    assert (t_act, j) not in got.matches


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "mv_avg"])
def test_a_scripted_scene_through_both_routes(ctx, name):
    """14 frames with the host bookkeeping of Tracker: tracks go inactive, are found again, expire into `idle`, are released and new tracks are born
    into released slots, with a warp on some frames.  The state of both routes is equal after every frame."""
    from busca_amd import tracking
    cfg, patience = CONFIGS[name], 2
    rs = np.random.RandomState(77)
    st = tracking.GhostStore(CAP, BUDGET, E, HIST, ctx=ctx)
    ref = tracking.GhostStore(CAP, BUDGET, E, HIST, ctx=ctx)
    people = []                                                    # (base feature, x, y, vx, vy, first frame, hidden frames)
    for p in range(12):
        hidden = {0: (), 1: (4, 5), 2: range(5, 40), 3: (6,), 4: range(3, 40), 5: (7, 8, 9)}.get(p % 6, ())
        people.append((rs.standard_normal(E), 80.0 * p, 50.0 * (p % 3), rs.uniform(-3, 3), rs.uniform(-2, 2), 0 if p < 8 else 8 + (p - 8), set(hidden)))
    active, inactive, free = [], {}, [int(s) for s in PERM[:14]]
    seen = dict(found=0, idle=0, released=0, reborn=0, warped=0)
    released = set()
    for frame in range(14):
        vis = [p for p, q in enumerate(people) if q[5] <= frame and frame not in q[6]]
        feats = np.stack([people[p][0] + 0.1 * rs.standard_normal(E) for p in vis]).astype(np.float32)
        boxes = np.stack([np.array([q[1] + q[3] * frame, q[2] + q[4] * frame, q[1] + q[3] * frame + 30, q[2] + q[4] * frame + 70]) + rs.uniform(-1, 1, 4)
                          for q in (people[p] for p in vis)])
        conf = np.full(len(vis), 0.9)
        warp = WARP if frame in (3, 7, 8) else None
        seen["warped"] += warp is not None
        curr = [s for s, c in inactive.items() if c <= patience]
        idle = [s for s, c in inactive.items() if c > patience]
        seen["idle"] += bool(idle)
        got = st.frame(active, curr, feats, boxes, frame, cfg, det_conf=conf, idle=idle, free_slots=free, warp=warp)
        want = composed(ctx, ref, active, curr, idle, feats, boxes, frame, cfg, conf, free, warp=warp)
        assert_frame(got, want, frame)
        assert_same_states(store_state(st), store_state(ref), frame)
        assert st.motion.all_warped == ref.motion.all_warped
        rows = active + curr
        hit = {rows[i] for i, _ in got.matches}
        seen["found"] += sum(1 for i, _ in got.matches if i >= len(active))
        for s in rows:
            if s in hit:
                inactive.pop(s, None)
            elif s in active:
                inactive[s] = 0
        active = [s for s in active if s in hit] + [s for s in curr if s in hit] + [s for _, s in got.new]
        seen["reborn"] += sum(1 for _, s in got.new if s in released)
        free = [s for s in free if s not in {s for _, s in got.new}]
        for s in list(inactive):
            inactive[s] += 1
            if inactive[s] > patience + 2:                         # gone: the slot goes back to the free list, at its front
                del inactive[s]
                for gallery in (st.gallery, ref.gallery):
                    gallery.release([s])
                free.insert(0, s)
                released.add(s)
                seen["released"] += 1
    assert seen["found"] >= 2 and seen["idle"] >= 2 and seen["released"] >= 1 and seen["reborn"] >= 1 and seen["warped"] == 3, seen
    assert int(_host(st.gallery.count).max()) == BUDGET and int(_host(st.motion.count).max()) == HIST       # the rings wrapped


@pytest.mark.gpu
def test_frame_makes_one_copy_home_after_the_apply_is_enqueued(ctx, monkeypatch):
    """Every route from a device tensor to the host is counted: one frame() takes exactly one, and none has happened when busca_gframe_apply is
    enqueued - in the separate mode too, with its two solves."""
    import torch
    from busca_amd import _gframe_lib
    sc = Scene(17, 65, 22)
    lib = _gframe_lib.load()
    for name in ("default", "separate", "every"):
        st = sc.store(ctx)
        want = composed(ctx, clone_store(ctx, st), sc.active, sc.inactive, sc.idle, sc.feats, sc.boxes, 23, CONFIGS[name], sc.conf, sc.free[:6], warp=WARP)
        d_feats = _dev(sc.feats)
        count = {"n": 0, "at_apply": None, "calls": 0}
        with monkeypatch.context() as mp:
            def counted(attr):
                orig = getattr(torch.Tensor, attr)

                def f(self, *a, **k):
                    to_host = attr != "to" or any(str(x).startswith("cpu") for x in list(a) + list(k.values()) if isinstance(x, (str, torch.device)))
                    if self.is_cuda and to_host:
                        count["n"] += 1
                    return orig(self, *a, **k)
                mp.setattr(torch.Tensor, attr, f)
            for attr in ("cpu", "item", "tolist", "numpy", "to"):
                counted(attr)
            real_apply = lib.busca_gframe_apply

            def apply(*a):
                count["at_apply"], count["calls"] = count["n"], count["calls"] + 1
                return real_apply(*a)
            mp.setattr(lib, "busca_gframe_apply", apply)
            got = st.frame(sc.active, sc.inactive, d_feats, sc.boxes, 23, CONFIGS[name], det_conf=sc.conf, idle=sc.idle, free_slots=sc.free[:6], warp=WARP)
            copies = count["n"]
        assert count["at_apply"] == 0 and count["calls"] == 1 and copies == 1, (name, count)
        assert_frame(got, want, name)
        assert len(got.matches) >= 6


@pytest.mark.gpu
def test_a_frame_behind_a_busy_stream(ctx, busy):
    from tests.test_streams_gpu import behind
    sc, other = Scene(17, 65, 22), Scene(17, 65, 99)
    st, poison = sc.store(ctx), other.store(ctx)
    tensors = lambda s: [getattr(s.motion, k) for k in MOTION_KEYS] + [getattr(s.gallery, k) for k in GALLERY_KEYS]      # noqa: E731
    true = [t.clone() for t in tensors(st)]
    cfg = CONFIGS["separate"]

    def call(x, outs, stream):
        st.motion.all_warped = False
        got = st.frame(sc.active, sc.inactive, sc.feats, sc.boxes, 23, cfg, det_conf=sc.conf, idle=sc.idle, free_slots=sc.free[:6], warp=WARP)
        return [np.asarray(v, dtype=np.int64).reshape(-1) for v in (got.matches, got.new, got.overflow, got.unassigned_active, got.unassigned_inactive)]
    want, got = behind(busy, "GhostStore.frame", call, true=true, poison=tensors(poison), x=tensors(st), form="current", host=True)
    k = len(true)
    assert len(got[k]) >= 12 and len(got[k + 1]) >= 2
    ref = sc.store(ctx)
    composed(ctx, ref, sc.active, sc.inactive, sc.idle, sc.feats, sc.boxes, 23, cfg, sc.conf, sc.free[:6], warp=WARP)
    assert_same_states(got[:k], store_state(ref), "behind a busy stream")
