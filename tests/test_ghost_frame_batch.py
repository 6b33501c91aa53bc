"""GHOST frames of many sequences on one store as one chain: libbusca_mgframe.so (include/busca_mgframe.h), its binding busca_amd._mgframe_lib and
GhostStore.frame_batch.

The oracle of every raw call is its single-problem counterpart (busca_gframe_*, busca_ghost_distance, busca_ghost_thresholds), problem by problem;
the oracle of frame_batch is GhostStore.frame per problem on a store loaded alike whose motion.all_warped was set to the problem's.  Every
comparison is exact: np.array_equal, NaN patterns compared by np.isnan.  No tolerance anywhere: the batched kernels run the same device functions."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests.test_ghost_frame import (BUDGET, CAP, CONFIGS, DEFAULT, E, GALLERY_KEYS, HIST, MOTION_KEYS, WARP, Scene, _dev, _host, _where,  # noqa: F401
                                    assert_same_states, busy, clone_gallery, clone_motion, ctx, random_motion, same, store_state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 777.25
WORDS = 13


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    import importlib
    builder = importlib.import_module("busca_amd.build")
    hip_lib = builder.build()
    from busca_amd import _gframe_lib, _lib, _mgframe_lib, _msframe_lib, _store_lib
    text = open(os.path.join(ROOT, "include", "busca_mgframe.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {}
    for name, args in re.findall(r"\b(busca_mgframe_[a-z0-9_]+)\s*\((.*?)\)\s*;", hdr, flags=re.S):
        declared[name] = 0 if args.strip() == "void" else len(args.split(","))
    assert declared == {name: len(args) for name, (_, args) in _mgframe_lib.MGFRAME_API.items()}
    assert sorted(declared) == ["busca_mgframe_advance", "busca_mgframe_apply", "busca_mgframe_cost", "busca_mgframe_distance", "busca_mgframe_keep",
                                "busca_mgframe_last_error", "busca_mgframe_thresholds", "busca_mgframe_version"]

    def define(name):
        return int(re.search(r"#define\s+BUSCA_MGFRAME_%s\s+\(?(-?\d+)\)?" % name, hdr).group(1))
    assert define("MAX_DETS") == _mgframe_lib.MAX_DETS == _gframe_lib.MAX_DETS and define("MAX_BATCH") == _mgframe_lib.MAX_BATCH == _msframe_lib.MAX_BATCH
    assert define("PROBLEM_WORDS") == _mgframe_lib.PROBLEM_WORDS == WORDS and define("EINVAL") == _mgframe_lib.EINVAL
    assert (define("DIFF32"), define("STEP")) == (_mgframe_lib.DIFF32, _mgframe_lib.STEP) and define("MAX_ROWS") == _mgframe_lib.MAX_ROWS
    assert (define("E_MIN"), define("E_MAX"), define("MEDIAN_BUDGET_MAX")) == (_mgframe_lib.E_MIN, _mgframe_lib.E_MAX, _mgframe_lib.MEDIAN_BUDGET_MAX)
    assert "this header is version 1000" in text

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    ours = {n for n in exported(_mgframe_lib.MGFRAME_LIB_PATH) if not n.startswith("_")}
    assert ours == set(_mgframe_lib.MGFRAME_API)
    for other in (hip_lib, _gframe_lib.GFRAME_LIB_PATH, _store_lib.STORE_LIB_PATH, _msframe_lib.MSFRAME_LIB_PATH):
        assert not [n for n in exported(other) if n.startswith("busca_mgframe")], other
    assert {n for n in exported(_gframe_lib.GFRAME_LIB_PATH) if not n.startswith("_")} == set(_gframe_lib.GFRAME_API)      # it keeps its exports
    assert "busca_mgframe.h" not in _lib.HEADERS
    assert builder.MGFRAME_OUT == _mgframe_lib.MGFRAME_LIB_PATH and os.path.exists(builder.MGFRAME_OUT + ".flags")
    lib = _mgframe_lib.load()
    assert lib.busca_mgframe_version() == 1000 and _mgframe_lib.ABI_MAJOR == 1 and lib.busca_mgframe_last_error() is not None


def test_refusals_and_noops_need_no_gpu():
    """Every argument is checked before the first HIP call: the pointers below are never followed."""
    from busca_amd import _mgframe_lib
    lib = _mgframe_lib.load()
    P, ODD = 0x10000, 0x10004                            # an aligned address, one that is 4- but not 8-byte (nor 16-byte) aligned
    nan = float("nan")
    base = dict(hist=P, frames=P, count=P, newest=P, pos=P, vel=P, S=8, H=4, slot=P, n_total=10, m_total=12, f_total=3, warps=P, n_warps=1, problems=P,
                batch=2, N=5, M=7, L=6, R=5, inact_row=-1, last_n=3, pos_out=P, gallery=P, g_count=P, rows=8, by_list=0, budget=3, dets=P, E=16, reduce=0,
                groups=3, out=P, cost=P, k_act=0.5, k_inact=1.0, which=3, thr=P, boxes=P, alpha=0.4, tl=P, dl=P, r2c=P, c2r=P, track_det=P, det_track=P,
                stage=0, merge=0, mask=0, g_newest=P, seen=P, feat=P, may=P, free=P, det_slot=P, dev=0)

    def call(name, **kw):
        a = dict(base, **kw)
        tail = (a["S"], a["slot"], a["n_total"], a["m_total"], a["f_total"], a["n_warps"], a["problems"], a["batch"], a["N"], a["M"], a["L"], a["R"],
                a["inact_row"])
        if name == "advance":
            return lib.busca_mgframe_advance(a["hist"], a["frames"], a["count"], a["newest"], a["pos"], a["vel"], a["S"], a["H"], a["slot"], a["n_total"],
                                             a["m_total"], a["f_total"], a["warps"], a["n_warps"], a["problems"], a["batch"], a["N"], a["M"], a["L"], a["R"],
                                             a["inact_row"], a["last_n"], a["pos_out"], a["dev"], None)
        if name == "distance":
            return lib.busca_mgframe_distance(a["gallery"], a["g_count"], a["rows"], a["by_list"], a["budget"], a["dets"], a["E"], a["reduce"], a["groups"],
                                              *tail, a["out"], a["dev"], None)
        if name == "thresholds":
            return lib.busca_mgframe_thresholds(a["cost"], a["k_act"], a["k_inact"], a["which"], *tail, a["thr"], a["dev"], None)
        if name == "cost":
            return lib.busca_mgframe_cost(a["cost"], a["pos"], a["boxes"], a["alpha"], a["tl"], a["dl"], a["thr"], *tail, a["dev"], None)
        if name == "keep":
            return lib.busca_mgframe_keep(a["cost"], a["r2c"], a["c2r"], a["thr"], a["track_det"], a["det_track"], a["stage"], a["merge"], a["mask"], *tail,
                                          a["dev"], None)
        assert name == "apply"
        return lib.busca_mgframe_apply(a["hist"], a["frames"], a["count"], a["newest"], a["pos"], a["vel"], a["H"], a["gallery"], a["g_count"], a["g_newest"],
                                       a["seen"], a["budget"], a["E"], a["track_det"], a["det_track"], a["feat"], a["boxes"], a["may"], a["free"], *tail,
                                       a["det_slot"], a["dev"], None)

    def refused(name, words, **kw):
        assert call(name, **kw) == _mgframe_lib.EINVAL, (name, kw)
        msg = lib.busca_mgframe_last_error().decode()
        assert msg.startswith("busca_mgframe_" + name) and words in msg, (name, kw, msg)
    names = ("advance", "distance", "thresholds", "cost", "keep", "apply")
    for name in names:                                   # what every call judges alike
        for size in ("S", "n_total", "m_total", "f_total", "n_warps", "batch", "N", "M", "L", "R"):
            refused(name, "negative size", **{size: -1})
        refused(name, "negative device", dev=-1)
        refused(name, "more than a grid holds", batch=65536)
        refused(name, "more than a grid holds", R=65536, N=65536)
        refused(name, "more than a grid holds", L=65536)
        refused(name, "beyond the slab", inact_row=6)
        refused(name, "null pointer (problems)", problems=None)
        refused(name, "misaligned", problems=0x10002)
        assert call(name, batch=0) == 0, name
    # advance
    refused("advance", "at least 2 rows", H=1)
    refused("advance", "last_n_frames", last_n=1)
    refused("advance", "null pointer (warps", warps=None)
    for ptr in ("hist", "frames", "count", "newest", "pos", "vel", "slot", "pos_out"):
        refused("advance", "null pointer", **{ptr: None})
    for ptr in ("hist", "pos", "vel", "pos_out"):
        refused("advance", "misaligned", **{ptr: ODD})
    for ptr in ("frames", "count", "newest", "slot", "warps"):
        refused("advance", "misaligned", **{ptr: 0x10002})
    assert call("advance", L=0) == 0 and call("advance", n_total=0, slot=None) == 0
    assert call("advance", n_warps=0, warps=None, batch=0) == 0
    # distance
    refused("distance", "negative size", rows=-1)
    refused("distance", "budget", budget=0)
    for bad in (8, 24, 4096):
        refused("distance", "multiple of 16", E=bad)
    refused("distance", "unknown reduce", reduce=5)
    refused("distance", "unknown reduce", reduce=-1)
    refused("distance", "budget of at most 256", reduce=4, budget=257)
    refused("distance", "groups", groups=0)
    refused("distance", "groups", groups=4)
    refused("distance", "indexed as the slot list", by_list=1, rows=8)
    for ptr in ("gallery", "dets", "out", "slot"):
        refused("distance", "null pointer", **{ptr: None})
    refused("distance", "16 bytes", gallery=ODD)
    refused("distance", "16 bytes", dets=0x10008)
    refused("distance", "misaligned", out=ODD)
    refused("distance", "misaligned", g_count=0x10002)
    for empty in ("R", "M", "n_total", "m_total"):
        assert call("distance", **{empty: 0, "inact_row": -1}) == 0, empty
    assert call("distance", by_list=1, rows=10, slot=None, batch=0) == 0
    # thresholds
    refused("thresholds", "which", which=0)
    refused("thresholds", "which", which=4)
    for ptr in ("cost", "thr"):
        refused("thresholds", "null pointer", **{ptr: None})
        refused("thresholds", "misaligned", **{ptr: ODD})
    for empty in ("R", "M", "n_total", "m_total"):
        assert call("thresholds", **{empty: 0}) == 0, empty
    # cost
    refused("cost", "alpha is NaN", alpha=nan)
    refused("cost", "go together", tl=None)
    refused("cost", "go together", dl=None)
    refused("cost", "null pointer (cost)", cost=None)
    refused("cost", "det_boxes with pos", boxes=None)
    for ptr in ("cost", "pos", "boxes", "thr"):
        refused("cost", "misaligned", **{ptr: ODD})
    for ptr in ("tl", "dl"):
        refused("cost", "misaligned", **{ptr: 0x10002})
    for empty in ("R", "M", "n_total", "m_total"):
        assert call("cost", **{empty: 0}) == 0, empty
    # keep
    refused("keep", "stage", stage=3)
    refused("keep", "stage", stage=-1)
    refused("keep", "the mask goes with stage 1", stage=0, mask=1)
    refused("keep", "the mask goes with stage 1", stage=2, mask=1)
    for ptr in ("c2r", "det_track", "cost", "r2c", "thr", "track_det"):
        refused("keep", "null pointer", **{ptr: None})
    for ptr in ("cost", "thr"):
        refused("keep", "misaligned", **{ptr: ODD})
    for ptr in ("r2c", "c2r", "track_det", "det_track"):
        refused("keep", "misaligned", **{ptr: 0x10002})
    assert call("keep", M=0) == 0 and call("keep", m_total=0) == 0
    # apply
    refused("apply", "negative size", H=-1)
    refused("apply", "at least 2 rows", H=1)
    refused("apply", "at least 1 row", budget=0)
    refused("apply", "at least 1 row", E=0)
    refused("apply", "one problem takes 2048", M=2049)
    for ptr in ("hist", "frames", "count", "newest", "pos", "vel", "gallery", "g_count", "g_newest", "seen", "slot", "track_det", "det_track", "feat", "boxes",
                "may", "det_slot", "free"):
        refused("apply", "null pointer", **{ptr: None})
    for ptr in ("hist", "pos", "vel", "boxes"):
        refused("apply", "misaligned", **{ptr: ODD})
    for ptr in ("frames", "count", "newest", "gallery", "g_count", "g_newest", "slot", "track_det", "det_track", "feat", "free", "det_slot"):
        refused("apply", "misaligned", **{ptr: 0x10002})
    assert call("apply", M=0) == 0 and call("apply", m_total=0) == 0
    refused("apply", "null pointer", R=0, N=0, slot=None, track_det=None, det_slot=None)      # without rows the row operands may be NULL, the others not
    # the message is the calling thread's own
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.busca_mgframe_last_error()))
    t.start()
    t.join()
    assert seen == [b""] and lib.busca_mgframe_last_error() != b""


def test_python_level_checks(monkeypatch):
    """Every check of frame() runs per problem and names it, and the checks across the batch raise, before any device work: the store is a shell
    without tensors, the library is never loaded and nothing is uploaded."""
    import types
    import torch
    from busca_amd import _mgframe_lib, ghost_store, tracking
    monkeypatch.setattr(_mgframe_lib, "load", lambda: pytest.fail("device work before the checks"))
    monkeypatch.setattr(ghost_store, "h2d_async", lambda *a, **k: pytest.fail("an upload before the checks"))
    monkeypatch.setattr(ghost_store, "to_dev", lambda *a, **k: pytest.fail("an upload before the checks"))
    st = object.__new__(tracking.GhostStore)
    st.capacity, st.budget, st.E, st.history = CAP, BUDGET, E, HIST
    st.motion = types.SimpleNamespace(box32=False, all_warped=True)
    st.gallery = types.SimpleNamespace(mv_avg=object(), mv_seen=object())
    feats, boxes = np.zeros((3, E), np.float32), np.zeros((3, 4))
    P = tracking.GhostFrameProblem
    assert P is ghost_store.GhostFrameProblem and P._fields == ("active", "inactive", "det_feats", "det_boxes", "frame", "det_conf", "idle", "free_slots",
                                                                "labels", "warp", "all_warped")
    assert P([1], [2], feats, boxes, 5)[5:] == (None, (), (), None, None, False)
    good = P((1, 2), (3,), feats, boxes, 5)

    def batch(second, cfg=DEFAULT, first=good):
        return st.frame_batch([first, second], cfg)
    other = dict(active=(11, 12), inactive=(13,), det_feats=feats, det_boxes=boxes, frame=6)
    for kw, words in ((dict(active=(11, 11)), "distinct"), (dict(idle=(13,)), "distinct"), (dict(active=(CAP,)), "beyond the capacity"),
                      (dict(active=(-1,)), "negative"), (dict(free_slots=(7, 7)), "distinct"), (dict(free_slots=(13,)), "free slot 13 is also listed"),
                      (dict(det_feats=np.zeros((2, E), np.float32)), "features for 3 detections"), (dict(det_boxes=np.zeros((3, 5))), "[m,4]"),
                      (dict(det_conf=[0.5]), "1 confidences for 3"), (dict(labels=([0, 1], [0, 0, 0])), "2 track labels"),
                      (dict(warp=np.zeros(5, np.float32)), "[2,3] warp"), (dict(active=torch.zeros(2, dtype=torch.int32)), "host slot lists"),
                      (dict(frame=2 ** 31), "no int32")):
        with pytest.raises(ValueError, match=re.escape(words)) as err:
            batch(P(**dict(other, **kw)))
        assert "GhostStore.frame_batch: problem 1" in str(err.value), (kw, str(err.value))
    # across the batch
    with pytest.raises(ValueError, match="distinct across the whole batch .slot 2 "):
        batch(P(**dict(other, active=(11, 2))))
    with pytest.raises(ValueError, match="distinct across the whole batch .slot 3 "):
        batch(P(**dict(other, free_slots=(3,))))                  # a free slot another problem lists as a track's
    with pytest.raises(ValueError, match="distinct across the whole batch .slot 40 "):
        batch(P(**dict(other, free_slots=(40,))), first=good._replace(free_slots=(40, 41)))
    with pytest.raises(ValueError, match="problem 1: host and device det_feats in one batch"):
        batch(P(**dict(other, det_feats=torch.zeros(3, E))))
    # the solver's limit: the slab of the separate mode is the most active plus the most inactive rows
    big = object.__new__(tracking.GhostStore)
    big.capacity, big.budget, big.E, big.history, big.motion, big.gallery = 8192, BUDGET, E, HIST, st.motion, st.gallery
    lots = P(tuple(range(1500)), (1500,), feats, boxes, 5), P((2000,), tuple(range(2001, 3001)), feats, boxes, 5)
    with pytest.raises(ValueError, match="2500 rows"):
        big.frame_batch(lots, CONFIGS["separate"])
    with pytest.raises(ValueError, match="problem 0: .*2049 tracks"):
        big.frame_batch([P(tuple(range(2049)), (), feats, boxes, 5)], DEFAULT)
    # what frame() refuses, per problem
    for cfg, exc, words in ((dict(DEFAULT, use_bism=True), ValueError, "use_bism"), (dict(DEFAULT, distance="euclidean"), ValueError, "distance"),
                            (dict(DEFAULT, kalman=True), ValueError, "Kalman"),
                            (dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], center_only=True)), ValueError, "center_only"),
                            (dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], combi="mult")), NotImplementedError, "combi"),
                            (dict(DEFAULT, avg_inact={"do": True, "num": 3, "proxy": "mode"}), NotImplementedError, "'mode'"),
                            (dict(DEFAULT, avg_inact={"do": True, "num": "all", "proxy": "mv_avg"}), ValueError, "'mv_avg' takes a number"),
                            (dict(DEFAULT, act_reid_thresh="sometimes"), ValueError, "must be a number"),
                            (dict(DEFAULT, motion_config=dict(DEFAULT["motion_config"], last_n_frames=1)), ValueError, "last_n_frames"),
                            (dict(DEFAULT, avg_inact={"do": True, "num": 9, "proxy": "each_sample"}), ValueError, "avg_inact")):
        with pytest.raises(exc, match=words) as err:
            batch(P(**other), cfg=cfg)
        assert "GhostStore.frame_batch" in str(err.value), str(err.value)
    with pytest.raises(ValueError, match="one call takes 65535"):
        st.frame_batch([good] * 65536, DEFAULT)
    assert st.motion.all_warped is True                            # nothing was touched
    import sys
    sys.path.insert(0, os.path.join(ROOT, "busca_amd", "compat"))
    try:
        from busca import tracking as alias
        assert alias.GhostFrameProblem is tracking.GhostFrameProblem
    finally:
        sys.path.remove(os.path.join(ROOT, "busca_amd", "compat"))


def test_all_warped_after():
    from busca_amd import tracking
    P, F = tracking.GhostFrameProblem, tracking.GhostFrame
    after = tracking.GhostStore.all_warped_after
    quiet, match, born = F([], [], [], [], [], (1.0, 1.0), None), F([(0, 1)], [], [], [], [], (1.0, 1.0), None), F([], [(2, 7)], [], [], [], (1.0, 1.0), None)
    still, warped, carried = P([], [], None, None, 1), P([], [], None, None, 1, warp=WARP), P([], [], None, None, 1, all_warped=True)
    assert after(still, quiet) is False and after(still, match) is False            # no warp, nothing carried
    assert after(warped, quiet) is True and after(carried, quiet) is True           # warped (now or before) and nothing added
    assert after(warped, match) is False and after(warped, born) is False           # a detection was added since
    assert after(carried, match) is False and after(carried, born) is False
    assert after(P([], [], None, None, 1, warp=WARP, all_warped=True), quiet) is True


# ---- GPU: the whole batch against the list of frames -------------------------------------------------------------------
def load_batch(ctx, scenes):
    """One store of len(scenes) * CAP slots holding scene k in the slots k * CAP .., and the single stores it was loaded from."""
    from busca_amd import tracking
    big = tracking.GhostStore(CAP * len(scenes), BUDGET, E, HIST, ctx=ctx)
    singles = [sc.store(ctx) for sc in scenes]
    for k, st in enumerate(singles):
        for key in GALLERY_KEYS:
            getattr(big.gallery, key)[k * CAP:(k + 1) * CAP].copy_(getattr(st.gallery, key)[:CAP])      # a gallery has a spare row behind its slots
        for key in MOTION_KEYS:
            getattr(big.motion, key)[k * CAP:(k + 1) * CAP].copy_(getattr(st.motion, key)[:CAP])
    return big, singles


def slice_state(big, k):
    return [x[k * CAP:(k + 1) * CAP] for x in store_state(big)]


def own_state(st):
    return [x[:CAP] for x in store_state(st)]


def problem_of(sc, k, frame, free=6, labels=True, warp=None, all_warped=False, device=False, lists=None, conf=True):
    """Scene `sc` as problem k of a batch (its slots moved by k * CAP) and the arguments of frame() on its own store."""
    from busca_amd import tracking
    active, inactive, idle = (sc.active, sc.inactive, sc.idle) if lists is None else lists
    off = k * CAP
    lab = None
    if labels:
        n = len(active) + len(inactive)
        lab = ((np.arange(n) % 4 == 3).astype(np.int32), sc.dlabels)
    feats = _dev(sc.feats) if device else sc.feats
    kw = dict(det_conf=sc.conf if conf else None, labels=lab, warp=warp)
    p = tracking.GhostFrameProblem([s + off for s in active], [s + off for s in inactive], feats, sc.boxes, frame, idle=[s + off for s in idle],
                                   free_slots=[s + off for s in sc.free[:free]], all_warped=all_warped, **kw)
    single = dict(args=(active, inactive, feats, sc.boxes, frame), kw=dict(kw, idle=idle, free_slots=sc.free[:free]))
    return p, single


def assert_batch(ctx, big, singles, problems, calls, cfg, what, apply=True):
    """frame_batch on `big` against frame() of every problem on its own store: results, distances and every bit of both rings."""
    got = big.frame_batch(problems, cfg, apply=apply)
    assert len(got) == len(problems) and big.motion.all_warped is False
    for k, (st, p, c) in enumerate(zip(singles, problems, calls)):
        st.motion.all_warped = p.all_warped
        want = st.frame(*c["args"], cfg, apply=apply, **c["kw"])
        g = got[k]
        assert g.matches == want.matches and g.overflow == want.overflow, (what, k, g.matches, want.matches)
        assert [(j, s - k * CAP) for j, s in g.new] == want.new, (what, k, g.new, want.new)
        assert g.unassigned_active == want.unassigned_active and g.unassigned_inactive == want.unassigned_inactive, (what, k)
        assert same(np.array(g.thresholds), np.array(want.thresholds)), (what, k, g.thresholds, want.thresholds)
        gd, wd = (g.dist if isinstance(g.dist, list) else [g.dist]), (want.dist if isinstance(want.dist, list) else [want.dist])
        assert len(gd) == len(wd), (what, k)
        for x, y in zip(gd, wd):
            assert (x is None) == (y is None), (what, k)
            if x is not None:
                assert same(_host(x.contiguous()), _host(y.contiguous())), (what, k, "dist")
        assert_same_states(slice_state(big, k), own_state(st), (what, k))
        from busca_amd import tracking
        if apply:
            assert tracking.GhostStore.all_warped_after(p, g) == st.motion.all_warped, (what, k)
    return got


RAGGED = [(17, 65), (1, 1), (15, 63), (16, 64), (9, 12), (14, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("B", [1, 3, 6])
def test_batch_equals_the_list_of_frames(ctx, B, name):
    """Ragged problems, a host warp and a device warp next to problems without, all_warped differing, device and host features, labels."""
    cfg = CONFIGS[name]
    for device in (B == 3,):                                       # device features in the batch of 3, host arrays in the others
        scenes = [Scene(n, m, 100 * B + 7 * k + n) for k, (n, m) in enumerate(RAGGED[:B])]
        big, singles = load_batch(ctx, scenes)
        problems, calls = [], []
        for k, sc in enumerate(scenes):
            warp = None if name == "mv_avg" else (WARP if k % 3 == 0 else _dev(WARP * np.float32(1.001)).reshape(6) if k % 3 == 1 else None)
            p, c = problem_of(sc, k, 23 + k, labels=name != "every" or k == 1, warp=warp, all_warped=k == 2, device=device)
            problems.append(p), calls.append(c)
        got = assert_batch(ctx, big, singles, problems, calls, cfg, (B, name, device))
        assert len(got[0].matches) >= 5 and got[0].new and got[0].overflow


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "separate", "every", "mv_avg"])
def test_degenerate_problems_in_a_batch(ctx, name):
    """One problem of each kind next to an ordinary one: no detections (warped only - and its mv_avg rows stay), no track to match (every detection
    starts a track whatever its confidence), no active track (in the separate mode nothing is matched), no free slot, no confidences."""
    cfg = CONFIGS[name]
    scenes = [Scene(9, 12, 3), Scene(9, 0, 4), Scene(0, 5, 5, n_idle=3), Scene(9, 12, 6), Scene(7, 9, 7), Scene(17, 65, 8)]
    big, singles = load_batch(ctx, scenes)
    warp = None if name == "mv_avg" else WARP
    specs = [dict(warp=warp), dict(warp=warp), dict(warp=warp), dict(lists=([], scenes[3].active + scenes[3].inactive, scenes[3].idle), free=20),
             dict(free=0), dict(conf=False, free=40)]
    problems, calls = zip(*[problem_of(sc, k, 30 - k, labels=False, **spec) for k, (sc, spec) in enumerate(zip(scenes, specs))])
    got = assert_batch(ctx, big, singles, list(problems), list(calls), cfg, name)
    assert got[1].matches == [] and got[1].dist is None and got[1].unassigned_active == list(range(scenes[1].na))
    assert [j for j, _ in got[2].new] == list(range(5)) and got[2].dist is None
    if name == "separate":
        assert got[3].matches == [] and got[3].dist[1] is None and got[3].new
    assert got[4].new == [] and got[4].overflow and got[4].matches
    assert len(got[5].new) == 40 and got[5].overflow           # without confidences every unassigned detection starts a track, while slots last
    # a batch without any detection: only the advance happens, nothing is copied home
    import torch
    big, singles = load_batch(ctx, scenes[:2])
    none = [problem_of(Scene(9, 0, 3 + k), k, 23, labels=False, warp=warp) for k in range(2)]
    count = {"n": 0}
    orig = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (count.__setitem__("n", count["n"] + 1), orig(self, *a, **k))[1]
    try:
        got = big.frame_batch([p for p, _ in none], cfg)
    finally:
        torch.Tensor.cpu = orig
    assert count["n"] == 0 and [g.matches for g in got] == [[], []]
    for k, st in enumerate(singles):
        st.frame(*none[k][1]["args"], cfg, **none[k][1]["kw"])
        assert_same_states(slice_state(big, k), own_state(st), ("no detections", k))
    assert big.frame_batch([], cfg) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "separate"])
def test_ties_and_the_threshold_edge_inside_a_batch(ctx, name):
    """Whole columns of equal costs, and in the separate mode a matched pair whose cost equals its threshold: not assigned by the active stage, its
    detection stays available to the problem's inactive tracks - next to other problems in the same slab."""
    tie = Scene(14, 24, 5, tie=True)
    edge_sc = Scene(8, 6, 17, n_idle=0)
    t_act, t_in = 0, edge_sc.na
    if name == "separate":                                         # a twin of the active track among the inactive ones
        edge_sc.samples[t_in] = [(f, feat.copy(), box.copy()) for f, feat, box in edge_sc.samples[t_act]]
    j = next(j for j in range(edge_sc.m) if np.abs(edge_sc.boxes[j] - edge_sc.samples[t_act][-1][2]).max() < 4)
    cfg = dict(CONFIGS[name], nan_first=True)
    probe = edge_sc.store(ctx).frame(edge_sc.active, edge_sc.inactive, edge_sc.feats, edge_sc.boxes, 23, cfg, det_conf=edge_sc.conf,
                                     free_slots=edge_sc.free[:6], apply=False)
    assert (t_act, j) in probe.matches
    dist = probe.dist[0] if name == "separate" else probe.dist
    cfg = dict(cfg, act_reid_thresh=float(_host(dist)[j, t_act]))
    scenes = [tie, edge_sc, Scene(17, 65, 9)]
    big, singles = load_batch(ctx, scenes)
    problems, calls = zip(*[problem_of(sc, k, 23, labels=False) for k, sc in enumerate(scenes)])
    got = assert_batch(ctx, big, singles, list(problems), list(calls), cfg, ("ties", name))
    assert (t_act, j) not in got[1].matches and t_act in got[1].unassigned_active
    if name == "separate":
        assert (t_in, j) in got[1].matches
    big, singles = load_batch(ctx, scenes)                          # and without applying: the state stays what the step left
    assert_batch(ctx, big, singles, list(problems), list(calls), cfg, ("ties, apply=False", name), apply=False)


class Sequence:
    """The host bookkeeping of one Tracker over scripted frames (test_a_scripted_scene_through_both_routes of test_ghost_frame.py, per sequence)."""

    def __init__(self, seed, first_frame, warp_on, slots):
        self.rs = np.random.RandomState(seed)
        self.people = []
        for p in range(10):
            hidden = {0: (), 1: (4, 5), 2: range(5, 40), 3: (6,), 4: range(3, 40), 5: (7, 8, 9)}.get((p + seed) % 6, ())
            self.people.append((self.rs.standard_normal(E), 80.0 * p, 50.0 * (p % 3), self.rs.uniform(-3, 3), self.rs.uniform(-2, 2), 0 if p < 7 else 7 + (p - 7),
                                set(hidden)))
        self.active, self.inactive, self.free = [], {}, list(slots)
        self.first_frame, self.warp_on, self.all_warped = first_frame, warp_on, False
        self.seen = dict(found=0, idle=0, released=0, reborn=0, carried=0)
        self.released = set()

    def step(self, t):
        vis = [p for p, q in enumerate(self.people) if q[5] <= t and t not in q[6]]
        self.feats = np.stack([self.people[p][0] + 0.1 * self.rs.standard_normal(E) for p in vis]).astype(np.float32)
        self.boxes = np.stack([np.array([q[1] + q[3] * t, q[2] + q[4] * t, q[1] + q[3] * t + 30, q[2] + q[4] * t + 70]) + self.rs.uniform(-1, 1, 4)
                               for q in (self.people[p] for p in vis)])
        self.curr = [s for s, c in self.inactive.items() if c <= 2]
        self.idle = [s for s, c in self.inactive.items() if c > 2]
        self.seen["idle"] += bool(self.idle)
        self.seen["carried"] += self.all_warped
        self.warp = WARP if t in self.warp_on else None
        self.frame = self.first_frame + 2 * t

    def problem(self, off=0):
        from busca_amd import tracking
        mv = lambda xs: [s + off for s in xs]                      # noqa: E731
        return tracking.GhostFrameProblem(mv(self.active), mv(self.curr), self.feats, self.boxes, self.frame, det_conf=np.full(len(self.feats), 0.9),
                                          idle=mv(self.idle), free_slots=mv(self.free), warp=self.warp, all_warped=self.all_warped)

    def book(self, got, off, galleries):
        from busca_amd import tracking
        self.all_warped = tracking.GhostStore.all_warped_after(self.problem(off), got)
        new = [s - off for _, s in got.new]
        rows = self.active + self.curr
        hit = {rows[i] for i, _ in got.matches}
        self.seen["found"] += sum(1 for i, _ in got.matches if i >= len(self.active))
        for s in rows:
            if s in hit:
                self.inactive.pop(s, None)
            elif s in self.active:
                self.inactive[s] = 0
        self.active = [s for s in self.active if s in hit] + [s for s in self.curr if s in hit] + new
        self.seen["reborn"] += sum(1 for s in new if s in self.released)
        self.free = [s for s in self.free if s not in set(new)]
        for s in list(self.inactive):
            self.inactive[s] += 1
            if self.inactive[s] > 4:                               # gone: the slot goes back to the free list, at its front
                del self.inactive[s]
                for gallery, o in galleries:
                    gallery.release([s + o])
                self.free.insert(0, s)
                self.released.add(s)
                self.seen["released"] += 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "mv_avg"])
def test_scripted_sequences_in_lock_step(ctx, name):
    """Three sequences of 13 frames on one store against three single-sequence stores driven by frame(): tracks are lost, found, expire into idle,
    are released and born into released slots; the frame numbers differ, one sequence is warped on some frames, all_warped is carried by
    all_warped_after.  Every bit of both stores is equal after every step."""
    from busca_amd import tracking
    cfg = CONFIGS[name]
    seqs = [Sequence(77 + k, 100 * k, (3, 7, 8) if k == 1 and name == "default" else (), [int(s) for s in np.random.RandomState(5 + k).permutation(CAP)[:14]])
            for k in range(3)]
    big = tracking.GhostStore(3 * CAP, BUDGET, E, HIST, ctx=ctx)
    singles = [tracking.GhostStore(CAP, BUDGET, E, HIST, ctx=ctx) for _ in seqs]
    for t in range(13):
        for q in seqs:
            q.step(t)
        got = big.frame_batch([q.problem(k * CAP) for k, q in enumerate(seqs)], cfg)
        for k, (q, st) in enumerate(zip(seqs, singles)):
            st.motion.all_warped = q.all_warped
            p = q.problem()
            want = st.frame(p.active, p.inactive, p.det_feats, p.det_boxes, p.frame, cfg, det_conf=p.det_conf, idle=p.idle, free_slots=p.free_slots,
                            warp=p.warp)
            g = got[k]
            assert g.matches == want.matches and [(j, s - k * CAP) for j, s in g.new] == want.new and g.overflow == want.overflow, (t, k)
            assert g.unassigned_active == want.unassigned_active and g.unassigned_inactive == want.unassigned_inactive, (t, k)
            assert_same_states(slice_state(big, k), own_state(st), (t, k))
            q.book(g, k * CAP, [(big.gallery, k * CAP), (st.gallery, 0)])
            assert q.all_warped == st.motion.all_warped, (t, k)
    for k, q in enumerate(seqs):
        assert q.seen["found"] >= 1 and q.seen["idle"] >= 2 and q.seen["released"] >= 1, (k, q.seen)
    assert sum(q.seen["reborn"] for q in seqs) >= 1
    assert big.motion.all_warped is False
    assert int(_host(big.gallery.count).max()) == BUDGET and int(_host(big.motion.count).max()) == HIST       # the rings wrapped


@pytest.mark.gpu
def test_one_copy_home_and_the_same_calls_whatever_the_batch(ctx, monkeypatch):
    """Every route from a device tensor to the host is counted: one frame_batch takes exactly one, and none has happened when busca_mgframe_apply is
    enqueued.  The library calls of a batch of 2 and of a batch of 5 are the same calls."""
    import torch
    from busca_amd import _mgframe_lib, _store_lib
    lib = _mgframe_lib.load()
    for name in ("default", "separate", "every", "mv_avg"):
        calls_of = {}
        for B in (1, 2, 5):
            scenes = [Scene(15 + k, 60 + k, 22 + k) for k in range(B)]
            big, singles = load_batch(ctx, scenes)
            problems, calls = zip(*[problem_of(sc, k, 23, labels=False, warp=None if name == "mv_avg" else WARP, device=True) for k, sc in enumerate(scenes)])
            count = {"n": 0, "at_apply": None, "calls": []}
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

                def logged(owner, fn):
                    real = getattr(owner, fn)

                    def f(*a):
                        count["calls"].append(fn)
                        if fn == "busca_mgframe_apply":
                            count["at_apply"] = count["n"]
                        return real(*a)
                    mp.setattr(owner, fn, f)
                for fn in _mgframe_lib.MGFRAME_API:
                    if fn not in ("busca_mgframe_version", "busca_mgframe_last_error"):
                        logged(lib, fn)
                for fn in ("busca_ghost_proxies", "busca_linear_assignment", "busca_ghost_distance", "busca_ghost_thresholds"):
                    logged(ctx.lib, fn)
                logged(_store_lib.load(), "busca_store_mv_avg")
                got = big.frame_batch(list(problems), CONFIGS[name])
                copies = count["n"]
            assert count["at_apply"] == 0 and count["calls"].count("busca_mgframe_apply") == 1 and copies == 1, (name, B, count)
            assert not [c for c in count["calls"] if c in ("busca_ghost_distance", "busca_ghost_thresholds")], (name, count["calls"])
            assert count["calls"].count("busca_linear_assignment") == (2 if name == "separate" else 1), (name, count["calls"])
            calls_of[B] = count["calls"]
            assert all(len(g.matches) >= 5 for g in got)
        assert calls_of[2] == calls_of[5] == calls_of[1], (name, calls_of)


@pytest.mark.gpu
def test_a_batch_behind_a_busy_stream(ctx, busy):
    from tests.test_streams_gpu import behind
    scenes, others = [Scene(17, 65, 22), Scene(9, 12, 23), Scene(15, 63, 24)], [Scene(17, 65, 99), Scene(9, 12, 98), Scene(15, 63, 97)]
    big, singles = load_batch(ctx, scenes)
    poison, _ = load_batch(ctx, others)
    tensors = lambda s: [getattr(s.motion, k) for k in MOTION_KEYS] + [getattr(s.gallery, k) for k in GALLERY_KEYS]      # noqa: E731
    true = [t.clone() for t in tensors(big)]
    cfg = CONFIGS["separate"]
    problems, calls = zip(*[problem_of(sc, k, 23 + k, labels=False, warp=WARP if k != 1 else None) for k, sc in enumerate(scenes)])

    def call(x, outs, stream):
        got = big.frame_batch(list(problems), cfg)
        return [np.asarray(v, dtype=np.int64).reshape(-1) for g in got for v in (g.matches, g.new, g.overflow, g.unassigned_active, g.unassigned_inactive)]
    want, got = behind(busy, "GhostStore.frame_batch", call, true=true, poison=tensors(poison), x=tensors(big), form="current", host=True)
    k = len(true)
    assert len(got[k]) >= 12 and len(got[k + 1]) >= 2
    for i, (st, c) in enumerate(zip(singles, calls)):
        st.frame(*c["args"], cfg, **c["kw"])
        assert_same_states([x[i * CAP:(i + 1) * CAP] for x in got[:k]], own_state(st), ("behind a busy stream", i))


# ---- GPU: the six calls, each against its single-problem counterpart ---------------------------------------------------------
BATCHES = {                                                        # the problems' (n_k, m_k), then E, budget, H
    "one": ([(17, 65)], 16, 1, 2),
    "two": ([(1, 1), (16, 64)], 64, 3, 5),
    "three": ([(15, 63), (17, 65), (16, 64)], 16, 3, 5),
}


class Raw:
    """A batch of problems over one random store, with - in the batch of three - one problem without detections, one without tracks, one without
    active tracks and one bad table row (its detections leave the table) that names rows other problems own.  Slots -1 and S + 5 are listed too."""

    def __init__(self, ctx, name, sep, seed=0):
        from busca_amd import tracking
        shapes, self.E, self.budget, self.H = BATCHES[name]
        rs = self.rs = np.random.RandomState(len(name) * 13 + seed)
        self.S, self.sep = 256, sep
        spec = [((n + 1) // 2, n // 2, 2, m, 3) for n, m in shapes]                     # na, ni, nidle, m, n_free
        if name == "three":
            spec += [(3, 2, 1, 0, 2), (0, 0, 3, 4, 5), (0, 6, 0, 7, 2), (2, 2, 1, 5, 1)]
        self.bad = {6} if name == "three" else set()
        self.B = B = len(spec)
        perm = rs.permutation(self.S)
        used = 0
        self.lists = []
        for na, ni, nidle, _, nf in spec:
            tot = na + ni + nidle + nf
            s = perm[used:used + tot].astype(np.int32)
            used += tot
            self.lists.append([s[:na], s[na:na + ni], s[na + ni:na + ni + nidle], s[na + ni + nidle:]])
        if shapes[-1][0] >= 15:                                    # skipped slots: touch no memory
            self.lists[len(shapes) - 1][0][1] = -1
            self.lists[len(shapes) - 1][1][2] = self.S + 5
        self.na, self.ni, self.nidle, self.m, self.nf = (np.array([x[i] for x in spec]) for i in range(5))
        good = [k for k in range(B) if k not in self.bad]
        self.A, self.I = int(self.na.sum()), int(self.ni.sum())
        self.n_total, self.m_total, self.f_total = int(self.A + self.I + self.nidle.sum()), int(self.m.sum()), int(self.nf.sum())
        self.N, self.M = int((self.na + self.ni)[good].max()), int(self.m[good].max())
        self.L = int((self.na + self.ni + self.nidle)[good].max())
        self.NA = int(self.na[good].max())
        self.R, self.inact_row = (self.NA + int(self.ni[good].max()), self.NA) if sep else (self.N, -1)
        t = np.zeros((B, WORDS), dtype=np.int32)
        t[:, 1], t[:, 3], t[:, 5], t[:, 7], t[:, 9] = self.na, self.ni, self.nidle, self.m, self.nf
        t[:, 0] = np.cumsum(np.r_[0, self.na[:-1]])
        t[:, 2] = self.A + np.cumsum(np.r_[0, self.ni[:-1]])
        t[:, 4] = self.A + self.I + np.cumsum(np.r_[0, self.nidle[:-1]])
        t[:, 6], t[:, 8] = np.cumsum(np.r_[0, self.m[:-1]]), np.cumsum(np.r_[0, self.nf[:-1]])
        t[:, 10] = [(-1, 0, 1)[k % 3] for k in range(B)]          # a problem with a warp next to one without
        t[:, 11] = 50 + 3 * np.arange(B)
        t[:, 12] = [(2, 3, 0, 1)[k % 4] for k in range(B)]        # stepped or not, diff32 differing between problems
        t[self.m == 0, 12] &= 1                                    # without detections: warped only
        for k in self.bad:
            t[k, 6] = self.m_total - 2                             # its detections leave the table; everything else of the row is plausible
            t[k, 0], t[k, 2], t[k, 4], t[k, 8] = 0, self.A, self.A + self.I, 0      # rows the first problem owns
        self.table = t
        self.slot = np.concatenate([x[g] for g in range(3) for x in self.lists]).astype(np.int32)
        self.free = np.concatenate([x[3] for x in self.lists]).astype(np.int32)
        self.warps = np.stack([WARP.reshape(6), (WARP * np.float32(0.999)).reshape(6)]).astype(np.float32)
        self.feats = rs.standard_normal((self.m_total, self.E)).astype(np.float32)
        self.boxes = rs.uniform(0, 500, (self.m_total, 4))
        self.boxes[:, 2:] += self.boxes[:, :2] + 10
        self.tl, self.dl = rs.randint(0, 2, self.n_total).astype(np.int32), rs.randint(0, 2, self.m_total).astype(np.int32)
        self.may = (rs.uniform(size=self.m_total) < 0.7).astype(np.uint8)
        self.motion = random_motion(ctx, self.S, self.H, 3 + seed)
        g = self.gallery = tracking.GhostGallery(self.S, self.budget, self.E, ctx=ctx)
        g._gallery.copy_(_dev(rs.standard_normal((self.S + 1, self.budget, self.E)).astype(np.float32)))
        g._count.copy_(_dev(rs.randint(0, self.budget + 1, self.S + 1).astype(np.int32)))
        g._newest.copy_(_dev(rs.randint(0, self.budget, self.S + 1).astype(np.int32)))
        g._mv_seen.copy_(_dev(rs.randint(0, 2, self.S + 1).astype(np.uint8)))
        self.d = {k: _dev(getattr(self, k)) for k in ("table", "slot", "free", "warps", "feats", "boxes", "tl", "dl", "may")}
        self.good = good

    def tail(self):
        return (self.S, self.d["slot"].data_ptr(), self.n_total, self.m_total, self.f_total, 2, self.d["table"].data_ptr(), self.B, self.N, self.M, self.L,
                self.R, self.inact_row)

    def rows(self, k):
        """-> (the list rows of problem k's matrix rows, their slab rows)."""
        t = self.table[k]
        at = t[1] if not self.sep else self.inact_row
        return np.r_[t[0]:t[0] + t[1], t[2]:t[2] + t[3]], np.r_[0:t[1], at:at + t[3]]

    def dets(self, k):
        return slice(int(self.table[k, 6]), int(self.table[k, 6] + self.table[k, 7]))

    def slab(self, fill=None):
        """A [B, R, M] float64 block between two guard slabs -> (the device tensor [B + 2, R, M], the pointer of slab 0)."""
        x = np.full((self.B + 2, self.R, self.M), CANARY) if fill is None else fill
        d = _dev(x)
        return d, d.data_ptr() + 8 * self.R * self.M


def rings(m):
    return (m.hist.data_ptr(), m.frames.data_ptr(), m.count.data_ptr(), m.newest.data_ptr(), m.pos.data_ptr(), m.vel.data_ptr())


def motion_state(gm):
    return [_host(getattr(gm, k)) for k in MOTION_KEYS]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_advance(ctx, name):
    """Rings empty, with one sample and wrapped; a problem with a warp next to one without; diff32 differing; a problem that is warped only."""
    from busca_amd import _gframe_lib, _mgframe_lib
    r = Raw(ctx, name, False)
    a, b = clone_motion(ctx, r.motion), clone_motion(ctx, r.motion)
    out = _dev(np.full((r.n_total + 2, 4), CANARY))
    t = r.tail()
    _mgframe_lib.check(_mgframe_lib.load().busca_mgframe_advance(*rings(a), r.S, r.H, t[1], r.n_total, r.m_total, r.f_total, r.d["warps"].data_ptr(), 2,
                                                                 t[6], r.B, r.N, r.M, r.L, r.R, r.inact_row, 3, out.data_ptr() + 32, *_where()))
    want = np.full((r.n_total + 2, 4), CANARY)
    for k in r.good:
        row = r.table[k]
        listed = np.concatenate(r.lists[k][:3])
        idx = np.r_[row[0]:row[0] + row[1], row[2]:row[2] + row[3], row[4]:row[4] + row[5]]
        step = bool(row[12] & 2)
        if not len(listed) or (row[10] < 0 and not step):
            continue
        o, d_listed = _dev(np.full((len(listed), 4), CANARY)), _dev(listed)
        _gframe_lib.check(_gframe_lib.load().busca_gframe_advance(*rings(b), r.S, r.H, d_listed.data_ptr(), len(listed), len(listed) if step else 0,
                                                                  int(row[1]) if step else 0, 3, int(row[12] & 1),
                                                                  r.d["warps"].data_ptr() + 24 * int(row[10]) if row[10] >= 0 else None, o.data_ptr(),
                                                                  *_where()))
        if step:
            want[1 + idx] = _host(o)
    assert same(_host(out), want)
    before = motion_state(r.motion)
    for key, x, y, z in zip(MOTION_KEYS, motion_state(a), motion_state(b), before):
        assert same(x, y), key
    assert not same(motion_state(a)[4], before[4]) and (name == "one" or not same(motion_state(a)[0], before[0]))
    if name != "three":
        assert np.isnan(want[1:-1]).any()                          # the skipped slots of a stepped problem: rows of NaN


@pytest.mark.gpu
@pytest.mark.parametrize("sep", [False, True], ids=["contiguous", "fixed"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_distance(ctx, name, sep):
    """All five reductions on the gallery route, the two groups in two calls, and the table of proxy rows with MIN: every entry is busca_ghost_distance's."""
    from busca_amd import _mgframe_lib
    lib = _mgframe_lib.load()
    r = Raw(ctx, name, sep)
    g = r.gallery
    table = _dev(r.rs.standard_normal((r.n_total, r.E)).astype(np.float32))
    for reduce in (0, 1, 2, 3, 4, "table", "groups"):
        red = reduce if isinstance(reduce, int) else 0
        slab, p = r.slab()
        if reduce == "table":
            _mgframe_lib.check(lib.busca_mgframe_distance(table.data_ptr(), None, r.n_total, 1, 1, r.d["feats"].data_ptr(), r.E, 0, 3, *r.tail(), p, *_where()))
        else:
            for groups in ((1, 2) if reduce == "groups" else (3,)):
                _mgframe_lib.check(lib.busca_mgframe_distance(g._gallery.data_ptr(), g._count.data_ptr(), r.S, 0, r.budget, r.d["feats"].data_ptr(), r.E, red,
                                                              groups, *r.tail(), p, *_where()))
        want = np.full((r.B + 2, r.R, r.M), CANARY)
        for k in r.good:
            lr, sr = r.rows(k)
            n, m = len(lr), int(r.table[k, 7])
            if n == 0 or m == 0:
                continue
            o = _dev(np.zeros((n, m)))
            f = r.d["feats"][r.dets(k)]
            if reduce == "table":
                rows = table[_dev(lr.astype(np.int64))].contiguous()
                ctx.check(ctx.lib.busca_ghost_distance(ctx.h, rows.data_ptr(), None, None, n, 1, f.data_ptr(), m, r.E, 0, o.data_ptr(), _where()[1]))
            else:
                s = r.slot[lr].copy()
                s[s >= r.S] = -1                                   # the single call skips a negative slot only
                d_s = _dev(s)
                ctx.check(ctx.lib.busca_ghost_distance(ctx.h, g._gallery.data_ptr(), d_s.data_ptr(), g._count.data_ptr(), n, r.budget, f.data_ptr(), m,
                                                       r.E, red, o.data_ptr(), _where()[1]))
            want[1 + k][sr, :m] = _host(o)
        assert same(_host(slab), want), (name, sep, reduce)
        assert np.isinf(want).any() or name != "three" or reduce == "table"      # a skipped slot, or a track without samples: a row of +inf


@pytest.mark.gpu
@pytest.mark.parametrize("sep", [False, True], ids=["contiguous", "fixed"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_thresholds_and_cost(ctx, name, sep):
    """busca_ghost_thresholds per problem - a NaN entry, an empty group, each of the two `which` - and busca_gframe_cost on every slab: the class
    mask alone, then the blend with nan_first against the problem's own thresholds."""
    from busca_amd import _gframe_lib, _mgframe_lib
    lib, flib = _mgframe_lib.load(), _gframe_lib.load()
    r = Raw(ctx, name, sep)
    fill = r.rs.uniform(0, 1, (r.B + 2, r.R, r.M))
    fill[1, 0, 0] = np.nan                                         # the first problem's first entry: its active threshold is NaN
    pos = r.rs.uniform(0, 500, (r.n_total, 4))
    pos[:, 2:] += pos[:, :2] + 10
    d_pos = _dev(pos)
    for which in (3, 1):
        slab, p = r.slab(fill.copy())
        thr = _dev(np.full((r.B + 2, 2), CANARY))
        _mgframe_lib.check(lib.busca_mgframe_thresholds(p, 0.5, 1.0, which, *r.tail(), thr.data_ptr() + 16, *_where()))
        want_thr = np.full((r.B + 2, 2), CANARY)
        apps = {}
        for k in r.good:
            lr, sr = r.rows(k)
            n, m, na = len(lr), int(r.table[k, 7]), int(r.table[k, 1])
            if n == 0 or m == 0:
                continue
            apps[k] = app = _dev(np.ascontiguousarray(fill[1 + k][sr, :m]))
            o = _dev(np.full(2, CANARY))
            if which == 3:
                ctx.check(ctx.lib.busca_ghost_thresholds(ctx.h, app.data_ptr(), n, m, na, 0.5, 1.0, o.data_ptr(), _where()[1]))
            elif na:
                ctx.check(ctx.lib.busca_ghost_thresholds(ctx.h, app.data_ptr(), na, m, na, 0.5, 1.0, o.data_ptr(), _where()[1]))
            want_thr[1 + k] = _host(o)
        got_thr = _host(thr)
        assert same(got_thr, want_thr), (name, sep, which)
        assert same(_host(slab), fill)                             # the costs are read only
    assert (want_thr[1:-1] == CANARY).any() and np.isnan(got_thr[1, 0])
    # cost: the class mask alone (pos NULL), then the blend and nan_first with thr[k]
    thr_in = r.rs.uniform(0.4, 0.9, (r.B, 2))
    thr_in[0, 1] = np.nan
    d_thr = _dev(thr_in)
    for masked in (True, False):
        slab, p = r.slab(fill.copy())
        args = (None, None, 0.0, r.d["tl"].data_ptr(), r.d["dl"].data_ptr(), None) if masked else \
            (d_pos.data_ptr(), r.d["boxes"].data_ptr(), 0.4, r.d["tl"].data_ptr(), r.d["dl"].data_ptr(), d_thr.data_ptr())
        _mgframe_lib.check(lib.busca_mgframe_cost(p, *args, *r.tail(), *_where()))
        want = fill.copy()
        for k, app in apps.items():
            lr, sr = r.rows(k)
            n, m, na = len(lr), int(r.table[k, 7]), int(r.table[k, 1])
            o = _dev(np.zeros((n, m)))
            tl, dl = _dev(r.tl[lr]), r.d["dl"][r.dets(k)]
            if masked:
                _gframe_lib.check(flib.busca_gframe_cost(app.data_ptr(), None, None, n, m, 0.0, tl.data_ptr(), dl.data_ptr(), na, None, o.data_ptr(), *_where()))
            else:
                p_k = _dev(pos[lr])
                _gframe_lib.check(flib.busca_gframe_cost(app.data_ptr(), p_k.data_ptr(), r.d["boxes"][r.dets(k)].data_ptr(), n, m, 0.4, tl.data_ptr(),
                                                         dl.data_ptr(), na, d_thr.data_ptr() + 16 * k, o.data_ptr(), *_where()))
            want[1 + k][sr, :m] = _host(o)
        assert same(_host(slab), want), (name, sep, masked)
        assert np.isnan(want[1:-1]).sum() > np.isnan(fill[1:-1]).sum()


def random_matching(rs, n, m):
    """A partial matching of n rows and m columns as the solver's two vectors."""
    r2c, c2r = np.full(n, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    k = min(n, m)
    rows, cols = rs.permutation(n)[:k - k // 4], rs.permutation(m)[:k - k // 4]
    r2c[rows], c2r[cols] = cols, rows
    return r2c, c2r


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_keep(ctx, name):
    """busca_gframe_keep per problem: a cost equal to its threshold (not kept), one ulp below it (kept) and NaN; all rows at once on contiguous
    slabs; the active stage with its mask down the problem's own inactive rows and the merging inactive stage on slabs with a fixed inactive row."""
    from busca_amd import _gframe_lib, _mgframe_lib
    lib, flib = _mgframe_lib.load(), _gframe_lib.load()
    for sep in (False, True):
        r = Raw(ctx, name, sep)
        fill = r.rs.uniform(0, 1, (r.B + 2, r.R, r.M))
        thr = np.tile(np.array([0.5, 0.6]), (r.B, 1))
        stages = [(1, 0, 1), (2, 1, 0)] if sep else [(0, 0, 0)]
        match = {}
        for k in r.good:                                           # one matching per stage and problem; its first pairs sit on the threshold's edge
            lr, sr = r.rows(k)
            n, m, na = len(lr), int(r.table[k, 7]), int(r.table[k, 1])
            for stage, _, _ in stages:
                lo, hi = (0, n) if stage == 0 else (0, na) if stage == 1 else (na, n)
                r2c, c2r = random_matching(r.rs, hi - lo, m)
                for q, i in enumerate(np.nonzero(r2c >= 0)[0][:3]):
                    t = thr[k, 0 if lo + i < na else 1]
                    fill[1 + k, sr[lo + i], r2c[i]] = (t, np.nextafter(t, -np.inf), np.nan)[q]
                match[k, stage] = (r2c, c2r, lo, hi)
        slab, p = r.slab(fill.copy())
        d_thr = _dev(thr)
        td, dt = _dev(np.full((r.B + 2, r.R), -77, dtype=np.int32)), _dev(np.full((r.B + 2, r.M), -77, dtype=np.int32))
        want_td, want_dt, want = np.full((r.B + 2, r.R), -77, dtype=np.int32), np.full((r.B + 2, r.M), -77, dtype=np.int32), fill.copy()
        singles = {}
        for stage, merge, mask in stages:
            r2c_all, c2r_all = np.full((r.B, r.R), -5, dtype=np.int32), np.full((r.B, r.M), -5, dtype=np.int32)
            for k in r.good:
                r2c, c2r, lo, hi = match[k, stage]
                r2c_all[k, :hi - lo], c2r_all[k, :len(c2r)] = r2c, c2r
            d_r2c, d_c2r = _dev(r2c_all), _dev(c2r_all)            # held: two temporaries in one call would share their memory
            _mgframe_lib.check(lib.busca_mgframe_keep(p, d_r2c.data_ptr(), d_c2r.data_ptr(), d_thr.data_ptr(), td.data_ptr() + 4 * r.R,
                                                      dt.data_ptr() + 4 * r.M, stage, merge, mask, *r.tail(), *_where()))
            for k in r.good:
                lr, sr = r.rows(k)
                n, m, na = len(lr), int(r.table[k, 7]), int(r.table[k, 1])
                if m == 0:
                    continue
                if k not in singles:
                    singles[k] = (_dev(np.ascontiguousarray(fill[1 + k][sr, :m]).reshape(n, m)), _dev(np.full(max(n, 1), -77, dtype=np.int32)),
                                  _dev(np.full(m, -77, dtype=np.int32)))
                cost, s_td, s_dt = singles[k]
                r2c, c2r, lo, hi = match[k, stage]
                s_r2c, s_c2r = _dev(r2c), _dev(c2r)
                _gframe_lib.check(flib.busca_gframe_keep(cost.data_ptr() if n else None, n, m, lo, hi, na, s_r2c.data_ptr() if hi > lo else None,
                                                         s_c2r.data_ptr(), d_thr.data_ptr() + 16 * k, s_td.data_ptr() if n else None, s_dt.data_ptr(),
                                                         merge, (na if mask and n > na else -1), *_where()))
        for k, (cost, s_td, s_dt) in singles.items():
            lr, sr = r.rows(k)
            n, m = len(lr), int(r.table[k, 7])
            want[1 + k][sr, :m] = _host(cost)
            want_td[1 + k, sr] = _host(s_td)[:n]
            v = _host(s_dt)
            want_dt[1 + k, :m] = np.where(v >= 0, sr[np.clip(v, 0, max(n - 1, 0))] if n else v, v)      # det_track holds slab rows
        assert same(_host(slab), want) and same(_host(td), want_td) and same(_host(dt), want_dt), (name, sep)
        assert (want_td[1:-1] >= 0).any() and (want_td[1:-1] == -1).any()
        if sep and name != "one":
            assert np.isnan(want[1:-1]).sum() > np.isnan(fill[1:-1]).sum()      # the mask went down inactive rows


@pytest.mark.gpu
@pytest.mark.parametrize("sep", [False, True], ids=["contiguous", "fixed"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_apply(ctx, name, sep):
    """busca_gframe_apply per problem: matched rows into both rings with the problem's frame number, new tracks ranked among the problem's own
    columns into its own free range, the range running out (-2), skipped slots, may_start; everything else bit-identical."""
    from busca_amd import _gframe_lib, _mgframe_lib
    r = Raw(ctx, name, sep)
    am, ag, bm, bg = clone_motion(ctx, r.motion), clone_gallery(ctx, r.gallery), clone_motion(ctx, r.motion), clone_gallery(ctx, r.gallery)
    td, dt = np.full((r.B + 2, r.R), -1, dtype=np.int32), np.full((r.B + 2, r.M), -1, dtype=np.int32)
    plain = {}
    for k in range(r.B):
        lr, sr = r.rows(k)
        n, m = len(lr), int(r.table[k, 7])
        r2c, c2r = random_matching(r.rs, n, m)
        plain[k] = (r2c, c2r)
        td[1 + k, sr] = r2c
        dt[1 + k, :m] = np.where(c2r >= 0, sr[np.clip(c2r, 0, max(n - 1, 0))] if n else c2r, c2r)
    ds = _dev(np.full((r.B + 2, r.M), -77, dtype=np.int32))
    d_td, d_dt = _dev(td), _dev(dt)                                # held: two temporaries in one call would share their memory
    _mgframe_lib.check(_mgframe_lib.load().busca_mgframe_apply(
        *rings(am), r.H, ag._gallery.data_ptr(), ag._count.data_ptr(), ag._newest.data_ptr(), ag._mv_seen.data_ptr(), r.budget, r.E,
        d_td.data_ptr() + 4 * r.R, d_dt.data_ptr() + 4 * r.M, r.d["feats"].data_ptr(), r.d["boxes"].data_ptr(), r.d["may"].data_ptr(),
        r.d["free"].data_ptr(), *r.tail(), ds.data_ptr() + 4 * r.M, *_where()))
    want_ds = np.full((r.B + 2, r.M), -77, dtype=np.int32)
    for k in r.good:
        lr, sr = r.rows(k)
        n, m, row = len(lr), int(r.table[k, 7]), r.table[k]
        if m == 0:
            continue
        r2c, c2r = plain[k]
        o = _dev(np.full(m, -77, dtype=np.int32))
        free = r.d["free"][int(row[8]):int(row[8] + row[9])]
        s_slot, s_r2c, s_c2r = _dev(r.slot[lr]), _dev(r2c), _dev(c2r)
        _gframe_lib.check(_gframe_lib.load().busca_gframe_apply(
            *rings(bm), r.H, bg._gallery.data_ptr(), bg._count.data_ptr(), bg._newest.data_ptr(), bg._mv_seen.data_ptr(), r.budget, r.E, r.S,
            s_slot.data_ptr() if n else None, n, s_r2c.data_ptr() if n else None, s_c2r.data_ptr(), r.d["feats"][r.dets(k)].data_ptr(),
            r.d["boxes"][r.dets(k)].data_ptr(), m, int(row[11]), r.d["may"][r.dets(k)].data_ptr(), free.data_ptr(), int(row[9]), o.data_ptr(), *_where()))
        want_ds[1 + k, :m] = _host(o)
    assert same(_host(ds), want_ds), (name, sep)
    for key, x, y in zip(MOTION_KEYS + GALLERY_KEYS, motion_state(am) + [_host(getattr(ag, q)) for q in GALLERY_KEYS],
                         motion_state(bm) + [_host(getattr(bg, q)) for q in GALLERY_KEYS]):
        assert same(x, y), (name, sep, key)
    assert (want_ds[1:-1] == -2).any() and (want_ds[1:-1] >= 0).any() and not same(motion_state(am)[1], motion_state(r.motion)[1])
