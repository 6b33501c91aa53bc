#!/usr/bin/env python3
"""Generate tests/golden/byte_tracker.npz, the fixture of tests/test_byte_tracker_replay.py: BYTETracker.update of the reference
(adapters/ByteTrack/yolox/tracker/byte_tracker.py) itself, run over three scripted scenes and recorded frame by frame.  Run from the repo root
where the reference is present:

    python tests/golden/make_golden_byte_tracker.py

byte_tracker.py is loaded from its file with the stand-ins of make_golden_appearance.py and: `lap.lapjv` as make_golden_assign.solve_padded,
`cython_bbox.bbox_overlaps` as oracle.geometry.iou_matrix, `cv2` as oracle/ref_shims, np.float = float, `yolox.tracker.kalman_filter` / `.basetrack`
from adapters/CenterTrack/src/lib/utils/mot_online (the fallback byte_tracker.py names itself), `yolox.tracker.matching` from the ByteTrack tree,
and empty modules for busca.network / .tracking / .visualization (use_busca is off).  While a scene runs, matching.iou_distance,
matching.linear_assignment, remove_duplicate_stracks and BaseTrack.mark_removed are wrapped: the reference's own cost matrices, limits, results,
duplicate decisions and removals are what is recorded.  BaseTrack._count is reset before each scene.

The fixture holds arrays only.  Per scene S in small, small_mot20, crowded (every `*_begin` is a prefix-sum table; frames are 0-based in it):
  S_params [6]                  track_thresh, track_buffer, match_thresh, mot20, frames, the store capacity the replay uses
  S_det [M,5], S_det_begin      the detections of every frame as given (tlbr, score)
  S_trk_int [T,7], S_trk_mean [T,8], S_trk_cov [T,8,8], S_trk_begin    after update(): every track of tracked_stracks, then lost_stracks: track_id,
                                state, is_activated, start_frame, frame_id, tracklet_len, list (0 tracked, 1 lost); mean; covariance
  S_removed, S_removed_begin    the ids mark_removed was called on in the frame
  S_out_id, S_out_tlwh, S_out_begin     the returned output_stracks
  S_dup_a, S_dup_b (+ _begin)   the ids remove_duplicate_stracks took out of the tracked / the lost list
  S_unassigned (+ _begin)       the ids of unassigned_stracks (:364), what step 3b would work on
  S_pool_tlbr [P,4] (+ _begin)  the predicted boxes of strack_pool, the rows of round one
  S_dup_cost, S_dup_age_a, S_dup_age_b (+ _begin)   what remove_duplicate_stracks saw: its IoU cost matrix (row-major, [len a, len b]) and
                                frame_id - start_frame of the tracked (a) and the lost (b) list before it
  S_rnd_rows, S_rnd_cols, S_rnd_pairs, S_rnd_cost (+ _begin, indexed 3 * frame + round), S_rnd_limit, S_rnd_kept    the three rounds: row track ids,
                                column detection indices into the frame's list, pairs (track id, detection index), the cost matrix row-major
restatement_err_mean / _cov / _cost [3]   per scene, the largest distance of tests/byte_replay.NumpyBackend driven by tests/byte_replay.Replay
                                from the reference: err_mean / err_cov of tests/test_kalman_filter.py over every held track of every frame, and the
                                largest absolute difference over every recorded matrix entry

The scripts are open loop, so small_mot20 sees small's detections.  `check_scenes` asserts that together they hold every case the tests rely on
(CASES), and on every frame of every scene: each round's optimum unique by more than MARGIN, no cost within MARGIN of its limit, no duplicate cost
within MARGIN of 0.15, no score within MARGIN of a threshold except the three deliberate equalities; and MARGIN > 1000 x 20 x every restatement
error, so a result within the tests' bars cannot change a decision."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_assign import solve_padded, unique  # noqa: E402
from oracle import geometry as ogeo  # noqa: E402
from tests import byte_replay as br  # noqa: E402

MARGIN = 1e-6
TRACK_THRESH, TRACK_BUFFER, MATCH_THRESH = 0.5, 5, 0.8
DET_THRESH = TRACK_THRESH + 0.1
SIZE = (1080, 1920)
CASES = ("activated_in_frame_one", "birth_confirmed_in_round_three", "unconfirmed_removed", "kept_by_low_score", "lost_stays_lost_on_low_score",
         "lost_reactivated", "lost_expired", "birth_after_expiry", "middling_score_starts_nothing", "score_equal_det_thresh_starts",
         "score_equal_track_thresh", "score_equal_low_thresh", "frame_without_detections", "frame_of_low_scores_only", "optimum_is_not_greedy",
         "fuse_score_changes_pairs", "duplicate_from_lost", "duplicate_from_tracked_older_lost", "duplicate_tie", "crowded_tiles")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _lapjv(cost, extend_cost=True, cost_limit=np.inf):
    assert extend_cost
    x = solve_padded(np.asarray(cost, dtype=np.float64), cost_limit)
    y = np.full(cost.shape[1], -1, dtype=np.int64)
    y[x[x >= 0]] = np.nonzero(x >= 0)[0]
    return float(cost[np.nonzero(x >= 0)[0], x[x >= 0]].sum()), x, y


def load_reference():
    """-> the byte_tracker module of the reference, imported with the stand-ins the docstring lists.  sys.modules and sys.path are left as they
    were: the module keeps what it imported (`matching`, `BaseTrack`), and a later `import busca` finds the real package."""
    if not hasattr(np, "float"):
        np.float = float
    names = ("lap", "cython_bbox", "cv2", "yolox", "yolox.tracker", "yolox.tracker.kalman_filter", "yolox.tracker.basetrack", "yolox.tracker.matching",
             "yolox.tracker.byte_tracker", "busca", "busca.network", "busca.tracking", "busca.visualization")
    saved, path = {k: sys.modules.pop(k, None) for k in names}, list(sys.path)
    try:
        return _load_reference()
    finally:
        sys.path[:] = path
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def _load_reference():
    mot = os.path.join(REF, "adapters/CenterTrack/src/lib/utils/mot_online")
    kfm = _load("yolox.tracker.kalman_filter", os.path.join(mot, "kalman_filter.py"))
    base = _load("yolox.tracker.basetrack", os.path.join(mot, "basetrack.py"))
    shims = os.path.join(ROOT, "oracle", "ref_shims")
    if shims not in sys.path:
        sys.path.insert(0, shims)                                # cv2
    lap = types.ModuleType("lap")
    lap.lapjv = _lapjv
    cb = types.ModuleType("cython_bbox")
    cb.bbox_overlaps = lambda a, b: ogeo.iou_matrix(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    yolox, tracker, busca = types.ModuleType("yolox"), types.ModuleType("yolox.tracker"), types.ModuleType("busca")
    yolox.__path__, tracker.__path__, busca.__path__ = [], [], []
    yolox.tracker, tracker.kalman_filter, tracker.basetrack = tracker, kfm, base
    mods = {"lap": lap, "cython_bbox": cb, "yolox": yolox, "yolox.tracker": tracker, "busca": busca}
    for name, attrs in (("busca.network", ("BUSCA",)), ("busca.tracking", ("center_distance",)), ("busca.visualization", ("plot_box",))):
        mods[name] = types.ModuleType(name)
        for a in attrs:
            setattr(mods[name], a, None)                         # never called: use_busca is off
    sys.modules.update(mods)
    tracker.matching = _load("yolox.tracker.matching", os.path.join(REF, "adapters/ByteTrack/yolox/tracker/matching.py"))
    return _load("yolox.tracker.byte_tracker", os.path.join(REF, "adapters/ByteTrack/yolox/tracker/byte_tracker.py"))


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def _box(x, y, score, w=40.0, h=80.0):
    return [x, y, x + w, y + h, score]


def small_script():
    """40 frames, nine areas 300 px apart, each its own story (the frame numbers below are 1-based) -> [F] of [m,5]."""
    rs = np.random.RandomState(5)
    F, frames = 40, []
    for f in range(1, F + 1):
        dets = []

        def area(k, wobble):
            """The corner of area k in this frame: a slow drift and a wobble shared by every box of the area."""
            return (100.0 + 300 * (k % 5) + 1.0 * f + wobble * rs.uniform(-1, 1), 100.0 + 400 * (k // 5) + 0.5 * f + wobble * rs.uniform(-1, 1),
                    80.0 * (1 + 0.01 * wobble * rs.uniform(-1, 1)))
        corners = [area(k, 0.2 if k < 3 else 1.5) for k in range(10)]
        hi = 0.3 if f == 30 else 0.9                             # frame 30: low scores only

        def put(k, dx, score, dy=0.0):
            x, y, h = corners[k]
            dets.append(_box(x + dx, y + dy, score, h=h))
        # area 4 first, so that its track holds slot 0: lost after frame 5, offered a low score in frame 7, expired in frame 11
        if f <= 5:
            put(4, 0, hi)
        if f == 7:
            put(4, 0, 0.3)
        # area 0: A (frames 1-7) and, 2 px beside it, B (from frame 3): in frame 8 A is lost and the younger B, tracked, is its duplicate
        if f <= 7:
            put(0, 0, hi)
        if f >= 3:
            put(0, 2, hi - 0.02)
        # area 1: A (always) and B (frames 5-9) 2 px beside it: in frame 10 the younger B is lost and a duplicate
        put(1, 0, hi)
        if 5 <= f <= 9:
            put(1, 2, hi - 0.02)
        # area 2: L (frames 1-3) and T (from frame 2): in frame 4 both are equally old
        if f <= 3:
            put(2, 0, hi)
        if f >= 2:
            put(2, 2, hi - 0.02)
        # area 3: K, kept by a low score in frame 7; a stray box half on it in frame 9 starts a track that frame 10 removes
        put(3, 0, 0.3 if f == 7 else hi)
        if f == 9:
            put(3, 14, 0.85)
        # area 5: two tracks 30 px apart; in frame 12 their detections sit so that the row-wise greedy choice is not the optimum
        if f < 12:
            put(5, 0, hi)
            put(5, 30, hi - 0.02)
        else:
            put(5, 12, hi)
            put(5, -14, hi - 0.02)
        # area 6: Z, whose detection scores exactly track_thresh in frame 16 and exactly 0.1 in frame 17
        put(6, 0, TRACK_THRESH if f == 16 else 0.1 if f == 17 else hi)
        # area 7: a lone detection scoring exactly det_thresh in frame 14 (after the expiry), one between the thresholds in frame 20
        if f == 14:
            put(7, 0, DET_THRESH)
        if f == 20:
            put(7, 0, 0.55)
        # area 8: X; in frame 38 the nearer box scores low enough for fuse_score to prefer the other one
        if f == 38:
            put(8, 10, 0.95)
            put(8, -7, 0.55)
        else:
            put(8, 0, hi)
        # a late birth far from everything, confirmed one frame on
        if f >= 33:
            put(9, 0, hi)
        if f == 25:
            dets = []                                            # frame 25: no detections
        frames.append(np.array(dets, dtype=np.float64).reshape(-1, 5))
    return frames


def crowded_script():
    """12 frames: 22 walkers on a grid (4 more from frame 4), two of them unseen in frames 5-6, two scoring low in frame 7, and from frame 3 on
    48 boxes of clutter per frame: 30 second-round scores, 18 below 0.1 -> [F] of [m,5]."""
    rs = np.random.RandomState(11)
    n, F = 26, 12
    pos = np.stack([80.0 + 130 * (np.arange(n) % 7), 60.0 + 170 * (np.arange(n) // 7)], 1) + rs.uniform(-8, 8, (n, 2))
    vel, h = rs.uniform(-2.5, 2.5, (n, 2)), rs.uniform(70, 95, n)
    frames = []
    for f in range(1, F + 1):
        dets = []
        for k in range(n):
            if (k >= 22 and f < 4) or (k in (3, 7) and f in (5, 6)):
                continue
            p = pos[k] + vel[k] * f + rs.uniform(-1.5, 1.5, 2)
            hh = h[k] * rs.uniform(0.98, 1.02)
            score = rs.uniform(0.15, 0.45) if (k in (10, 11) and f == 7) else rs.uniform(0.65, 0.97)
            dets.append(_box(p[0], p[1], score, w=0.5 * hh, h=hh))
        if f >= 3:
            for j in range(48):
                p, hh = rs.uniform([0, 0], [1000, 760]), rs.uniform(50, 110)
                dets.append(_box(p[0], p[1], rs.uniform(0.12, 0.45) if j < 30 else rs.uniform(0.01, 0.09), w=0.5 * hh, h=hh))
        order = rs.permutation(len(dets))                        # the rounds' columns are scattered over the frame's list
        frames.append(np.array(dets, dtype=np.float64).reshape(-1, 5)[order])
    return frames


# ---- recording --------------------------------------------------------------------------------------------------------------
def run_scene(bt, frames, mot20, capacity):
    """BYTETracker.update over the frames -> the scene's arrays, without the prefix."""
    matching, base = bt.matching, bt
    base.BaseTrack._count = 0
    log = {"iou": [], "la": [], "dup": [], "removed": []}
    orig = (matching.iou_distance, matching.linear_assignment, bt.remove_duplicate_stracks, base.BaseTrack.mark_removed)

    def iou_distance(a, b):
        cost = orig[0](a, b)
        log["iou"].append(([t.track_id for t in a], [np.array(t.tlbr) for t in a], [float(t.score) for t in b], np.array(cost, dtype=np.float64)))
        return cost

    def linear_assignment(cost, thresh):
        res = orig[1](cost, thresh)
        log["la"].append((np.array(cost, dtype=np.float64), float(thresh), np.asarray(res[0], dtype=np.int64).reshape(-1, 2),
                          np.asarray(res[1], dtype=np.int64), np.asarray(res[2], dtype=np.int64)))
        return res

    def remove_duplicate_stracks(a, b):
        ra, rb = orig[2](a, b)
        log["dup"].append(([t.track_id for t in a if t not in ra], [t.track_id for t in b if t not in rb],
                           [(t.frame_id - t.start_frame) for t in a], [(t.frame_id - t.start_frame) for t in b]))
        return ra, rb

    def mark_removed(self):
        log["removed"].append(self.track_id)
        orig[3](self)

    matching.iou_distance, matching.linear_assignment, bt.remove_duplicate_stracks, base.BaseTrack.mark_removed = (
        iou_distance, linear_assignment, remove_duplicate_stracks, mark_removed)
    try:
        args = types.SimpleNamespace(track_thresh=TRACK_THRESH, track_buffer=TRACK_BUFFER, match_thresh=MATCH_THRESH, mot20=mot20)
        tracker = bt.BYTETracker(args)
        lists = {k: [] for k in ("det", "trk_int", "trk_mean", "trk_cov", "removed", "out_id", "out_tlwh", "dup_a", "dup_b", "unassigned",
                                 "rnd_rows", "rnd_cols", "rnd_pairs", "rnd_cost", "pool_tlbr", "dup_cost", "dup_age_a", "dup_age_b")}
        limits = []
        for f, det in enumerate(frames):
            for v in log.values():
                del v[:]
            out = tracker.update(det.copy(), SIZE, SIZE)
            assert len(log["iou"]) == 4 and len(log["la"]) == 3 and len(log["dup"]) == 1
            scores = det[:, 4]
            cols = [np.nonzero(scores > TRACK_THRESH)[0], np.nonzero(np.logical_and(scores > 0.1, scores < TRACK_THRESH))[0]]
            cols.append(cols[0][log["la"][0][4]])                # round three: round one's unmatched columns
            rows = [np.array(log["iou"][r][0], dtype=np.int64) for r in range(3)]
            for r in range(3):
                cost, limit, matches, ua, ub = log["la"][r]
                assert cost.shape == (len(rows[r]), len(cols[r])) and log["iou"][r][2] == [float(s) for s in scores[cols[r]]]
                lists["rnd_rows"].append(rows[r])
                lists["rnd_cols"].append(cols[r].astype(np.int64))
                lists["rnd_pairs"].append(np.stack([rows[r][matches[:, 0]], cols[r][matches[:, 1]]], 1).reshape(-1).astype(np.int64))
                lists["rnd_cost"].append(cost.reshape(-1))
                limits.append(limit)
            second_left = [int(rows[1][i]) for i in log["la"][1][3]]
            first_left = [int(rows[0][i]) for i in log["la"][0][3]]
            lists["unassigned"].append(np.array(second_left + [i for i in first_left if i not in set(rows[1].tolist())], dtype=np.int64))
            both = tracker.tracked_stracks + tracker.lost_stracks
            lists["trk_int"].append(np.array([[t.track_id, t.state, int(t.is_activated), t.start_frame, t.frame_id, t.tracklet_len,
                                               int(k >= len(tracker.tracked_stracks))] for k, t in enumerate(both)], dtype=np.int64).reshape(-1, 7))
            lists["trk_mean"].append(np.array([t.mean for t in both], dtype=np.float64).reshape(-1, 8))
            lists["trk_cov"].append(np.array([t.covariance for t in both], dtype=np.float64).reshape(-1, 8, 8))
            lists["det"].append(det)
            lists["removed"].append(np.array(log["removed"], dtype=np.int64))
            lists["out_id"].append(np.array([t.track_id for t in out], dtype=np.int64))
            lists["out_tlwh"].append(np.array([t.tlwh for t in out], dtype=np.float64).reshape(-1, 4))
            lists["dup_a"].append(np.array(log["dup"][0][0], dtype=np.int64))
            lists["dup_b"].append(np.array(log["dup"][0][1], dtype=np.int64))
            lists["pool_tlbr"].append(np.array(log["iou"][0][1], dtype=np.float64).reshape(-1, 4))
            lists["dup_cost"].append(log["iou"][3][3].reshape(-1))
            lists["dup_age_a"].append(np.array(log["dup"][0][2], dtype=np.int64))
            lists["dup_age_b"].append(np.array(log["dup"][0][3], dtype=np.int64))
    finally:
        matching.iou_distance, matching.linear_assignment, bt.remove_duplicate_stracks, base.BaseTrack.mark_removed = orig
    out = {"params": np.array([TRACK_THRESH, TRACK_BUFFER, MATCH_THRESH, float(mot20), len(frames), capacity], dtype=np.float64),
           "rnd_limit": np.array(limits, dtype=np.float64), "rnd_kept": np.ones(len(limits), dtype=np.uint8)}
    shared = {"trk_mean": "trk", "trk_cov": "trk", "trk_int": "trk", "out_id": "out", "out_tlwh": "out"}
    for key, parts in lists.items():
        tail = {"det": (0, 5), "trk_int": (0, 7), "trk_mean": (0, 8), "trk_cov": (0, 8, 8), "out_tlwh": (0, 4), "pool_tlbr": (0, 4)}.get(key, (0,))
        dtype = np.float64 if key in ("det", "trk_mean", "trk_cov", "out_tlwh", "rnd_cost", "pool_tlbr", "dup_cost") else np.int64
        out[key] = np.concatenate([np.zeros(tail, dtype=dtype)] + parts)
        rows_of = [len(p) // 2 if key == "rnd_pairs" else len(p) for p in parts]
        if key == "rnd_pairs":
            out[key] = out[key].reshape(-1, 2)
        out["%s_begin" % shared.get(key, key)] = np.concatenate([[0], np.cumsum(rows_of)]).astype(np.int64)
    return out


# ---- what the scenes must hold ------------------------------------------------------------------------------------------------
def check_scenes(scenes):
    """The CASES, in the `seen`-set style, and the margins that keep exact comparisons meaningful.  scenes: name -> (params, frames) as
    byte_replay.load_scene gives them: the fixture alone is enough."""
    seen, exact = set(), {"track": 0, "low": 0, "det": 0}
    for name, (params, frames) in scenes.items():
        born = {}                                                # id -> start_frame
        expired_at = None
        for f, fr in enumerate(frames):
            scores, ints = fr["det"][:, 4], fr["trk_int"]
            side = dict(before={} if f == 0 else {int(i): int(s) for i, s in frames[f - 1]["trk_int"][:, :2]}, pool_tlbr=fr["pool_tlbr"],
                        dup_cost=fr["dup_cost"], dup_ages=(fr["dup_age_a"], fr["dup_age_b"]))
            r1, r2, r3 = fr["rounds"]
            matched = {int(j) for r in fr["rounds"] for _, j in r["pairs"]}
            new = [int(i) for i, s in zip(ints[:, 0], ints[:, 3]) if s == f + 1 and int(i) not in born]
            for i in new:
                born[i] = f + 1
            # ---- margins
            for th, key in ((0.1, "low"), (TRACK_THRESH, "track"), (DET_THRESH, "det")):
                d = np.abs(scores - th)
                exact[key] += int((d == 0).sum()) if name == "small" else 0
                assert not np.logical_and(d > 0, d <= MARGIN).any(), (name, f + 1, "a score within the margin of", th)
            for k, r in enumerate(fr["rounds"]):
                c = r["cost"]
                if c.size:
                    assert np.abs(c - r["limit"]).min() > MARGIN, (name, f + 1, k, "a cost within the margin of the limit")
                    x = np.full(len(r["rows"]), -1, dtype=np.int64)
                    for i, j in r["pairs"]:
                        x[list(r["rows"]).index(i)] = list(r["cols"]).index(j)
                    assert unique(c, r["limit"], x, MARGIN), (name, f + 1, k, "the optimum is not unique by the margin")
            if side["dup_cost"].size:
                assert np.abs(side["dup_cost"] - br.DUPLICATE_THRESH).min() > MARGIN, (name, f + 1, "a duplicate cost within the margin of 0.15")
            # ---- cases
            if f == 0 and len(ints) and ints[:, 2].all():
                seen.add("activated_in_frame_one")
            if len(fr["det"]) == 0:
                seen.add("frame_without_detections")
            elif (scores < TRACK_THRESH).all() and (scores > 0.1).any():
                seen.add("frame_of_low_scores_only")
            if len(r2["pairs"]):
                seen.add("kept_by_low_score")
            for i, j in r3["pairs"]:
                if born.get(int(i)) == f and f > 0:
                    seen.add("birth_confirmed_in_round_three")
            if set(r3["rows"].tolist()) - {int(i) for i, _ in r3["pairs"]}:
                seen.add("unconfirmed_removed")
            for i, j in r1["pairs"]:
                if side["before"].get(int(i)) == br.LOST:
                    seen.add("lost_reactivated")
            lo = fr["det"][np.logical_and(scores > 0.1, scores < TRACK_THRESH)]
            for k, i in enumerate(r1["rows"]):
                if side["before"].get(int(i)) == br.LOST and (r1["cost"].shape[1] == 0 or (r1["cost"][k] == 1).all()) and len(lo):
                    overlap = ogeo.iou_matrix(side["pool_tlbr"][k][None], br.detections_tlbr(lo))[0]
                    state = ints[list(ints[:, 0]).index(i), 1]
                    if (overlap > 0.6).sum() == 1 and state == br.LOST:
                        seen.add("lost_stays_lost_on_low_score")
            for i in fr["removed"]:
                if side["before"].get(int(i)) == br.LOST:
                    seen.add("lost_expired")
                    expired_at = f + 1 if expired_at is None else expired_at
            if new and expired_at is not None and f + 1 > expired_at + 1:
                seen.add("birth_after_expiry")
            for j in r1["cols"]:
                if int(j) not in matched:
                    if TRACK_THRESH < scores[j] < DET_THRESH:
                        seen.add("middling_score_starts_nothing")
                    if scores[j] == DET_THRESH and len(new) == sum(1 for q in r1["cols"] if int(q) not in matched and scores[q] >= DET_THRESH):
                        seen.add("score_equal_det_thresh_starts")
            if (scores == TRACK_THRESH).any():
                seen.add("score_equal_track_thresh")
            if (scores == 0.1).any():
                seen.add("score_equal_low_thresh")
            if r1["cost"].size and not params["mot20"]:
                greedy = br.NumpyBackend(0, ("greedy_rows",))._solve(r1["cost"], r1["limit"])
                pairs = sorted((int(r1["rows"][i]), int(r1["cols"][j])) for i, j in enumerate(greedy) if j >= 0)
                if pairs != sorted((int(a), int(b)) for a, b in r1["pairs"]):
                    seen.add("optimum_is_not_greedy")
            ages_a, ages_b = side["dup_ages"]
            if len(fr["dup_b"]):
                seen.add("duplicate_from_lost")
            for p, q in zip(*np.nonzero(side["dup_cost"] < br.DUPLICATE_THRESH)) if side["dup_cost"].size else ():
                if ages_a[p] < ages_b[q] and len(fr["dup_a"]):
                    seen.add("duplicate_from_tracked_older_lost")
                if ages_a[p] == ages_b[q] and len(fr["dup_a"]) and name == "small":
                    seen.add("duplicate_tie")
            if name == "crowded" and len(r1["rows"]) > 16 and len(fr["det"]) > 64 and any(side["before"].get(int(i)) == br.LOST for i in r1["rows"]):
                seen.add("crowded_tiles")
    a, b = scenes["small"][1], scenes["small_mot20"][1]
    for fa, fb in zip(a, b):
        pa, pb = [r["pairs"].tolist() for r in fa["rounds"]], [r["pairs"].tolist() for r in fb["rounds"]]
        if pa != pb:
            seen.add("fuse_score_changes_pairs")
            break
        assert np.array_equal(fa["trk_int"], fb["trk_int"])      # until fuse_score decides a pair the two scenes agree
    assert exact == {"track": 1, "low": 1, "det": 1}, exact
    assert seen == set(CASES), sorted(set(CASES) - seen)


def restatement(made, name):
    """The numpy backend over a recorded scene -> (err_mean, err_cov, err_cost), asserting that every decision is the reference's."""
    worst = [0.0]

    def on_frame(rp, want, f):
        for r in range(3):
            ref, got = want["rounds"][r], rp.backend.costs[r]
            rows = [(rp.pool if r < 2 else rp.unconfirmed)[i].track_id for i in rp.backend.rounds[r][0]]
            assert rows == ref["rows"].tolist() and rp.backend.rounds[r][1] == ref["cols"].tolist(), (name, f + 1, r)
            if ref["cost"].size:
                worst[0] = max(worst[0], float(np.abs(got - ref["cost"]).max()))
    bad, err, rp = br.replay_scene(name, br.NumpyBackend, on_frame=on_frame, g=made)
    assert bad is None, (name, bad)
    return err["mean"], err["cov"], worst[0], rp


def make(bt):
    made = {}
    for name, frames, mot20, capacity in (("small", small_script(), False, 16), ("small_mot20", small_script(), True, 16),
                                           ("crowded", crowded_script(), False, 40)):
        arrays = run_scene(bt, frames, mot20, capacity)
        made.update({"%s_%s" % (name, k): v for k, v in arrays.items()})
    check_scenes({name: br.load_scene(name, made) for name in br.SCENES})
    errs = []
    for name in br.SCENES:
        em, ec, ecost, rp = restatement(made, name)
        assert np.isfinite([em, ec, ecost]).all()
        assert MARGIN > 1000 * 20 * max(ecost, em), (name, em, ecost)      # a result within the bars cannot change a decision
        if name == "small":                                          # the expired track's slot is taken again by a later birth
            assert any(len(ids) > 1 for ids in rp.slot_history.values())
        errs.append([em, ec, ecost])
        print("%-12s %2d frames, %4d detections, %4d track-frames: restatement mean %.3g  covariance %.3g  cost %.3g"
              % (name, len(made[name + "_det_begin"]) - 1, len(made[name + "_det"]), len(made[name + "_trk_int"]), em, ec, ecost))
    errs = np.array(errs, dtype=np.float64)
    made.update(restatement_err_mean=errs[:, 0], restatement_err_cov=errs[:, 1], restatement_err_cost=errs[:, 2])
    return made


def main():
    made = make(load_reference())
    path = os.path.join(OUT, "byte_tracker.npz")
    np.savez_compressed(path, **made)
    print("wrote byte_tracker.npz: %d arrays, %d bytes" % (len(made), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
