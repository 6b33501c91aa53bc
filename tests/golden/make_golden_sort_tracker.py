#!/usr/bin/env python3
"""Generate tests/golden/sort_tracker.npz, the fixture of tests/test_sort_tracker_replay.py: the reference's StrongSORT tracker itself
(adapters/StrongSORT/deep_sort/tracker.py, track.py, linear_assignment.py, detection.py), driven as deep_sort_app.py:186-190 drives it -
camera_update where the frame has a matrix, predict, update - over three scripted scenes and recorded frame by frame.  Run from the repo root where
the reference is present:

    python tests/golden/make_golden_sort_tracker.py

The four files are loaded from the reference tree with these stand-ins, all written here: `opts.opt` (MC, MC_lambda, woC, EMA=True, EMA_alpha,
ecc={video: {str(frame): 3 x 3}}); `deep_sort.kalman_filter`: the KalmanFilter of adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py,
subclassed - only `project` and `update` are overridden (and `gating_distance`, to record what it returns) - so that they take `confidence` and
scale the innovation noise by 1 - confidence as upstream StrongSORT does (restated, as tests/test_sort_store.r_update_nsa restates it), with its
chi2inv95; `deep_sort.iou_matching.iou_cost`: the upstream function restated, as tests/test_sort_store.r_iou_cost; a cosine nearest-neighbour metric with budget 1 (what opts.py:137-138 sets under EMA); `cv2` from oracle/ref_shims;
empty busca.network / busca.tracking (use_busca is off).  The generator gives the tracker detections that have passed the confidence filter and
NMS (`preprocessing` is not in the tree).  Detection makes features float64 (detection.py:32): the reference's features and appearance costs are
float64.  While a scene runs, linear_assignment.min_cost_matching, KalmanFilter.gating_distance and Tracker._match are wrapped: the reference's own
clamped matrices, index lists, limits, pairs, gating distances and returned lists are what is recorded.

The fixture holds arrays only.  Per scene S in small, small_woc, crowded (every `*_begin` is a prefix-sum table; frames are 0-based in it):
  S_params [11]                 max_age, n_init, max_iou_distance, matching_threshold, EMA_alpha, MC, MC_lambda, woC, frames, the store capacity the
                                replay uses, the feature width
  S_det [M,5], S_feat [M,E] float32, S_det_begin     the detections of every frame as given (tlwh, confidence) and their features
  S_warp [F,3,3], S_warp_on [F] the matrix opt.ecc holds for the frame, where it holds one
  S_trk_int [T,5], S_trk_mean [T,8], S_trk_cov [T,8,8], S_trk_feat [T,E], S_trk_begin    after update(), every track in Tracker.tracks order:
                                track_id, state, hits, age, time_since_update; mean; covariance; features[-1]
  S_deleted (+ _begin)          the ids deleted in the frame
  S_out_id, S_out_tlwh, S_out_begin     the output rows of deep_sort_app.py:201-206
  S_match [K,2] (+ _begin), S_match_cascade [F], S_ut, S_ud (+ _begin)    Tracker._match's three lists as returned (track index into the frame's
                                Tracker.tracks, detection index), and how many of the matches the cascade made
  S_call_frame_begin [F+1]      the min_cost_matching calls of every frame that reached the solver; per call c: S_call_kind (0 cascade, 1 IoU),
  S_call_limit, S_call_rows, S_call_cols, S_call_pairs [k,2], S_call_cost, S_call_gate (+ _begin)    its max_distance, track indices, detection
                                indices, pairs, the clamped cost matrix row-major, and for a cascade call the gating distances row-major (+inf above GATE_KEPT = 100)
restatement_err_mean / _cov / _iou / _gate / _feat / _cost, _feat32 / _cost32 [3]   per scene, the largest distance of tests/sort_replay.NumpyBackend
                                from the reference: err_mean / err_cov of tests/test_kalman_filter.py over every held track of every frame, the
                                largest absolute difference over every recorded IoU / cascade matrix entry and feature entry, err_mean over the
                                gating distances; _feat32 / _cost32: the same with features, EMA and appearance cost in float32
appearance_margin_factor        the factor by which MARGIN_APP exceeds the float32 bar of the appearance plane (1000, or less and never below 100)

The scripts are open loop, so small_woc sees small's detections and warps.  `check_scenes` asserts, from the fixture alone, that together the
scenes hold every case of CASES, that the reference's unmatched detections are ascending in every frame (tests/sort_replay.py says why) and, on every
recorded call: the optimum unique by more than the margin of its plane, no admissible cost within it of the limit, no gating distance within
MARGIN of chi2inv95[4].  make() asserts besides, on the numpy restatement's unclamped planes, that no inadmissible cost is within the margin of its
limit either, that MARGIN exceeds 1000 x every float64 bar and MARGIN_APP the float32 bar by the recorded factor - so a result within the tests'
bars cannot change a decision - and that at a camera frame with rotation and scale predict-then-warp lies more than 1000 x the mean bar from
warp-then-predict: the order is observable."""
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

from make_golden_assign import unique  # noqa: E402
from tests import sort_replay as sr  # noqa: E402

MARGIN, MARGIN_APP = 1e-6, 1.2e-2
GATE_KEPT = 100.0                                              # a gating distance above this is recorded as +inf
MAX_AGE, N_INIT, MAX_IOU, MATCH_THRESH, EMA_ALPHA, MC_LAMBDA, E = 3, 3, 0.7, 0.3, 0.9, 0.98, 32
VIDEO = "scene"
U = 2.0 ** -53
CASES = ("birth_as_tentative", "confirmed_at_third_hit", "tentative_deleted_at_first_miss", "deleted_only_beyond_max_age", "beyond_max_age_in_no_stage",
         "slot_reused", "rematched_above_level_0", "level_priority", "rejected_on_appearance_rescued_by_iou", "stale_confirmed_not_in_iou_stage",
         "matching_feature_rejected_by_gate", "mc_blend_changes_pair", "optimum_is_not_greedy", "crowded_tiles", "frame_without_detections",
         "confidence_0_and_0999", "camera_rotation_and_scale", "camera_matrix_replaced_by_identity", "frame_without_matrix")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---- stand-ins ----------------------------------------------------------------------------------------------------------------
def _kalman_module():
    base = _load("ref_mot_online_kalman_filter", os.path.join(REF, "adapters/CenterTrack/src/lib/utils/mot_online/kalman_filter.py"))

    class KalmanFilter(base.KalmanFilter):
        """Upstream StrongSORT's NSA filter: project and update take the detection confidence, and the innovation noise is scaled by 1 - confidence.
        With the observation matrix [I 0] the projection is the leading block of the state, exactly; update is the base class's own, which asks
        project for the innovation covariance."""
        gate_log = []
        _confidence = 0.0

        def project(self, mean, covariance, confidence=None):
            c = self._confidence if confidence is None else confidence
            w, h = self._std_weight_position, mean[3]
            noise = np.square([(1 - c) * s for s in (w * h, w * h, 1e-1, w * h)])
            return np.array(mean[:4], dtype=np.float64), covariance[:4, :4] + np.diag(noise)

        def update(self, mean, covariance, measurement, confidence=.0):
            self._confidence = confidence
            try:
                return base.KalmanFilter.update(self, mean, covariance, measurement)
            finally:
                self._confidence = 0.0

        def gating_distance(self, mean, covariance, measurements, only_position=False, metric="maha"):
            d = base.KalmanFilter.gating_distance(self, mean, covariance, measurements, only_position, metric)
            KalmanFilter.gate_log.append(np.array(d, dtype=np.float64))
            return d

    mod = types.ModuleType("deep_sort.kalman_filter")
    mod.KalmanFilter, mod.chi2inv95 = KalmanFilter, base.chi2inv95
    return mod


def _iou_module():
    """iou_matching.iou / iou_cost of upstream StrongSORT, restated."""
    mod = types.ModuleType("deep_sort.iou_matching")

    def iou(bbox, candidates):
        bbox_tl, bbox_br = bbox[:2], bbox[:2] + bbox[2:]
        candidates_tl, candidates_br = candidates[:, :2], candidates[:, :2] + candidates[:, 2:]
        tl = np.c_[np.maximum(bbox_tl[0], candidates_tl[:, 0])[:, np.newaxis], np.maximum(bbox_tl[1], candidates_tl[:, 1])[:, np.newaxis]]
        br = np.c_[np.minimum(bbox_br[0], candidates_br[:, 0])[:, np.newaxis], np.minimum(bbox_br[1], candidates_br[:, 1])[:, np.newaxis]]
        wh = np.maximum(0., br - tl)
        area_intersection = wh.prod(axis=1)
        return area_intersection / (bbox[2:].prod() + candidates[:, 2:].prod(axis=1) - area_intersection)

    def iou_cost(tracks, detections, track_indices=None, detection_indices=None):
        if track_indices is None:
            track_indices = np.arange(len(tracks))
        if detection_indices is None:
            detection_indices = np.arange(len(detections))
        cost_matrix = np.zeros((len(track_indices), len(detection_indices)))
        for row, track_idx in enumerate(track_indices):
            if tracks[track_idx].time_since_update > 1:
                cost_matrix[row, :] = 1e+5
                continue
            bbox = tracks[track_idx].to_tlwh()
            candidates = np.asarray([detections[i].tlwh for i in detection_indices])
            cost_matrix[row, :] = 1. - iou(bbox, candidates)
        return cost_matrix

    mod.iou, mod.iou_cost = iou, iou_cost
    return mod


class CosineMetric:
    """NearestNeighborDistanceMetric("cosine", matching_threshold, budget=1) of upstream deep_sort, restated."""

    def __init__(self, matching_threshold, budget=1):
        self.matching_threshold, self.budget, self.samples = matching_threshold, budget, {}

    def partial_fit(self, features, targets, active_targets):
        for feature, target in zip(features, targets):
            self.samples.setdefault(target, []).append(feature)
            if self.budget is not None:
                self.samples[target] = self.samples[target][-self.budget:]
        self.samples = {k: self.samples[k] for k in active_targets}

    def distance(self, features, targets):
        cost_matrix = np.zeros((len(targets), len(features)))
        for i, target in enumerate(targets):
            a, b = np.asarray(self.samples[target]), np.asarray(features)
            a = a / np.linalg.norm(a, axis=1, keepdims=True)
            b = b / np.linalg.norm(b, axis=1, keepdims=True)
            cost_matrix[i, :] = (1. - np.dot(a, b.T)).min(axis=0)
        return cost_matrix


def load_reference():
    """-> namespace(tracker, track, la, detection, kf, opt): the reference's modules imported with the stand-ins the docstring lists.  sys.modules and
    sys.path are left as they were."""
    names = ("opts", "cv2", "deep_sort", "deep_sort.kalman_filter", "deep_sort.iou_matching", "deep_sort.detection", "deep_sort.linear_assignment",
             "deep_sort.track", "deep_sort.tracker", "busca", "busca.network", "busca.tracking", "ref_mot_online_kalman_filter")
    saved, path = {k: sys.modules.pop(k, None) for k in names}, list(sys.path)
    try:
        shims = os.path.join(ROOT, "oracle", "ref_shims")
        if shims not in sys.path:
            sys.path.insert(0, shims)                                # cv2
        opts = types.ModuleType("opts")
        opts.opt = types.SimpleNamespace(MC=True, MC_lambda=MC_LAMBDA, woC=False, EMA=True, EMA_alpha=EMA_ALPHA, ecc={VIDEO: {}})
        pkg, busca = types.ModuleType("deep_sort"), types.ModuleType("busca")
        pkg.__path__, busca.__path__ = [], []
        kf, iou = _kalman_module(), _iou_module()
        pkg.kalman_filter, pkg.iou_matching = kf, iou
        mods = {"opts": opts, "deep_sort": pkg, "deep_sort.kalman_filter": kf, "deep_sort.iou_matching": iou, "busca": busca}
        for name, attr in (("busca.network", "BUSCA"), ("busca.tracking", "center_distance")):
            mods[name] = types.ModuleType(name)
            setattr(mods[name], attr, None)                          # never called: use_busca is off
        sys.modules.update(mods)
        d = os.path.join(REF, "adapters/StrongSORT/deep_sort")
        out = types.SimpleNamespace(kf=kf, opt=opts.opt)
        for name in ("detection", "linear_assignment", "track", "tracker"):
            mod = _load("deep_sort." + name, os.path.join(d, name + ".py"))
            setattr(pkg, name, mod)
            setattr(out, "la" if name == "linear_assignment" else name, mod)
        return out
    finally:
        sys.path[:] = path
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def _warp(theta, scale, dx, dy):
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([[c, -s, dx], [s, c, dy], [0.0, 0.0, 1.0]])


def _unit(v):
    return v / np.linalg.norm(v)


class _Script:
    """Boxes in a world frame seen through a camera: a frame's matrix (where sort_replay.get_matrix keeps it) moves every later detection as
    Track.camera_update moves a track."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.cam = np.eye(3)
        self.frames, self.warps = [], {}

    def camera(self, f, matrix):
        self.warps[f] = matrix
        self.cam = sr.get_matrix(matrix) @ self.cam

    def box(self, x, y, w, h):
        x1, y1, _ = self.cam @ np.array([x, y, 1.0])
        x2, y2, _ = self.cam @ np.array([x + w, y + h, 1.0])
        return [x1, y1, x2 - x1, y2 - y1]

    def feature(self, base, noise=0.01):
        v = _unit(base) + noise * self.rs.normal(size=E) / np.sqrt(E)
        return (v * self.rs.uniform(0.5, 3.0)).astype(np.float32)            # not normalised

    def close(self, dets):
        order = self.rs.permutation(len(dets))                   # the columns are scattered over the frame's list
        det = np.array([d[0] for d in dets], dtype=np.float64).reshape(-1, 5)[order]
        feat = np.array([d[1] for d in dets], dtype=np.float32).reshape(-1, E)[order]
        self.frames.append((det, feat))


def small_script():
    """40 frames, eleven areas 300 px apart, each its own story (the frame numbers are 1-based) -> ([F] of (det [m,5], feat [m,E]), {frame: 3 x 3})."""
    sc = _Script(7)
    rs = sc.rs
    eye = np.eye(E)
    ang = np.arccos(1 - 0.04)                                     # G and H: cosine distance 0.04

    def plane(a, b, phi):
        return np.cos(phi) * eye[a] + np.sin(phi) * eye[b]
    base = {"A": eye[0], "B": eye[1], "C": eye[2], "D": eye[3], "E": plane(3, 4, np.arccos(1 - 0.15)), "G": eye[5], "H": plane(5, 6, ang), "I": eye[7],
            "J": eye[8], "K": eye[9], "N": eye[10], "L": eye[11], "M": eye[12], "P": eye[13], "Q": eye[14], "odd": eye[20]}
    for f in range(1, 41):
        if f in (5, 36):
            sc.camera(f, _warp(0.012 if f == 5 else -0.008, 1.02 if f == 5 else 0.985, 6.0, -4.0))       # rotation and scale
        if f == 15:
            sc.camera(f, _warp(0.0, 1.0, 150.0, 90.0))           # ||I - M|| >= 100: get_matrix answers with the identity
        dets = []

        def put(area, who, dx=0.0, conf=None, feat=None, dy=0.0, still=False):
            jx, jy = rs.uniform(-0.3, 0.3, 2) * (0.0 if still else 1.0)
            x, y = 150.0 + 300 * (area % 5) + 1.0 * f + jx, 150.0 + 350 * (area // 5) + 0.5 * f + jy
            h = 80.0 * (1 + 0.004 * rs.uniform(-1, 1))
            dets.append((sc.box(x + dx, y + dy, 40.0, h) + [rs.uniform(0.5, 0.95) if conf is None else conf],
                         sc.feature(base[who]) if feat is None else feat))
        # area 0: A, always seen; confidence 0 in frame 8 and 0.999 in frame 11
        put(0, "A", conf=0.0 if f == 8 else 0.999 if f == 11 else None)
        # area 1: B, seen once: a tentative track deleted at its first miss
        if f == 1:
            put(1, "B")
        # area 2: C, unseen in frames 7-8 (back at cascade level 2) and from frame 16 on; in frame 19 it has time_since_update 4, takes part in no
        # stage and is deleted, while a detection with its feature sits on it and starts a track that goes on
        if f <= 6 or 9 <= f <= 15 or f >= 19:
            put(2, "C")
        # area 3: D and E 10 px apart with features 0.15 apart.  E is unseen in frame 12; in frame 13 the only detection is E's, and D, one level
        # up in the cascade, takes it
        if f != 13:
            put(3, "D")
        if f != 12:
            put(3, "E", dx=10.0)
        # area 4: G and H 12 px apart with features 0.04 apart; in frame 6 the detection on G looks more like H and the other way round: the
        # appearance alone swaps them, the MC blend does not
        if f == 6:
            put(4, "G", feat=sc.feature(plane(5, 6, 0.19), 0.0))
            put(4, "H", dx=12.0, feat=sc.feature(plane(5, 6, ang - 0.19), 0.0))
        else:
            put(4, "G")
            put(4, "H", dx=12.0)
        # area 5: I; in frame 10 its detection carries a foreign feature: the cascade rejects it, the IoU stage takes it
        put(5, "I", feat=sc.feature(base["odd"]) if f == 10 else None)
        # area 6: J, unseen in frame 20; in frame 21 (time_since_update 2) a foreign feature sits on it: the cascade rejects it, the IoU stage does not
        # see J, the detection starts a track that dies one frame on
        if f != 20:
            put(6, "J", feat=sc.feature(base["odd"]) if f == 21 else None)
        # area 7: K; from frame 24 on its detections sit 60 px aside with the same feature: beyond the chi-square gate and without overlap
        put(7, "K", dx=60.0 if f >= 24 else 0.0)
        # area 8: N, born in frame 9
        if f >= 9:
            put(8, "N")
        # area 9: L and M 12 px apart, born in frame 33; in frame 34 their detections sit so that the row-wise greedy choice is not the optimum
        if f == 33:
            put(9, "L")
            put(9, "M", dx=12.0)
        elif f >= 34:
            put(9, "M", dx=18.0 + (f - 34) * 0.2)
            put(9, "L", dx=7.0 - (f - 34) * 0.2)
        # area 10: P and Q 6 px apart, born in frame 37.  In frame 38 one detection sits 2.5 px from P, the other 22 px to its other side, beyond
        # max_iou_distance for both: the clamp makes the two inadmissible entries equal, and P takes the near one; without the clamp the solver
        # would hand it to Q, because Q's inadmissible entry is the dearer one
        if f == 37:
            put(10, "P", still=True)
            put(10, "Q", dx=6.0, still=True)
        elif f >= 38:
            put(10, "P", dx=1.5, still=True)
            put(10, "Q", dx=-23.0, still=True)
        if f == 30:
            dets = []                                            # frame 30: no detections
        sc.close(dets)
    return sc.frames, sc.warps


def crowded_script():
    """12 frames: 66 walkers on a grid from frame 1, four more from frame 5, two unseen in frames 6-7, a camera matrix in frame 9
    -> ([F] of (det [m,5], feat [m,E]), {frame: 3 x 3})."""
    sc = _Script(13)
    rs = sc.rs
    n = 70
    pos = np.stack([60.0 + 120 * (np.arange(n) % 10), 60.0 + 190 * (np.arange(n) // 10)], 1) + rs.uniform(-6, 6, (n, 2))
    vel, h = rs.uniform(-1.5, 1.5, (n, 2)), rs.uniform(70, 95, n)
    base = np.stack([_unit(v) for v in rs.normal(size=(n, E))])
    for f in range(1, 13):
        if f == 9:
            sc.camera(f, _warp(-0.01, 1.015, -5.0, 3.0))
        dets = []
        for k in range(n):
            if (k >= 66 and f < 5) or (k in (5, 17) and f in (6, 7)):
                continue
            p = pos[k] + vel[k] * f + rs.uniform(-0.8, 0.8, 2)
            hh = h[k] * rs.uniform(0.99, 1.01)
            dets.append((sc.box(p[0], p[1], 0.5 * hh, hh) + [rs.uniform(0.4, 0.97)], sc.feature(base[k], 0.05)))
        sc.close(dets)
    return sc.frames, sc.warps


# ---- recording --------------------------------------------------------------------------------------------------------------
def _kept(gate):
    return np.where(gate > GATE_KEPT, np.inf, gate)


def run_scene(ref, frames, warps, mc, woc, capacity):
    """The reference's tracker over the frames -> the scene's arrays, without the prefix."""
    la, opt, KF = ref.la, ref.opt, ref.kf.KalmanFilter
    opt.MC, opt.woC, opt.ecc = bool(mc), bool(woc), {VIDEO: {str(f): m for f, m in warps.items()}}
    calls, matched = [], []
    orig_mcm, orig_match = la.min_cost_matching, ref.tracker.Tracker._match

    def min_cost_matching(distance_metric, max_distance, tracks, detections, track_indices=None, detection_indices=None):
        kept, at = [], len(KF.gate_log)

        def metric(*a):
            kept.append(distance_metric(*a))                     # clamped in place by the caller
            return kept[0]
        res = orig_mcm(metric, max_distance, tracks, detections, track_indices, detection_indices)
        if kept:
            gates = KF.gate_log[at:]
            calls.append(dict(kind=0 if gates else 1, limit=float(max_distance), rows=np.array(track_indices, dtype=np.int64),
                              cols=np.array(detection_indices, dtype=np.int64), cost=np.array(kept[0], dtype=np.float64),
                              gate=_kept(np.array(gates, dtype=np.float64).reshape(kept[0].shape)) if gates else np.zeros(0),
                              pairs=np.array(res[0], dtype=np.int64).reshape(-1, 2)))
        return res

    def _match(self, detections):
        n_calls = len(calls)
        res = orig_match(self, detections)
        cascade = sum(len(c["pairs"]) for c in calls[n_calls:] if c["kind"] == 0)
        matched.append((np.array(res[0], dtype=np.int64).reshape(-1, 2), cascade, np.array(list(res[1]), dtype=np.int64),
                        np.array(list(res[2]), dtype=np.int64)))
        return res

    la.min_cost_matching, ref.tracker.Tracker._match = min_cost_matching, _match
    try:
        tracker = ref.tracker.Tracker(CosineMetric(MATCH_THRESH, 1), max_iou_distance=MAX_IOU, max_age=MAX_AGE, n_init=N_INIT)
        keys = ("det", "feat", "trk_int", "trk_mean", "trk_cov", "trk_feat", "deleted", "out_id", "out_tlwh", "match", "ut", "ud")
        lists = {k: [] for k in keys}
        cascade_counts, call_begin = [], [0]
        for f, (det, feat) in enumerate(frames, start=1):
            del KF.gate_log[:]
            detections = [ref.detection.Detection(d[:4].copy(), d[4], ft.astype(np.float64)) for d, ft in zip(det, feat)]
            before = [t.track_id for t in tracker.tracks]
            if str(f) in opt.ecc[VIDEO]:                          # opt.ECC
                tracker.camera_update(VIDEO, f)
            tracker.predict()
            tracker.update(detections)
            m, cascade, ut, ud = matched[-1]
            ids = [t.track_id for t in tracker.tracks]
            out = [t for t in tracker.tracks if t.is_confirmed() and t.time_since_update <= 1]
            lists["det"].append(det)
            lists["feat"].append(feat)
            lists["trk_int"].append(np.array([[t.track_id, t.state, t.hits, t.age, t.time_since_update] for t in tracker.tracks],
                                             dtype=np.int64).reshape(-1, 5))
            lists["trk_mean"].append(np.array([t.mean for t in tracker.tracks], dtype=np.float64).reshape(-1, 8))
            lists["trk_cov"].append(np.array([t.covariance for t in tracker.tracks], dtype=np.float64).reshape(-1, 8, 8))
            lists["trk_feat"].append(np.array([t.features[-1] for t in tracker.tracks], dtype=np.float64).reshape(-1, E))
            lists["deleted"].append(np.array([i for i in before if i not in ids], dtype=np.int64))
            lists["out_id"].append(np.array([t.track_id for t in out], dtype=np.int64))
            lists["out_tlwh"].append(np.array([t.to_tlwh() for t in out], dtype=np.float64).reshape(-1, 4))
            lists["match"].append(m)
            lists["ut"].append(ut)
            lists["ud"].append(ud)
            cascade_counts.append(cascade)
            call_begin.append(len(calls))
    finally:
        la.min_cost_matching, ref.tracker.Tracker._match = orig_mcm, orig_match
    F = len(frames)
    out = {"params": np.array([MAX_AGE, N_INIT, MAX_IOU, MATCH_THRESH, EMA_ALPHA, float(mc), MC_LAMBDA, float(woc), F, capacity, E], dtype=np.float64),
           "warp": np.array([warps.get(f, np.zeros((3, 3))) for f in range(1, F + 1)], dtype=np.float64),
           "warp_on": np.array([f in warps for f in range(1, F + 1)], dtype=np.uint8),
           "match_cascade": np.array(cascade_counts, dtype=np.int64), "call_frame_begin": np.array(call_begin, dtype=np.int64),
           "call_kind": np.array([c["kind"] for c in calls], dtype=np.int64), "call_limit": np.array([c["limit"] for c in calls], dtype=np.float64)}
    tails = {"det": (0, 5), "feat": (0, E), "trk_int": (0, 5), "trk_mean": (0, 8), "trk_cov": (0, 8, 8), "trk_feat": (0, E), "out_tlwh": (0, 4), "match": (0, 2)}
    shared = {"feat": "det", "trk_int": "trk", "trk_mean": "trk", "trk_cov": "trk", "trk_feat": "trk", "out_id": "out", "out_tlwh": "out"}
    for key, parts in lists.items():
        dtype = np.float32 if key == "feat" else np.float64 if key in ("det", "trk_mean", "trk_cov", "trk_feat", "out_tlwh") else np.int64
        out[key] = np.concatenate([np.zeros(tails.get(key, (0,)), dtype=dtype)] + parts)
        out["%s_begin" % shared.get(key, key)] = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    for key in ("rows", "cols", "pairs", "cost", "gate"):
        parts = [c[key].reshape(-1, 2) if key == "pairs" else c[key].reshape(-1) for c in calls]
        dtype = np.float64 if key in ("cost", "gate") else np.int64
        out["call_" + key] = np.concatenate([np.zeros((0, 2) if key == "pairs" else (0,), dtype=dtype)] + parts)
        out["call_%s_begin" % key] = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return out


# ---- what the scenes must hold ------------------------------------------------------------------------------------------------
def _margin_of(call):
    return MARGIN_APP if call["kind"] == 0 else MARGIN


def check_scenes(scenes, found=None):
    """The CASES, in the `seen`-set style, and the margins that keep exact comparisons meaningful.  scenes: name -> (params, frames) as
    sort_replay.load_scene gives them: the fixture alone is enough."""
    seen, confs, at = set(), set(), [None, 0]

    def note(case):
        seen.add(case)
        if found is not None:
            found.setdefault(case, "%s, frame %d" % tuple(at))
    for name, (p, frames) in scenes.items():
        slots, free, freed = {}, list(range(p["capacity"])), set()    # the slot bookkeeping of sort_replay.Replay, from the ids alone
        for f, fr in enumerate(frames):
            at[:] = [name, f + 1]
            prev = frames[f - 1] if f else dict(trk_int=np.zeros((0, 5), dtype=np.int64), trk_feat=np.zeros((0, p["E"])), trk_mean=np.zeros((0, 8)))
            ids_before = [int(i) for i in prev["trk_int"][:, 0]]
            before = {int(r[0]): r for r in prev["trk_int"]}
            after = {int(r[0]): r for r in fr["trk_int"]}
            tsu = {i: int(before[i][4]) + 1 for i in ids_before}                   # as _match reads it
            matched = {ids_before[int(a)]: int(b) for a, b in fr["match"]}
            z = sr.xyah_of(fr["det"][:, :4])
            confs.update(float(c) for c in fr["det"][:, 4])
            # ---- margins, and the order of the unmatched detections
            assert fr["ud"].tolist() == sorted(fr["ud"].tolist()), (name, f + 1, "the reference's unmatched detections are not ascending")
            for k, c in enumerate(fr["calls"]):
                cost, m = c["cost"], _margin_of(c)
                ok = cost <= c["limit"]
                assert not (ok & (cost > c["limit"] - m)).any(), (name, f + 1, k, "a cost within the margin of the limit")
                x = np.full(len(c["rows"]), -1, dtype=np.int64)
                for a, b in c["pairs"]:
                    x[list(c["rows"]).index(a)] = list(c["cols"]).index(b)
                assert unique(cost, c["limit"] + 1e-5, x, m), (name, f + 1, k, "the optimum is not unique by the margin")
                if c["kind"] == 0:
                    assert np.abs(c["gate"] - sr.CHI2_4).min() > MARGIN, (name, f + 1, k, "a gating distance within the margin of chi2inv95[4]")
            # ---- cases about the state machine
            born = [i for i in after if i not in before]
            if born and all(after[i][1] == sr.TENTATIVE and after[i][2] == 1 for i in born):
                note("birth_as_tentative")
            for i, r in after.items():
                if i in before and before[i][1] == sr.TENTATIVE and r[1] == sr.CONFIRMED and r[2] == 3 and before[i][2] == 2:
                    note("confirmed_at_third_hit")
            for i in fr["deleted"]:
                i = int(i)
                if before[i][1] == sr.TENTATIVE and before[i][4] == 0:
                    note("tentative_deleted_at_first_miss")
                if before[i][1] == sr.CONFIRMED and tsu[i] == p["max_age"] + 1:
                    note("deleted_only_beyond_max_age")
                    in_a_call = any(ids_before.index(i) in c["rows"] for c in fr["calls"])
                    on_it = [j for j in range(len(z)) if np.abs(z[j, :2] - prev["trk_mean"][ids_before.index(i), :2]).max() < 12
                             and sr.cosine(prev["trk_feat"][ids_before.index(i)][None], fr["feat"][j][None], np.float64)[0, 0] < 0.01]
                    if not in_a_call and on_it and not p["woc"] and all(j in fr["ud"] for j in on_it):
                        note("beyond_max_age_in_no_stage")
            assert not any(before[i][1] == sr.CONFIRMED and tsu[i] <= p["max_age"] for i in map(int, fr["deleted"])), (name, f + 1)
            for i in map(int, fr["deleted"]):
                freed.add(slots[i])
                free.append(slots.pop(i))
            free.sort()
            # ---- cases about matching
            for k, c in enumerate(fr["calls"]):
                level = {tsu[ids_before[int(r)]] - 1 for r in c["rows"]}
                if c["kind"] == 0 and not p["woc"]:
                    assert len(level) == 1
                    if min(level) > 0 and len(c["pairs"]):
                        note("rematched_above_level_0")
                    if min(level) == 0:
                        for a, b in c["pairs"]:                                    # an older confirmed track, left unmatched, whose feature is nearer
                            for i in ids_before:
                                if before[i][1] == sr.CONFIRMED and 2 <= tsu[i] <= p["max_age"] and i not in matched:
                                    feats = prev["trk_feat"][[ids_before.index(i), int(a)]]
                                    d = sr.cosine(feats, fr["feat"][int(b)][None], np.float64)[:, 0]
                                    near = np.abs(z[int(b), :2] - prev["trk_mean"][ids_before.index(i), :2]).max() < 12
                                    if near and d[0] < d[1] - MARGIN_APP and d[0] < p["match_thresh"]:
                                        note("level_priority")
                if c["kind"] == 0:
                    app = sr.cosine(prev["trk_feat"][c["rows"]], fr["feat"][c["cols"]], np.float64)
                    if ((c["gate"] > sr.CHI2_4) & (app < 0.01)).any():
                        note("matching_feature_rejected_by_gate")
                if c["cost"].size and c["cost"].shape[0] > 1:
                    greedy, taken = [], set()
                    for r in range(c["cost"].shape[0]):
                        order = [j for j in np.argsort(c["cost"][r], kind="stable") if j not in taken and c["cost"][r, j] <= c["limit"]]
                        if order:
                            greedy.append((int(c["rows"][r]), int(c["cols"][order[0]])))
                            taken.add(int(order[0]))
                    if sorted(greedy) != sorted((int(a), int(b)) for a, b in c["pairs"]):
                        note("optimum_is_not_greedy")
                        if found is not None:
                            found.setdefault("optimum_is_not_greedy, every frame", []).append("%s %d (%s)" % (name, f + 1, "IoU" if c["kind"] else "cascade"))
                if name == "crowded" and len(c["rows"]) > 16 and len(c["cols"]) > 64:
                    note("crowded_tiles_%d" % c["kind"])
            iou_calls = [c for c in fr["calls"] if c["kind"] == 1]
            for c in iou_calls:
                for a, b in c["pairs"]:
                    i = ids_before[int(a)]
                    if before[i][1] == sr.CONFIRMED and tsu[i] == 1 and any(int(a) in k["rows"] for k in fr["calls"] if k["kind"] == 0):
                        note("rejected_on_appearance_rescued_by_iou")
            for i in ids_before:
                if before[i][1] == sr.CONFIRMED and tsu[i] == 2 and i not in matched and not any(ids_before.index(i) in c["rows"] for c in iou_calls):
                    idx = ids_before.index(i)
                    for j in map(int, fr["ud"]):                                   # a detection on it that nothing took
                        if np.abs(z[j, :2] - prev["trk_mean"][idx, :2]).max() < 12 and any(idx in c["rows"] for c in fr["calls"] if c["kind"] == 0):
                            note("stale_confirmed_not_in_iou_stage")
            # ---- cases about confidences, empty frames and camera frames
            if len(fr["det"]) == 0 and len(ids_before):
                note("frame_without_detections")
            if fr["warp"] is None:
                note("frame_without_matrix")
            elif np.linalg.norm(np.eye(3) - fr["warp"]) >= 100:
                note("camera_matrix_replaced_by_identity")
            elif abs(fr["warp"][0, 1]) > 1e-3 and abs(np.hypot(fr["warp"][0, 0], fr["warp"][1, 0]) - 1) > 1e-3 and len(ids_before):
                note("camera_rotation_and_scale")
            # ---- the slots
            for i in born:
                slots[i] = free.pop(0)
                if slots[i] in freed:
                    note("slot_reused")
    if {0.0, 0.999} <= confs:
        note("confidence_0_and_0999")
    if {"crowded_tiles_0", "crowded_tiles_1"} <= seen:
        note("crowded_tiles")
    seen -= {"crowded_tiles_0", "crowded_tiles_1"}
    a, b = scenes["small"][1], scenes["small_woc"][1]
    for f, (fa, fb) in enumerate(zip(a, b)):
        if fa["match"].tolist() != fb["match"].tolist():                          # until here the two scenes agree in everything discrete, and
            at[:] = ["small", f + 1]                                              # here the cascade had one populated level: woC is not the cause
            only_level_0 = sum(1 for c in fa["calls"] if c["kind"] == 0) == 1
            if only_level_0 and sorted(fa["match"][:, 0].tolist()) == sorted(fb["match"][:, 0].tolist()):
                note("mc_blend_changes_pair")
            break
        assert np.array_equal(fa["trk_int"], fb["trk_int"])
    assert seen == set(CASES), (sorted(set(CASES) - seen), sorted(seen - set(CASES)))


def restatement(made, name, f32):
    """The numpy backend over a recorded scene -> (dict of distances, the Replay), asserting that every decision is the reference's and, in
    float64, the margins of the inadmissible entries on the unclamped planes."""
    worst = {"iou": 0.0, "cost": 0.0, "gate": 0.0}
    p, frames = sr.load_scene(name, made)
    state = {}

    def before_frame(rp, want, f, args):
        if f32:
            return
        probe = sr.NumpyBackend(p["capacity"], p["E"], p)                          # a copy of the state, advanced as frame() is about to
        probe.mean, probe.cov, probe.feat = rp.backend.mean.copy(), rp.backend.cov.copy(), rp.backend.feat.copy()
        probe.advance(args[0], args[7])
        state["planes"] = probe.planes(args[0], args[1], args[2], args[3], args[5]) if len(args[0]) and len(args[3]) else None

    def on_frame(rp, want, f):
        compare_calls(rp.backend.calls, want["calls"], worst, (name, f + 1))
        if not f32 and state["planes"] is not None:
            _, _, p0, p1 = state["planes"]
            for c in want["calls"]:
                raw = (p0 if c["kind"] == 0 else p1)[np.ix_(c["rows"], c["cols"])]
                bad = (raw > c["limit"]) & (raw < c["limit"] + _margin_of(c))
                assert not bad.any(), (name, f + 1, "an inadmissible cost within the margin of its limit")
    bad, err, rp = sr.replay_scene(name, lambda cap, e, q: sr.NumpyBackend(cap, e, q, f32=f32), on_frame=on_frame, before_frame=before_frame, g=made)
    assert bad is None, (name, bad)
    return dict(mean=err["mean"], cov=err["cov"], feat=err["feat"], **worst), rp


def compare_calls(got, want, worst, where):
    """The min_cost_matching calls of a numpy frame against the recorded ones: the same calls on the same rows and columns (as sets: the
    reference's column order follows its solver), the entries into worst["cost"] / ["iou"] / ["gate"]."""
    from tests.test_kalman_filter import err_mean
    assert len(got) == len(want), (where, "calls", len(got), len(want))
    for a, b in zip(got, want):
        assert a.kind == b["kind"] and sorted(a.rows) == sorted(b["rows"].tolist()) and sorted(a.cols) == sorted(b["cols"].tolist()), (where, a.kind)
        r, c = [a.rows.index(int(i)) for i in b["rows"]], [a.cols.index(int(j)) for j in b["cols"]]
        key = "cost" if a.kind == 0 else "iou"
        worst[key] = max(worst[key], float(np.abs(a.cost[np.ix_(r, c)] - b["cost"]).max()))
        if a.kind == 0:
            g, kept = a.gate[np.ix_(r, c)], np.isfinite(b["gate"])
            assert (g[~kept] > GATE_KEPT * (1 - 1e-9)).all(), (where, "a gating distance recorded as beyond GATE_KEPT")
            if kept.any():
                worst["gate"] = max(worst["gate"], err_mean(g[kept], b["gate"][kept]))


def order_is_observable(made, name, bar_mean):
    """At every camera frame with rotation and scale where tracks are held, predict-then-warp lies more than 1000 x the mean bar from
    warp-then-predict (err_mean over the advanced means) -> the number of such frames."""
    from tests.test_kalman_filter import err_mean
    p, frames = sr.load_scene(name, made)
    count = [0]

    def before_frame(rp, want, f, args):
        m = args[7]
        if m is None or not len(args[0]) or abs(m[0, 1]) < 1e-3:
            return
        a, b = sr.NumpyBackend(p["capacity"], p["E"], p), sr.NumpyBackend(p["capacity"], p["E"], p, ("predict_before_camera",))
        for x in (a, b):
            x.mean, x.cov = rp.backend.mean.copy(), rp.backend.cov.copy()
            x.advance(args[0], m)
        assert err_mean(b.mean[args[0]], a.mean[args[0]]) > 1000 * bar_mean, (name, f + 1, "the order of warp and prediction is not observable")
        count[0] += 1
    sr.replay_scene(name, sr.NumpyBackend, before_frame=before_frame, g=made)
    return count[0]


def floors(frames):
    """The rounding bounds the bars are floored at (tests/test_sort_tracker_replay.py derives them): mean, cov, iou, gate, feat, cost; feat32, cost32."""
    u32 = 2.0 ** -24
    return dict(mean=(frames + 1) * U, cov=(frames + 1) * U, iou=16 * U, gate=64 * U, feat=(E + 8) * U, cost=(2 * E + 8) * U, feat32=(E + 8) * u32,
                cost32=(2 * E + 8) * u32)


def make(ref):
    made = {}
    small, small_warps = small_script()
    crowded, crowded_warps = crowded_script()
    for name, frames, warps, mc, woc, capacity in (("small", small, small_warps, True, False, 24), ("small_woc", small, small_warps, False, True, 24),
                                                    ("crowded", crowded, crowded_warps, True, False, 96)):
        arrays = run_scene(ref, frames, warps, mc, woc, capacity)
        made.update({"%s_%s" % (name, k): v for k, v in arrays.items()})
    check_scenes({name: sr.load_scene(name, made) for name in sr.SCENES})
    keys = ("mean", "cov", "iou", "gate", "feat", "cost")
    errs = {k: [] for k in keys + ("feat32", "cost32")}
    factor = 1000.0
    for name in sr.SCENES:
        e64, rp = restatement(made, name, False)
        e32, _ = restatement(made, name, True)
        fl = floors(len(made[name + "_warp_on"]))
        for k in keys:
            errs[k].append(e64[k])
            assert np.isfinite(e64[k]) and MARGIN > 1000 * max(20 * e64[k], fl[k]) or k in ("feat", "cost"), (name, k, e64[k])
        assert MARGIN_APP > 1000 * max(20 * e64["cost"], fl["cost"])
        errs["feat32"].append(e32["feat"])
        errs["cost32"].append(e32["cost"])
        bar32 = max(20 * e32["cost"], fl["cost32"])
        factor = min(factor, float(np.floor(MARGIN_APP / bar32)))
        assert name == "crowded" or any(len(ids) > 1 for ids in rp.slot_history.values())      # a freed slot is taken again
        n_cam = order_is_observable(made, name, max(20 * e64["mean"], fl["mean"]))
        assert n_cam >= 1, name
        print("%-10s %2d frames, %4d detections, %4d track-frames, %3d calls: restatement mean %.3g  cov %.3g  iou %.3g  gate %.3g  feat %.3g  cost %.3g"
              "  | float32 feat %.3g  cost %.3g" % (name, len(made[name + "_warp_on"]), len(made[name + "_det"]), len(made[name + "_trk_int"]),
                                                   len(made[name + "_call_kind"]), *[e64[k] for k in keys], e32["feat"], e32["cost"]))
    assert factor >= 100, factor
    for k, v in errs.items():
        made["restatement_err_" + k] = np.array(v, dtype=np.float64)
    made["appearance_margin_factor"] = np.array([factor], dtype=np.float64)
    return made


def main():
    made = make(load_reference())
    path = os.path.join(OUT, "sort_tracker.npz")
    np.savez_compressed(path, **made)
    print("wrote sort_tracker.npz: %d arrays, %d bytes, appearance margin factor %g" % (len(made), os.path.getsize(path),
                                                                                      made["appearance_margin_factor"][0]))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
