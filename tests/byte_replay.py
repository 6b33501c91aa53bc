"""The adapter loop INTEGRATION.md prints for KalmanStore.frame, made executable: the host bookkeeping of BYTETracker.update
(adapters/ByteTrack/yolox/tracker/byte_tracker.py:226-456, 660-698) around ONE `frame` call per frame.  A plain module (no conftest): the tests of
tests/test_byte_tracker_replay.py and the generator tests/golden/make_golden_byte_tracker.py import it.

  Replay(backend, ...)   track records (id counter, state, is_activated, start_frame, frame_id, tracklet_len, slot), the tracked / lost / removed
                         lists in the reference's order (joint_stracks, sub_stracks), the free-slot list (ascending: a freed slot is the next
                         one taken), expiry, and remove_duplicate_stracks on boxes read from the backend
  backends               anything with frame(...) -> ByteFrame fields as KalmanStore.frame, boxes(slots, tlbr), states(slots) and
                         remove_duplicates(a, b): DeviceBackend (busca_amd.kalman_store.KalmanStore), ComposedBackend (the same store driven by
                         three round() calls, update and initiate) and NumpyBackend - float64, built from restatements the suite already has
  DEVIATIONS             planted misreadings of byte_tracker.py, switched on by name in NumpyBackend / Replay only: what the sensitivity test
                         proves the recorded scenes notice
  load_scene / compare   tests/golden/byte_tracker.npz cut into frames, and one frame of a replay held against it

The list algebra is the reference's, literally - including that a Lost track marked Removed at its expiry stays in the lost list, and so in the
pool, for one more frame (byte_tracker.py:439 subtracts the removed list of the frame BEFORE), where round one may still re-activate it."""
import collections
import os
import types

import numpy as np

from oracle import bytetrack as obt
from oracle import geometry as ogeo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "byte_tracker.npz")
SCENES = ("small", "small_mot20", "crowded")
NEW, TRACKED, LOST, REMOVED = 0, 1, 2, 3                     # basetrack.py:5-9
LOW_THRESH, SECOND_THRESH, UNCONFIRMED_THRESH, DUPLICATE_THRESH = 0.1, 0.5, 0.7, 0.15
DEVIATIONS = ("lost_rows_in_round_two", "no_fuse_score", "fuse_score_in_round_two", "det_thresh_is_track_thresh", "unconfirmed_predicted",
              "births_activated_at_once", "round_three_sees_matched", "greedy_rows", "no_duplicate_removal", "duplicate_ties_flipped",
              "ge_at_track_thresh")
INT_FIELDS = ("track_id", "state", "is_activated", "start_frame", "frame_id", "tracklet_len")

Frame = collections.namedtuple("Frame", "first second unconfirmed unmatched_pool unmatched_unconfirmed new_tracks overflow det_class")


class Track:
    """What an STrack keeps beside its Kalman state, and the slot that holds the state."""

    def __init__(self, track_id, frame_id, slot, activated):
        self.track_id, self.state, self.is_activated, self.start_frame, self.frame_id, self.tracklet_len = track_id, TRACKED, activated, frame_id, frame_id, 0
        self.slot = slot
        self.tlbr = None                                       # set before remove_duplicates

    def ints(self):
        return [int(getattr(self, k)) for k in INT_FIELDS]


def detections_of(rows):
    """[m,5] (tlbr, score) -> objects with .tlwh / .tlbr / .score derived as STrack derives them: tlbr_to_tlwh, then tlwh_to_tlbr (:179-189)."""
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 5):
        tlwh = r[:4].copy()
        tlwh[2:] -= tlwh[:2]
        tlbr = tlwh.copy()
        tlbr[2:] += tlbr[:2]
        out.append(types.SimpleNamespace(tlwh=tlwh, tlbr=tlbr, score=r[4]))
    return out


def detections_tlbr(rows):
    return np.array([d.tlbr for d in detections_of(rows)], dtype=np.float64).reshape(-1, 4)


def joint_stracks(a, b):
    seen, res = set(), []
    for t in list(a) + list(b):
        if t.track_id not in seen:
            seen.add(t.track_id)
            res.append(t)
    return res


def sub_stracks(a, b):
    d = collections.OrderedDict()
    for t in a:
        d[t.track_id] = t
    for t in b:
        d.pop(t.track_id, None)
    return list(d.values())


# ---- backends -------------------------------------------------------------------------------------------------------------
class NumpyBackend:
    """KalmanStore's contract in numpy float64: oracle.bytetrack.kalman_multi_predict, r_update / r_initiate / r_boxes of tests/test_kalman_filter.py,
    oracle.geometry.iou_matrix, oracle.bytetrack.duplicate_keep_masks and scipy's padded solve (r_padded of tests/test_linear_assignment.py).
    `costs` holds the three cost matrices of the last frame (None where a round had no row or no column), `rounds` their rows (indices into
    pool / unconfirmed) and columns (detection indices)."""

    def __init__(self, capacity, deviations=()):
        self.capacity = capacity
        self.mean, self.cov = np.zeros((capacity, 8)), np.zeros((capacity, 8, 8))
        self.dev = set(deviations)
        self.costs, self.rounds = [None] * 3, [None] * 3

    def boxes(self, slots, tlbr=True):
        from tests.test_kalman_filter import r_boxes
        return r_boxes(self.mean[np.asarray(slots, dtype=np.int64)].reshape(-1, 8), tlbr)

    def states(self, slots):
        slots = np.asarray(slots, dtype=np.int64)
        return self.mean[slots].copy(), self.cov[slots].copy()

    def remove_duplicates(self, a, b):
        if not a or not b:
            return list(a), list(b)
        cost = 1 - ogeo.iou_matrix(np.stack([t.tlbr for t in a]), np.stack([t.tlbr for t in b]))
        age_a, age_b = [t.frame_id - t.start_frame for t in a], [t.frame_id - t.start_frame for t in b]
        if "duplicate_ties_flipped" in self.dev:                # the tie goes to the first list: b loses where a is at least as old
            age_a = [x + 0.5 for x in age_a]
        ka, kb = obt.duplicate_keep_masks(cost, age_a, age_b, DUPLICATE_THRESH)
        return [t for t, k in zip(a, ka) if k], [t for t, k in zip(b, kb) if k]

    def _solve(self, c, limit):
        from tests.test_linear_assignment import r_padded
        if "greedy_rows" in self.dev:
            x, taken = np.full(c.shape[0], -1, dtype=np.int64), set()
            for i in range(c.shape[0]):
                order = [j for j in np.argsort(c[i], kind="stable") if j not in taken and c[i, j] <= limit]
                if order:
                    x[i] = order[0]
                    taken.add(int(order[0]))
            return x
        return r_padded(c, limit)

    def frame(self, pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh, free_slots=(), mot20=False):
        from tests.test_kalman_filter import r_boxes, r_initiate, r_update
        pool, unc = np.asarray(pool_slots, dtype=np.int64), np.asarray(unconfirmed_slots, dtype=np.int64)
        lost = np.asarray(lost, dtype=bool)
        scores = np.asarray(det_scores, dtype=np.float64)
        m, n_pool = len(scores), len(pool)
        if n_pool:
            self.mean[pool], self.cov[pool] = obt.kalman_multi_predict(self.mean[pool], self.cov[pool], lost)
        if len(unc) and "unconfirmed_predicted" in self.dev:
            self.mean[unc], self.cov[unc] = obt.kalman_multi_predict(self.mean[unc], self.cov[unc])
        first = scores >= track_thresh if "ge_at_track_thresh" in self.dev else scores > track_thresh
        cls = np.full(m, 2, dtype=np.uint8)
        cls[np.logical_and(scores > LOW_THRESH, scores < track_thresh)] = 1
        cls[first] = 0
        fuse = not mot20 and "no_fuse_score" not in self.dev
        det_tlbr = np.array([d.tlbr for d in detections], dtype=np.float64).reshape(-1, 4)
        xyah = np.array([d.tlwh for d in detections], dtype=np.float64).reshape(-1, 4)
        xyah[:, :2] += xyah[:, 2:] / 2
        xyah[:, 2] /= xyah[:, 3]

        def round_(rows, slots, cols, limit, fused):
            """-> row -> detection index or -1, over `rows`."""
            cost = 1 - ogeo.iou_matrix(r_boxes(self.mean[slots].reshape(-1, 8), True), det_tlbr[cols])
            if fused and cost.size:
                cost = 1 - (1 - cost) * scores[cols][None, :].repeat(cost.shape[0], axis=0)
            if cost.size == 0:
                return cost, np.full(len(rows), -1, dtype=np.int64)
            x = self._solve(cost, limit)
            return cost, np.where(x >= 0, np.asarray(cols, dtype=np.int64)[np.maximum(x, 0)], -1)

        cols1 = np.nonzero(cls == 0)[0]
        c1, x1 = round_(range(n_pool), pool, cols1, match_thresh, fuse)
        rows2 = [i for i in range(n_pool) if x1[i] < 0 and (not lost[i] or "lost_rows_in_round_two" in self.dev)]
        cols2 = np.nonzero(cls == 1)[0]
        c2, x2 = round_(rows2, pool[rows2], cols2, SECOND_THRESH, fuse and "fuse_score_in_round_two" in self.dev)
        cols3 = cols1 if "round_three_sees_matched" in self.dev else np.array([j for j in cols1 if j not in set(x1.tolist())], dtype=np.int64)
        c3, x3 = round_(range(len(unc)), unc, cols3, UNCONFIRMED_THRESH, fuse)
        self.costs = [c1, c2, c3]
        self.rounds = [(list(range(n_pool)), cols1.tolist()), (rows2, cols2.tolist()), (list(range(len(unc))), cols3.tolist())]
        first_pairs = [(i, int(x1[i])) for i in range(n_pool) if x1[i] >= 0]
        second_pairs = [(rows2[k], int(x2[k])) for k in range(len(rows2)) if x2[k] >= 0]
        unc_pairs = [(i, int(x3[i])) for i in range(len(unc)) if x3[i] >= 0]
        matched = {i for i, _ in first_pairs + second_pairs}
        left = [i for i in range(n_pool) if i not in matched]
        unmatched_pool = [i for i in left if not lost[i]] + [i for i in left if lost[i]]
        taken = {j for _, j in first_pairs + unc_pairs}
        starts = [int(j) for j in cols1 if j not in taken and not scores[j] < det_thresh]
        for slot, j in [(pool[i], j) for i, j in first_pairs + second_pairs] + [(unc[i], j) for i, j in unc_pairs]:
            self.mean[slot], self.cov[slot] = r_update(self.mean[slot], self.cov[slot], xyah[j])
        free = list(free_slots)
        k = min(len(starts), len(free))
        if k:
            self.mean[free[:k]], self.cov[free[:k]] = r_initiate(xyah[starts[:k]])
        return Frame(first_pairs, second_pairs, unc_pairs, unmatched_pool, [i for i in range(len(unc)) if x3[i] < 0],
                     list(zip(starts[:k], [int(s) for s in free[:k]])), starts[k:], cls)


class DeviceBackend:
    """busca_amd.kalman_store.KalmanStore: one frame() per frame."""

    def __init__(self, capacity):
        from busca_amd.kalman_store import KalmanStore
        self.capacity = capacity
        self.store = KalmanStore(capacity)
        self.store._state()

    def frame(self, pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh, free_slots=(), mot20=False):
        return self.store.frame(pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh,
                                free_slots=free_slots, mot20=mot20)

    def boxes(self, slots, tlbr=True):
        return self.store.boxes(np.asarray(slots, dtype=np.int64), tlbr).cpu().numpy()

    def states(self, slots):
        import torch
        rows = torch.from_numpy(np.asarray(slots, dtype=np.int64)).to(self.store.dev)
        return self.store.mean.index_select(0, rows).cpu().numpy(), self.store.cov.index_select(0, rows).cpu().numpy()

    def remove_duplicates(self, a, b):
        from busca_amd import tracking
        return tracking.remove_duplicate_stracks(a, b)


class ComposedBackend(DeviceBackend):
    """The same frame as three KalmanStore.round calls with the lists compacted on the host between them as byte_tracker.py:312-425 compacts them,
    then KalmanStore.update and KalmanStore.initiate: the route INTEGRATION.md prints above the frame's."""

    def frame(self, pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh, free_slots=(), mot20=False):
        from busca_amd.kalman import _measurements
        st = self.store
        pool, unc = np.asarray(pool_slots, dtype=np.int64), np.asarray(unconfirmed_slots, dtype=np.int64)
        lost, scores, free = np.asarray(lost, dtype=bool), np.asarray(det_scores, dtype=np.float64), list(free_slots)
        hi = np.nonzero(scores > track_thresh)[0]
        lo = np.nonzero(np.logical_and(scores > LOW_THRESH, scores < track_thresh))[0]
        cls = np.full(len(scores), 2, dtype=np.uint8)
        cls[lo], cls[hi] = 1, 0
        m1, ut, ud = st.round(pool, [detections[j] for j in hi], match_thresh, det_scores=None if mot20 else scores[hi], not_tracked=lost)
        first = [(int(r), int(hi[c])) for r, c in m1]
        r_tracked, r_lost = [int(i) for i in ut if not lost[i]], [int(i) for i in ut if lost[i]]
        m2, ut2, _ = st.round(pool[r_tracked], [detections[j] for j in lo], SECOND_THRESH, predict=False)
        second = [(r_tracked[r], int(lo[c])) for r, c in m2]
        left = [int(hi[c]) for c in ud]
        m3, uu, ud3 = st.round(unc, [detections[j] for j in left], UNCONFIRMED_THRESH, det_scores=None if mot20 else scores[left], predict=False)
        unconfirmed = [(int(r), left[c]) for r, c in m3]
        starts = [left[c] for c in ud3 if not scores[left[c]] < det_thresh]
        pairs = [(pool[r], j) for r, j in first + second] + [(unc[r], j) for r, j in unconfirmed]
        xyah = _measurements(detections) if len(detections) else np.zeros((0, 4))
        if pairs:
            assert not st.update([s for s, _ in pairs], xyah, [j for _, j in pairs]).cpu().numpy().any()
        k = min(len(starts), len(free))
        if k:
            st.initiate(free[:k], xyah, starts[:k])
        return Frame(first, second, unconfirmed, [r_tracked[i] for i in ut2] + r_lost, [int(r) for r in uu],
                     [(int(j), int(s)) for j, s in zip(starts[:k], free[:k])], [int(j) for j in starts[k:]], cls)


# ---- the driver -----------------------------------------------------------------------------------------------------------
class Replay:
    """BYTETracker (byte_tracker.py:195-456) with the Kalman side behind `backend`.  step(rows [m,5]) is one update(); afterwards `tracked`, `lost`,
    `removed_now`, `output`, `fr` (what the backend returned), `pool` / `unconfirmed` (the lists its rows index), `pairs` (the three rounds as
    (track id, detection index)), `dup_a` / `dup_b` (the ids remove_duplicate_stracks took from the tracked / lost list) describe the frame."""

    def __init__(self, backend, track_thresh, track_buffer, match_thresh, mot20, frame_rate=30, deviations=(), before_frame=None):
        self.backend, self.dev = backend, set(deviations)
        self.track_thresh, self.match_thresh, self.mot20 = track_thresh, match_thresh, bool(mot20)
        self.det_thresh = track_thresh if "det_thresh_is_track_thresh" in self.dev else track_thresh + 0.1      # :210
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        self.tracked, self.lost, self.removed = [], [], []
        self.free = list(range(backend.capacity))
        self.frame_id = self.count = 0
        self.slot_history = {}                                  # slot -> the track ids that held it, in order
        self.before_frame = before_frame

    def _matched(self, t, activated, refind):
        """The bookkeeping of track.update / re_activate (:77-121): the state is updated already."""
        if t.state == TRACKED:
            t.tracklet_len += 1
            activated.append(t)
        else:
            t.tracklet_len = 0
            refind.append(t)
        t.frame_id, t.state, t.is_activated = self.frame_id, TRACKED, True

    def step(self, rows):
        self.frame_id += 1
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
        dets, scores = detections_of(rows), rows[:, 4].copy()
        activated, refind, lost_now, removed_now = [], [], [], []
        unconfirmed = [t for t in self.tracked if not t.is_activated]                       # :304-310
        pool = joint_stracks([t for t in self.tracked if t.is_activated], self.lost)        # :313
        flags = [t.state != TRACKED for t in pool]
        if self.before_frame is not None:
            self.before_frame(self, pool, flags, unconfirmed, dets, scores)
        fr = self.backend.frame([t.slot for t in pool], flags, [t.slot for t in unconfirmed], dets, scores, self.track_thresh, self.match_thresh,
                                self.det_thresh, free_slots=list(self.free), mot20=self.mot20)
        assert list(fr.overflow) == [], "the store is full"
        self.pairs = [[(pool[i].track_id, int(j)) for i, j in fr.first], [(pool[i].track_id, int(j)) for i, j in fr.second],
                      [(unconfirmed[i].track_id, int(j)) for i, j in fr.unconfirmed]]
        self.unassigned = [pool[i].track_id for i in fr.unmatched_pool]                   # unassigned_stracks (:364), what step 3b works on
        for i, j in list(fr.first) + list(fr.second):                                       # :321-362
            self._matched(pool[i], activated, refind)
        for i in fr.unmatched_pool:                                                         # :399-403
            if pool[i].state != LOST:
                pool[i].state = LOST
                lost_now.append(pool[i])
        for i, j in fr.unconfirmed:                                                         # :411-413
            self._matched(unconfirmed[i], activated, refind)
        for i in fr.unmatched_unconfirmed:                                                  # :414-417
            unconfirmed[i].state = REMOVED
            removed_now.append(unconfirmed[i])
        for j, slot in fr.new_tracks:                                                       # :420-425, STrack.activate (:63-75)
            assert slot == self.free[0], "new tracks take the free slots in detection order"
            self.free.pop(0)
            self.count += 1
            t = Track(self.count, self.frame_id, int(slot), self.frame_id == 1 or "births_activated_at_once" in self.dev)
            self.slot_history.setdefault(int(slot), []).append(t.track_id)
            activated.append(t)
        for t in self.lost:                                                                 # :427-430
            if self.frame_id - t.frame_id > self.max_time_lost:
                t.state = REMOVED
                removed_now.append(t)
        self.tracked = [t for t in self.tracked if t.state == TRACKED]                     # :434-443
        self.tracked = joint_stracks(joint_stracks(self.tracked, activated), refind)
        self.lost = sub_stracks(self.lost, self.tracked)
        self.lost.extend(lost_now)
        self.lost = sub_stracks(self.lost, self.removed)
        self.removed.extend(removed_now)
        self.removed = [t for t in self.removed if self.frame_id - t.frame_id < 10 * self.max_time_lost]
        ids_a, ids_b = [t.track_id for t in self.tracked], [t.track_id for t in self.lost]
        if "no_duplicate_removal" not in self.dev:                                         # :444
            both = self.tracked + self.lost
            for t, box in zip(both, self.backend.boxes([t.slot for t in both], True) if both else []):
                t.tlbr = np.asarray(box, dtype=np.float64)
            self.tracked, self.lost = self.backend.remove_duplicates(self.tracked, self.lost)
        self.dup_a = [i for i in ids_a if i not in {t.track_id for t in self.tracked}]
        self.dup_b = [i for i in ids_b if i not in {t.track_id for t in self.lost}]
        held = {t.slot for t in self.tracked + self.lost}                                  # a track in neither list gives its slot back
        self.free = [s for s in range(self.backend.capacity) if s not in held]
        self.removed_now = [t.track_id for t in removed_now]
        self.output = [t for t in self.tracked if t.is_activated]                          # :446
        self.fr, self.pool, self.unconfirmed = fr, pool, unconfirmed
        return self.output

    def held(self):
        """-> (ints [T,7]: INT_FIELDS and the list (0 tracked, 1 lost), mean [T,8], cov [T,8,8]) of every track in the two lists, in their order."""
        both = self.tracked + self.lost
        ints = np.array([t.ints() + [int(k >= len(self.tracked))] for k, t in enumerate(both)], dtype=np.int64).reshape(-1, 7)
        mean, cov = self.backend.states([t.slot for t in both])
        return ints, mean.reshape(-1, 8), cov.reshape(-1, 8, 8)

    def output_tlwh(self):
        return self.backend.boxes([t.slot for t in self.output], False).reshape(-1, 4)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
_CACHE = {}


def gold():
    if "g" not in _CACHE:
        with np.load(GOLD) as f:
            _CACHE["g"] = {k: f[k] for k in f.files}
    return _CACHE["g"]


def _cut(g, name, key, f, begin=None):
    b = g["%s_%s_begin" % (name, begin or key)]
    return g["%s_%s" % (name, key)][b[f]:b[f + 1]]


def load_scene(name, g=None):
    """-> (params dict, [frame dict]) of a recorded scene.  A frame: det [m,5]; trk_int [T,7], trk_mean, trk_cov; removed, out_id, out_tlwh, dup_a,
    dup_b, unassigned, pool_tlbr, dup_cost, dup_age_a, dup_age_b; rounds: three of dict(rows track ids, cols detection indices, pairs [k,2] (track id, detection index), limit, cost [r,c] or
    None where the matrices of that frame are not kept)."""
    g = gold() if g is None else g
    p = g[name + "_params"]
    params = dict(track_thresh=float(p[0]), track_buffer=int(p[1]), match_thresh=float(p[2]), mot20=bool(p[3]), frames=int(p[4]), capacity=int(p[5]))
    frames = []
    for f in range(params["frames"]):
        fr = dict(det=_cut(g, name, "det", f), trk_int=_cut(g, name, "trk_int", f, "trk"), trk_mean=_cut(g, name, "trk_mean", f, "trk"),
                  trk_cov=_cut(g, name, "trk_cov", f, "trk"), removed=_cut(g, name, "removed", f), out_id=_cut(g, name, "out_id", f, "out"),
                  out_tlwh=_cut(g, name, "out_tlwh", f, "out"), dup_a=_cut(g, name, "dup_a", f), dup_b=_cut(g, name, "dup_b", f),
                  unassigned=_cut(g, name, "unassigned", f), pool_tlbr=_cut(g, name, "pool_tlbr", f), dup_age_a=_cut(g, name, "dup_age_a", f),
                  dup_age_b=_cut(g, name, "dup_age_b", f), rounds=[])
        fr["dup_cost"] = _cut(g, name, "dup_cost", f).reshape(len(fr["dup_age_a"]), len(fr["dup_age_b"]))
        for r in range(3):
            k = 3 * f + r
            rows, cols = _cut(g, name, "rnd_rows", k), _cut(g, name, "rnd_cols", k)
            cost = _cut(g, name, "rnd_cost", k)
            kept = bool(g[name + "_rnd_kept"][k])
            fr["rounds"].append(dict(rows=rows, cols=cols, pairs=_cut(g, name, "rnd_pairs", k).reshape(-1, 2), limit=float(g[name + "_rnd_limit"][k]),
                                     cost=cost.reshape(len(rows), len(cols)) if kept else None))
        frames.append(fr)
    return params, frames


def compare_frame(rp, want, f, err, bar_mean=None, bar_cov=None, exact_new=True):
    """One frame of a replay against the recorded one: everything discrete exactly; the states into err["mean"] / err["cov"] (the running maxima,
    by err_mean / err_cov of tests/test_kalman_filter.py) and, where bars are given, within them.  -> None, or a line naming what diverged."""
    from tests.test_kalman_filter import err_cov, err_mean
    where = "frame %d: " % (f + 1)
    for r, name in enumerate(("first", "second", "unconfirmed")):
        got, ref = sorted(rp.pairs[r]), sorted((int(a), int(b)) for a, b in want["rounds"][r]["pairs"])
        if got != ref:
            return where + "%s-round pairs %s, recorded %s" % (name, got, ref)
    if rp.unassigned != [int(x) for x in want["unassigned"]]:
        return where + "unmatched_pool %s, recorded unassigned_stracks %s" % (rp.unassigned, want["unassigned"].tolist())
    ints, mean, cov = rp.held()
    if ints.shape != want["trk_int"].shape or not np.array_equal(ints, want["trk_int"]):
        return where + "tracked / lost lists (%s, list)\n%s\nrecorded\n%s" % (", ".join(INT_FIELDS), ints, want["trk_int"])
    if sorted(rp.removed_now) != sorted(int(x) for x in want["removed"]):
        return where + "removed ids %s, recorded %s" % (rp.removed_now, want["removed"].tolist())
    if [t.track_id for t in rp.output] != [int(x) for x in want["out_id"]]:
        return where + "output ids %s, recorded %s" % ([t.track_id for t in rp.output], want["out_id"].tolist())
    if rp.dup_a != [int(x) for x in want["dup_a"]] or rp.dup_b != [int(x) for x in want["dup_b"]]:
        return where + "duplicates removed %s / %s, recorded %s / %s" % (rp.dup_a, rp.dup_b, want["dup_a"].tolist(), want["dup_b"].tolist())
    if len(mean):
        em, ec = err_mean(mean, want["trk_mean"]), err_cov(cov, want["trk_cov"])
        err["mean"], err["cov"] = max(err["mean"], em), max(err["cov"], ec)
        if not (np.isfinite(em) and np.isfinite(ec)):
            return where + "a state is not finite"
        if bar_mean is not None and (em > bar_mean or ec > bar_cov):
            return where + "states off by %.3g (mean, bar %.3g) / %.3g (covariance, bar %.3g)" % (em, bar_mean, ec, bar_cov)
        if exact_new:
            new = np.nonzero(np.logical_and(ints[:, 3] == f + 1, ints[:, 4] == f + 1))[0]      # started this frame: initiation is exact
            if not (np.array_equal(mean[new], want["trk_mean"][new]) and np.array_equal(cov[new], want["trk_cov"][new])):
                return where + "the state of a new track differs from the recorded initiation"
    if len(rp.output):
        et = err_mean(rp.output_tlwh(), want["out_tlwh"])
        err["tlwh"] = max(err.get("tlwh", 0.0), et)
        if bar_mean is not None and et > bar_mean:
            return where + "output tlwh off by %.3g (bar %.3g)" % (et, bar_mean)
    return None


def replay_scene(name, backend_of, deviations=(), bars=None, on_frame=None, before_frame=None, g=None):
    """The recorded scene through a fresh Replay on backend_of(capacity) -> (None or the first divergence, err dict, the Replay)."""
    params, frames = load_scene(name, g)
    rp = Replay(backend_of(params["capacity"]), params["track_thresh"], params["track_buffer"], params["match_thresh"], params["mot20"],
                deviations=deviations, before_frame=before_frame)
    err = {"mean": 0.0, "cov": 0.0}
    for f, want in enumerate(frames):
        try:
            rp.step(want["det"])
        except AssertionError as e:                             # a planted deviation may run the store full
            return "frame %d: %s" % (f + 1, e), err, rp
        bad = compare_frame(rp, want, f, err, *(bars or (None, None)))
        if bad is not None:
            return bad, err, rp
        if on_frame is not None:
            on_frame(rp, want, f)
    return None, err, rp
