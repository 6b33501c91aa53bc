"""The adapter loop INTEGRATION.md prints for SortStore.frame, made executable: the host bookkeeping of the reference's StrongSORT tracker
(adapters/StrongSORT/deep_sort/tracker.py:94-104, 193-199, track.py:202-278, the loop of deep_sort_app.py:186-206) around ONE `frame` call per frame.
A plain module (no conftest): the tests of tests/test_sort_tracker_replay.py and the generator tests/golden/make_golden_sort_tracker.py import it.

  Replay(backend, ...)   track records in Tracker.tracks order (id counter, state, hits, age, time_since_update, slot), confirmation, mark_missed and
                         deletion, the get_matrix rule (track.py:210-218), the free-slot list in pop order (ascending: a freed slot is the next one
                         taken) and the output rows of deep_sort_app.py:201-206.  begin() / finish() are the two halves of step(), so that several
                         sequences can share one frame_batch call between them
  backends               anything with frame(slots, time_since_update, confirmed, det_tlwh, det_confidence, det_features, free_slots, camera_matrix)
                         -> the fields of SortFrame, states(slots) -> (mean, cov, feat) and boxes(slots) -> tlwh: NumpyBackend (float64 from the
                         restatements the suite already has; `f32=True`: features, EMA and appearance cost in float32 as the device keeps them),
                         DeviceBackend (one SortStore.frame per frame), ComposedBackend (camera_update, predict, match, update, initiate and
                         busca_store_ema_fit on the same kind of store) and run_batched (SortStore.frame_batch over several Replays in lock step)
  DEVIATIONS             planted misreadings of the reference, switched on by name in NumpyBackend / Replay only: what the sensitivity test proves
                         the recorded scenes notice.  The reference never hands iou_cost a row with time_since_update > 1 (tracker.py:239-241 filter
                         the candidates first), so "an IoU stage without the stale rule" cannot be told from the reference on its own and is part of
                         `iou_takes_every_unmatched_confirmed`, which drops the filter and the rule together
  load_scene / compare_frame   tests/golden/sort_tracker.npz cut into frames, and one frame of a replay held against it

Two things in the reference's lists are artefacts of containers and of the solver's choice among inadmissible entries, and are compared as sets or made
unobservable by the scenes: the order of `unmatched_tracks` (a list(set(...))), the order of the IoU stage's confirmed rows (the same) - and the order
of `unmatched_detections`, which min_cost_matching lists as the unassigned columns followed by the columns the solver assigned at the clamped cost
(linear_assignment.py:71-82).  New tracks get their ids in that order; frame() starts them in detection order.  The generator asserts that the
reference's list is ascending in every frame of every scene, so the two agree there."""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sort_tracker.npz")
SCENES = ("small", "small_woc", "crowded")
TENTATIVE, CONFIRMED, DELETED = 1, 2, 3                     # track.py:16-18
INFTY, CHI2_4 = 1e+5, 9.4877                                # linear_assignment.py:12, chi2inv95[4]
DEVIATIONS = ("predict_before_camera", "cascade_ignores_age", "iou_takes_every_unmatched_confirmed", "no_clamp", "no_mc_blend", "nsa_ignores_confidence",
              "ema_starts_at_confirmation", "first_feature_not_normalised", "delete_at_max_age", "confirm_one_hit_late", "tentative_survives_miss",
              "new_tracks_before_survivors", "get_matrix_ignored")
INT_FIELDS = ("track_id", "state", "hits", "age", "time_since_update")

Frame = collections.namedtuple("Frame", "matches unmatched_tracks unmatched_detections new_tracks overflow")
Call = collections.namedtuple("Call", "kind rows cols cost gate")      # one min_cost_matching call: kind 0 cascade / 1 IoU, rows into the frame's track list


class Track:
    """What a deep_sort Track keeps beside its Kalman state and feature, and the slot that holds those."""

    def __init__(self, track_id, slot):
        self.track_id, self.state, self.hits, self.age, self.time_since_update, self.slot = track_id, TENTATIVE, 1, 1, 0, slot

    def ints(self):
        return [int(getattr(self, k)) for k in INT_FIELDS]


def xyah_of(tlwh):
    """Detection.to_xyah (detection.py:43-50) of [m,4]."""
    out = np.array(tlwh, dtype=np.float64).reshape(-1, 4)
    out[:, :2] += out[:, 2:] / 2
    out[:, 2] /= out[:, 3]
    return out


def get_matrix(matrix):
    """Track.get_matrix (track.py:210-218)."""
    eye = np.eye(3)
    return matrix if np.linalg.norm(eye - matrix) < 100 else eye


def cosine(a, b, dt):
    """1 - <a_i, b_j> / (|a_i| |b_j|) with every sum left to right in `dt` (restate_cosine of tests/golden/make_golden_appearance.py without the
    floor at 0, which the nearest-neighbour cosine metric does not have) -> float64 [len a, len b]."""
    a, b = a.astype(dt), b.astype(dt)
    dot = np.zeros((a.shape[0], b.shape[0]), dtype=dt)
    na, nb = np.zeros(a.shape[0], dtype=dt), np.zeros(b.shape[0], dtype=dt)
    for k in range(a.shape[1]):
        dot += a[:, k, None] * b[None, :, k]
        na += a[:, k] * a[:, k]
        nb += b[:, k] * b[:, k]
    return (dt(1) - dot / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :])).astype(np.float64)


def solve(cost, max_distance):
    """min_cost_matching's solve (linear_assignment.py:63-85) on a matrix that is clamped already -> [(row, column)] in row order."""
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(cost)
    return [(int(r), int(c)) for r, c in zip(rows, cols) if not cost[r, c] > max_distance]


# ---- backends -------------------------------------------------------------------------------------------------------------
class NumpyBackend:
    """SortStore.frame's contract in numpy: r_camera, r_predict, r_update_nsa, r_iou_cost of tests/test_sort_store.py, r_initiate, r_gating and
    r_boxes of tests/test_kalman_filter.py, `cosine` above and scipy's linear_sum_assignment.  The Kalman state is float64; the feature rows, the
    EMA and the appearance cost are float64, or float32 with `f32`.  `calls` holds the min_cost_matching calls of the last frame."""

    def __init__(self, capacity, E, p, deviations=(), f32=False):
        self.capacity, self.p, self.dev = capacity, p, set(deviations)
        self.dt = np.float32 if f32 else np.float64
        self.mean, self.cov, self.feat = np.zeros((capacity, 8)), np.zeros((capacity, 8, 8)), np.zeros((capacity, E), dtype=self.dt)
        self.confirmed_slots = set()
        self.calls = []

    def states(self, slots):
        s = np.asarray(slots, dtype=np.int64)
        return self.mean[s].copy(), self.cov[s].copy(), self.feat[s].astype(np.float64)

    def boxes(self, slots):
        from tests.test_kalman_filter import r_boxes
        return r_boxes(self.mean[np.asarray(slots, dtype=np.int64)].reshape(-1, 8), False)

    def advance(self, slots, matrix):
        from tests.test_sort_store import r_camera, r_predict
        for s in slots:
            if matrix is not None and "predict_before_camera" not in self.dev:
                self.mean[s, :4] = r_camera(self.mean[s], matrix)                  # Tracker.camera_update first (deep_sort_app.py:186-189)
            self.mean[s], self.cov[s] = r_predict(self.mean[s], self.cov[s])
            if matrix is not None and "predict_before_camera" in self.dev:
                self.mean[s, :4] = r_camera(self.mean[s], matrix)

    def planes(self, slots, tsu, confirmed, tlwh, feats):
        """-> (appearance [n,m] in float64 as `dt` computed it, gating distances [n,m], plane 0 before the clamp, plane 1 before the clamp)."""
        from tests.test_kalman_filter import r_boxes, r_gating
        from tests.test_sort_store import r_iou_cost
        s = np.asarray(slots, dtype=np.int64)
        z = xyah_of(tlwh)
        app = cosine(self.feat[s], np.asarray(feats).astype(self.dt), self.dt) if len(s) else np.zeros((0, len(z)))
        gate = np.array([r_gating(self.mean[k], self.cov[k], z, False, "maha") for k in s], dtype=np.float64).reshape(len(s), len(z))
        p0 = np.where(gate > CHI2_4, INFTY, app)
        if self.p["mc_lambda"] is not None and "no_mc_blend" not in self.dev:
            p0 = self.p["mc_lambda"] * p0 + (1 - self.p["mc_lambda"]) * gate
        stale = np.asarray(tsu) > 1 if "iou_takes_every_unmatched_confirmed" not in self.dev else None
        p1 = r_iou_cost(r_boxes(self.mean[s].reshape(-1, 8), False), np.asarray(tlwh, dtype=np.float64).reshape(-1, 4), stale)
        return app, gate, p0, p1

    def _min_cost(self, kind, plane, gate, max_distance, rows, cols):
        if not len(rows) or not len(cols):
            return [], list(cols)
        c = plane[np.ix_(rows, cols)].copy()
        if "no_clamp" not in self.dev:
            c[c > max_distance] = max_distance + 1e-5
        self.calls.append(Call(kind, list(rows), list(cols), c, gate[np.ix_(rows, cols)] if kind == 0 else None))
        pairs = solve(c, max_distance)
        taken = {j for _, j in pairs}
        return [(rows[i], cols[j]) for i, j in pairs], [cols[j] for j in range(len(cols)) if j not in taken]

    def match(self, slots, tsu, confirmed, tlwh, feats):
        """Tracker._match (tracker.py:214-252) over the advanced state -> (matches, unmatched rows, unmatched detections)."""
        n, m, p = len(slots), len(tlwh), self.p
        self.calls = []
        app, gate, p0, p1 = self.planes(slots, tsu, confirmed, tlwh, feats)
        conf = [i for i in range(n) if confirmed[i]]
        left, matches = list(range(m)), []
        if p["depth"] is None or "cascade_ignores_age" in self.dev:
            levels = [conf]
        else:
            levels = [[i for i in conf if tsu[i] == 1 + level] for level in range(p["depth"])]
        for k, rows in enumerate(levels):
            if not left and p["depth"] is not None:
                break
            got, left = self._min_cost(0, p0, gate, p["match_thresh"], rows, left)
            matches += got
        matched = {i for i, _ in matches}
        again = [i for i in conf if i not in matched and (tsu[i] == 1 or "iou_takes_every_unmatched_confirmed" in self.dev)]
        got, left = self._min_cost(1, p1, gate, p["max_iou"], [i for i in range(n) if not confirmed[i]] + again, left)
        matches += got
        matched = {i for i, _ in matches}
        return matches, [i for i in range(n) if i not in matched], sorted(left)

    def frame(self, slots, tsu, confirmed, tlwh, conf, feats, free_slots, matrix):
        from tests.test_kalman_filter import r_initiate
        from tests.test_sort_store import r_update_nsa
        dt, p = self.dt, self.p
        self.advance(slots, matrix)
        matches, ut, ud = self.match(slots, tsu, confirmed, tlwh, feats)
        z = xyah_of(tlwh)
        f = np.asarray(feats).astype(dt)
        for i, j in matches:                                                       # Track.update (track.py:232-255)
            s = slots[i]
            self.mean[s], self.cov[s] = r_update_nsa(self.mean[s], self.cov[s], z[j], 0.0 if "nsa_ignores_confidence" in self.dev else float(conf[j]))
            feature = f[j] / np.linalg.norm(f[j]).astype(dt)
            if "ema_starts_at_confirmation" in self.dev and s not in self.confirmed_slots:
                self.feat[s] = feature
            else:
                smooth = dt(p["ema_alpha"]) * self.feat[s] + dt(1 - p["ema_alpha"]) * feature
                self.feat[s] = smooth / np.linalg.norm(smooth).astype(dt)
        free = list(free_slots)
        k = min(len(ud), len(free))
        for j, s in zip(ud[:k], free[:k]):                                         # Tracker._initiate_track, Track.__init__ (track.py:85-98)
            self.mean[s], self.cov[s] = (a[0] for a in r_initiate(z[j:j + 1]))
            self.feat[s] = f[j] if "first_feature_not_normalised" in self.dev else f[j] / np.linalg.norm(f[j]).astype(dt)
            self.confirmed_slots.discard(s)
        return Frame(matches, ut, ud, list(zip(ud[:k], free[:k])), ud[k:])

    def confirmed(self, slot):
        self.confirmed_slots.add(slot)


class DeviceBackend:
    """busca_amd.sort_store.SortStore: one frame() per frame."""

    def __init__(self, capacity, E, p, store=None):
        from busca_amd.sort_store import SortStore
        self.capacity, self.p = capacity, p
        self.store = SortStore(capacity, feature_dim=E) if store is None else store
        self.store._state()

    def kw(self):
        p = self.p
        return dict(max_iou_distance=p["max_iou"], matching_threshold=p["match_thresh"], ema_alpha=p["ema_alpha"], cascade_depth=p["depth"],
                    mc_lambda=p["mc_lambda"])

    def frame(self, slots, tsu, confirmed, tlwh, conf, feats, free_slots, matrix):
        return self.store.frame(slots, tsu, confirmed, tlwh, conf, np.asarray(feats, dtype=np.float32), free_slots=free_slots, camera_matrix=matrix,
                                **self.kw())

    def states(self, slots):
        import torch
        st = self.store
        rows = torch.from_numpy(np.asarray(slots, dtype=np.int64)).to(st.dev)
        return (st.mean.index_select(0, rows).cpu().numpy(), st.cov.index_select(0, rows).cpu().numpy(),
                st.feat.index_select(0, rows).cpu().numpy().astype(np.float64))

    def boxes(self, slots):
        return self.store.boxes(np.asarray(slots, dtype=np.int64), False).cpu().numpy().reshape(-1, 4)

    def confirmed(self, slot):
        pass


class RowMetric:
    """What SortStore.match needs of a metric, over the feature rows of the store: track ids are slots, the gallery is `feat` seen as
    [capacity + 1, 1, E] (as RowMetric of tests/test_sort_frame.py)."""

    def __init__(self, st, threshold):
        from busca_amd import geometry
        self.st, self.ctx, self.matching_threshold = st, geometry.default_context(st.dev.index), threshold

    def distance(self, features, targets, device=False):
        from busca_amd.appearance import appearance_cost
        out = appearance_cost(self.st.feat.view(self.st.capacity + 1, 1, -1), features, "min", slot=np.asarray(targets, dtype=np.int32), ctx=self.ctx)
        return out if device else out.cpu().numpy()


class ComposedBackend(DeviceBackend):
    """The same frame as the calls INTEGRATION.md prints above the frame's: camera_update, predict, match with a metric over the feature rows, update,
    initiate, and busca_store_ema_fit for the rows (as `_composed` of tests/test_sort_frame.py)."""

    def frame(self, slots, tsu, confirmed, tlwh, conf, feats, free_slots, matrix):
        from busca_amd import _store_lib
        from busca_amd._xfer import to_dev
        import torch
        st, p = self.store, self.p
        slots = np.asarray(slots, dtype=np.int64)
        n, m = len(slots), len(tlwh)
        if n:
            if matrix is not None:
                st.camera_update(slots, matrix)
            st.predict(slots)
        if m == 0:
            return Frame([], list(range(n)), [], [], [])
        z, boxes = xyah_of(tlwh), np.asarray(tlwh, dtype=np.float64).reshape(-1, 4)
        d_feats = to_dev(np.ascontiguousarray(feats, dtype=np.float32), st.dev, torch.float32)
        matches, ut, ud = st.match(RowMetric(st, p["match_thresh"]), slots, [int(s) for s in slots], list(tsu), list(confirmed), d_feats, z, boxes,
                                   p["max_iou"], cascade_depth=p["depth"], mc_lambda=p["mc_lambda"])
        if matches:
            assert not st.update(slots[[r for r, _ in matches]], z, [c for _, c in matches], confidence=conf).cpu().numpy().any()
        free = list(free_slots)
        k = min(len(ud), len(free))
        st.initiate(free[:k], z, ud[:k])
        pairs = [(int(slots[r]), 0, int(c)) for r, c in matches] + [(int(s), -1, int(j)) for j, s in zip(ud[:k], free[:k])]
        g = len(pairs)
        if g:
            table = to_dev(np.concatenate([[s for s, _, _ in pairs], [o for _, o, _ in pairs], np.arange(g + 1), [j for _, _, j in pairs]]).astype(np.int32),
                           st.dev, torch.int32)
            _store_lib.check(_store_lib.load().busca_store_ema_fit(st.feat.data_ptr(), st.capacity + 1, 1, st.feature_dim, d_feats.data_ptr(), m,
                                                                   table.data_ptr(), table[g:].data_ptr(), table[2 * g:].data_ptr(),
                                                                   table[3 * g + 1:].data_ptr(), g, g, float(p["ema_alpha"]), *st._where()))
        return Frame([(int(r), int(c)) for r, c in matches], sorted(int(r) for r in ut), [int(j) for j in ud],
                     [(int(j), int(s)) for j, s in zip(ud[:k], free[:k])], [int(j) for j in ud[k:]])


# ---- the driver -----------------------------------------------------------------------------------------------------------
class Replay:
    """The reference's Tracker with the Kalman state and the features behind `backend`.  step(det [m,5] (tlwh, confidence), features [m,E], matrix or
    None) is one camera_update / predict / update of deep_sort_app.py:186-190; afterwards `tracks`, `deleted_now`, `output` (ids), `fr` (what the
    backend returned), `listed` (the tracks its rows index) and `born` describe the frame.  `base`: the first slot of this sequence in a shared store."""

    def __init__(self, backend, p, deviations=(), base=0, capacity=None):
        self.backend, self.p, self.dev, self.base = backend, p, set(deviations), base
        self.capacity = backend.capacity if capacity is None else capacity
        self.tracks, self.next_id = [], 1
        self.slot_history = {}                                  # slot -> the track ids that held it, in order

    def free(self):
        held = {t.slot for t in self.tracks}
        return [self.base + s for s in range(self.capacity) if self.base + s not in held]

    def begin(self, det, feats, matrix):
        det = np.asarray(det, dtype=np.float64).reshape(-1, 5)
        if matrix is not None and "get_matrix_ignored" not in self.dev:
            matrix = get_matrix(np.asarray(matrix, dtype=np.float64))
        for t in self.tracks:                                                      # Track.predict (track.py:207-208)
            t.age += 1
            t.time_since_update += 1
        self.listed = list(self.tracks)
        self.listed_confirmed = [t.state == CONFIRMED for t in self.listed]
        self.offered = self.free()
        return ([t.slot for t in self.listed], [t.time_since_update for t in self.listed], list(self.listed_confirmed), det[:, :4].copy(),
                det[:, 4].copy(), feats, self.offered, matrix)

    def finish(self, fr):
        p = self.p
        assert list(fr.overflow) == [], "the store is full"
        self.fr = fr
        for i, _ in fr.matches:                                                    # Track.update (track.py:252-255)
            t = self.listed[i]
            t.hits += 1
            t.time_since_update = 0
            if t.state == TENTATIVE and t.hits >= p["n_init"] + ("confirm_one_hit_late" in self.dev):
                t.state = CONFIRMED
                self.backend.confirmed(t.slot)
        for i in fr.unmatched_tracks:                                              # Track.mark_missed (track.py:272-278)
            t = self.listed[i]
            if t.state == TENTATIVE:
                if "tentative_survives_miss" not in self.dev:
                    t.state = DELETED
            elif t.time_since_update > p["max_age"] - ("delete_at_max_age" in self.dev):
                t.state = DELETED
        self.born = []
        for k, (j, slot) in enumerate(fr.new_tracks):                              # Tracker._initiate_track (tracker.py:254-259)
            assert slot == self.offered[k] and j == fr.unmatched_detections[k], "new tracks take the free slots in detection order"
            t = Track(self.next_id, int(slot))
            self.next_id += 1
            self.slot_history.setdefault(int(slot), []).append(t.track_id)
            self.born.append(t)
        self.deleted_now = [t.track_id for t in self.tracks if t.state == DELETED]
        alive = [t for t in self.tracks if t.state != DELETED]
        self.tracks = self.born + alive if "new_tracks_before_survivors" in self.dev else alive + self.born
        self.output = [t for t in self.tracks if t.state == CONFIRMED and t.time_since_update <= 1]      # deep_sort_app.py:201-206
        return self.output

    def step(self, det, feats, matrix):
        return self.finish(self.backend.frame(*self.begin(det, feats, matrix)))

    def held(self):
        """-> (ints [T,5]: INT_FIELDS, mean [T,8], cov [T,8,8], feat [T,E]) of every track, in Tracker.tracks order."""
        ints = np.array([t.ints() for t in self.tracks], dtype=np.int64).reshape(-1, 5)
        mean, cov, feat = self.backend.states([t.slot for t in self.tracks])
        return ints, mean.reshape(-1, 8), cov.reshape(-1, 8, 8), feat.reshape(len(ints), -1)

    def output_tlwh(self):
        return self.backend.boxes([t.slot for t in self.output]).reshape(-1, 4)


def run_batched(store, replays, frames_of):
    """SortStore.frame_batch over several Replays in lock step: frames_of[k][f] is the recorded frame f of sequence k, or None where the sequence has
    no frame at that step.  Yields (step, [frame or None per sequence]) after every step; every Replay's backend is a DeviceBackend on `store`."""
    from busca_amd.sort_store import SortFrameProblem
    kw = replays[0].backend.kw()
    for f in range(max(len(x) for x in frames_of)):
        active = [(rp, fr[f]) for rp, fr in zip(replays, frames_of) if f < len(fr) and fr[f] is not None]
        problems = []
        for rp, want in active:
            slots, tsu, conf, tlwh, c, feats, free, matrix = rp.begin(want["det"], want["feat"], want["warp"])
            problems.append(SortFrameProblem(slots, tsu, conf, tlwh, c, np.asarray(feats, dtype=np.float32), free, matrix))
        for (rp, _), fr in zip(active, store.frame_batch(problems, **kw)):
            rp.finish(fr)
        yield f, [fr[f] if f < len(fr) else None for fr in frames_of]


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


def params_of(p):
    """S_params -> the dict the backends and the Replay take."""
    return dict(max_age=int(p[0]), n_init=int(p[1]), max_iou=float(p[2]), match_thresh=float(p[3]), ema_alpha=float(p[4]),
                mc_lambda=float(p[6]) if p[5] else None, depth=None if p[7] else int(p[0]), woc=bool(p[7]), frames=int(p[8]), capacity=int(p[9]),
                E=int(p[10]))


def load_scene(name, g=None):
    """-> (params dict, [frame dict]) of a recorded scene.  A frame: det [m,5], feat [m,E] float32, warp 3 x 3 or None; trk_int [T,5], trk_mean,
    trk_cov, trk_feat; deleted, out_id, out_tlwh; match [k,2] (row of the frame's track list, detection) with match_cascade of them from the cascade,
    ut, ud; calls: the min_cost_matching calls as dict(kind, limit, rows, cols, cost [r,c], gate [r,c] for a cascade call, pairs [k,2])."""
    g = gold() if g is None else g
    p = params_of(g[name + "_params"])
    frames = []
    for f in range(p["frames"]):
        fr = dict(det=_cut(g, name, "det", f), feat=_cut(g, name, "feat", f, "det"), warp=g[name + "_warp"][f] if g[name + "_warp_on"][f] else None,
                  trk_int=_cut(g, name, "trk_int", f, "trk"), trk_mean=_cut(g, name, "trk_mean", f, "trk"), trk_cov=_cut(g, name, "trk_cov", f, "trk"),
                  trk_feat=_cut(g, name, "trk_feat", f, "trk"), deleted=_cut(g, name, "deleted", f), out_id=_cut(g, name, "out_id", f, "out"),
                  out_tlwh=_cut(g, name, "out_tlwh", f, "out"), match=_cut(g, name, "match", f), match_cascade=int(g[name + "_match_cascade"][f]),
                  ut=_cut(g, name, "ut", f), ud=_cut(g, name, "ud", f), calls=[])
        cb = g[name + "_call_frame_begin"]
        for c in range(cb[f], cb[f + 1]):
            rows, cols = _cut(g, name, "call_rows", c), _cut(g, name, "call_cols", c)
            kind = int(g[name + "_call_kind"][c])
            fr["calls"].append(dict(kind=kind, limit=float(g[name + "_call_limit"][c]), rows=rows, cols=cols,
                                    cost=_cut(g, name, "call_cost", c).reshape(len(rows), len(cols)),
                                    gate=_cut(g, name, "call_gate", c).reshape(len(rows), len(cols)) if kind == 0 else None,
                                    pairs=_cut(g, name, "call_pairs", c).reshape(-1, 2)))
        frames.append(fr)
    return p, frames


def canonical_matches(want, confirmed):
    """The recorded matches in the order that does not depend on a set's iteration: the cascade's as they are (level by level, rows ascending), the
    IoU stage's unconfirmed rows ascending, then its confirmed rows ascending (tracker.py:239-241)."""
    m = [(int(a), int(b)) for a, b in want["match"]]
    k = want["match_cascade"]
    return m[:k] + sorted(m[k:], key=lambda x: (bool(confirmed[x[0]]), x[0]))


def compare_frame(rp, want, f, err, bars=None, exact_new=True):
    """One frame of a replay against the recorded one: everything discrete exactly; the states, feature rows and output boxes into err["mean"] /
    ["cov"] / ["feat"] / ["tlwh"] (the running maxima; err_mean / err_cov of tests/test_kalman_filter.py, the largest absolute difference of a
    feature entry) and, where bars (mean, cov, feat) are given, within them.  -> None, or a line naming what diverged."""
    from tests.test_kalman_filter import err_cov, err_mean
    where = "frame %d: " % (f + 1)
    fr = rp.fr
    confirmed = rp.listed_confirmed
    got = [(int(a), int(b)) for a, b in fr.matches]
    if got != canonical_matches(want, confirmed):
        return where + "matches %s, recorded %s" % (got, canonical_matches(want, confirmed))
    if sorted(int(i) for i in fr.unmatched_tracks) != sorted(int(i) for i in want["ut"]):
        return where + "unmatched tracks %s, recorded %s" % (sorted(fr.unmatched_tracks), sorted(want["ut"].tolist()))
    if [int(j) for j in fr.unmatched_detections] != [int(j) for j in want["ud"]]:
        return where + "unmatched detections %s, recorded %s" % (list(fr.unmatched_detections), want["ud"].tolist())
    ints, mean, cov, feat = rp.held()
    if ints.shape != want["trk_int"].shape or not np.array_equal(ints, want["trk_int"]):
        return where + "tracks (%s)\n%s\nrecorded\n%s" % (", ".join(INT_FIELDS), ints, want["trk_int"])
    if sorted(rp.deleted_now) != sorted(int(x) for x in want["deleted"]):
        return where + "deleted ids %s, recorded %s" % (rp.deleted_now, want["deleted"].tolist())
    if [t.track_id for t in rp.output] != [int(x) for x in want["out_id"]]:
        return where + "output ids %s, recorded %s" % ([t.track_id for t in rp.output], want["out_id"].tolist())
    if [t.track_id for t in rp.born] != [int(i) for i in ints[len(ints) - len(rp.born):, 0]] or len(rp.born) != len(want["ud"]):
        return where + "new tracks %s for the recorded unmatched detections %s" % ([t.track_id for t in rp.born], want["ud"].tolist())
    if len(mean):
        em, ec, ef = err_mean(mean, want["trk_mean"]), err_cov(cov, want["trk_cov"]), float(np.abs(feat - want["trk_feat"]).max())
        err["mean"], err["cov"], err["feat"] = max(err["mean"], em), max(err["cov"], ec), max(err["feat"], ef)
        if not np.isfinite([em, ec, ef]).all():
            return where + "a state is not finite"
        if bars is not None and (em > bars[0] or ec > bars[1] or ef > bars[2]):
            return where + "states off by %.3g (mean, bar %.3g) / %.3g (covariance, bar %.3g) / %.3g (feature, bar %.3g)" % (em, bars[0], ec, bars[1], ef, bars[2])
        if exact_new and len(rp.born):
            new = slice(len(ints) - len(rp.born), len(ints))                       # started this frame: KalmanFilter.initiate is exact
            if not (np.array_equal(mean[new], want["trk_mean"][new]) and np.array_equal(cov[new], want["trk_cov"][new])):
                return where + "the Kalman state of a new track differs from the recorded initiation"
    if len(rp.output):
        et = err_mean(rp.output_tlwh(), want["out_tlwh"])
        err["tlwh"] = max(err.get("tlwh", 0.0), et)
        if bars is not None and et > bars[0]:
            return where + "output tlwh off by %.3g (bar %.3g)" % (et, bars[0])
    return None


def replay_scene(name, backend_of, deviations=(), bars=None, on_frame=None, before_frame=None, g=None):
    """The recorded scene through a fresh Replay on backend_of(capacity, E, params) -> (None or the first divergence, err dict, the Replay)."""
    p, frames = load_scene(name, g)
    rp = Replay(backend_of(p["capacity"], p["E"], p), p, deviations=deviations)
    err = {"mean": 0.0, "cov": 0.0, "feat": 0.0}
    for f, want in enumerate(frames):
        try:
            args = rp.begin(want["det"], want["feat"], want["warp"])
            if before_frame is not None:
                before_frame(rp, want, f, args)
            rp.finish(rp.backend.frame(*args))
        except AssertionError as e:                             # a planted deviation may run the store full
            return "frame %d: %s" % (f + 1, e), err, rp
        bad = compare_frame(rp, want, f, err, bars)
        if bad is not None:
            return bad, err, rp
        if on_frame is not None:
            on_frame(rp, want, f)
    return None, err, rp
