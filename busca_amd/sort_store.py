"""StrongSORT's Kalman state resident on the device: the means and covariances of all tracks stay in two device tensors over `capacity` slots, and
every step names the slots it serves.  Fronts include/busca_sort.h (libbusca_sort.so, bound by _sort_lib), for the two steps whose arithmetic is
ByteTrack's (initiate, the box conversions) include/busca_track.h through a KalmanStore over the same tensors, and for a whole frame as one chain
include/busca_sframe.h (libbusca_sframe.so, bound by _sframe_lib), and for the frames of many sequences on one store include/busca_msframe.h
(libbusca_msframe.so, bound by _msframe_lib).  Restates Track.predict / update /
camera_update (adapters/StrongSORT/deep_sort/track.py:202-250), gate_cost_matrix with min_cost_matching's clamp (linear_assignment.py:61,164-210)
and the two stages of Tracker._match (tracker.py:211-248) without the objects.  deep_sort/kalman_filter.py and iou_matching.py are not in the
reference tree: predict, the confidence-scaled update and iou_cost are restated from upstream StrongSORT (DESIGN K-SORT)."""
import collections

import numpy as np
import torch

from . import _lib, _msframe_lib, _sframe_lib, _sort_lib, geometry
from ._xfer import h2d_async, small_to_dev, stream_of, to_dev
from .appearance import INFTY_COST
from .assignment import _assign_dev, _assign_stages_dev, _solved
from .ghost_motion import _slots_checked
from .kalman import _measurements, _raise_flagged
from .kalman_store import KalmanStore, _small


# what SortStore.frame returns: the matches as (row, detection) in the order Tracker._match lists them (the cascade level by level, then the IoU
# stage, its unconfirmed tracks first; rows index `slots`), the rows and the detections nothing matched, the tracks started as (detection, slot),
# and the detections that would have started one but found the store full
SortFrame = collections.namedtuple("SortFrame", "matches unmatched_tracks unmatched_detections new_tracks overflow")
# one frame of SortStore.frame_batch: the arguments of frame() that belong to a sequence - its tracks, its detections, its free slots, its camera matrix
SortFrameProblem = collections.namedtuple("SortFrameProblem", "slots time_since_update confirmed det_tlwh det_confidence det_features free_slots camera_matrix",
                                          defaults=((), None))
APPEAR_E_MIN, APPEAR_E_MAX = 16, 2048      # BUSCA_APPEAR_E_MIN / _MAX: the feature widths busca_appearance_cost takes (multiples of 16)

assert (_sframe_lib.MC, _sframe_lib.CLAMP) == (_sort_lib.MC, _sort_lib.CLAMP) == (_msframe_lib.MC, _msframe_lib.CLAMP)
assert (_msframe_lib.E_MIN, _msframe_lib.E_MAX, _msframe_lib.MAX_DETS) == (APPEAR_E_MIN, APPEAR_E_MAX, _sframe_lib.MAX_DETS)


def _frame_boxes(det_tlwh):
    """The detections of frame() on the host -> (tlwh [m,4], xyah [m,4]): a host [m,4] array of tlwh boxes or objects with `.tlwh`; the measurements
    follow by the operations of Detection.to_xyah (deep_sort/detection.py: ret[:2] += ret[2:] / 2, ret[2] /= ret[3])."""
    if torch.is_tensor(det_tlwh):
        raise ValueError("SortStore.frame takes a host [m,4] array of tlwh boxes or detection objects with .tlwh")
    if not isinstance(det_tlwh, np.ndarray) and len(det_tlwh) and hasattr(det_tlwh[0], "tlwh"):
        det_tlwh = [d.tlwh for d in det_tlwh]
    tlwh = np.array(det_tlwh, dtype=np.float64).reshape(-1, 4)
    xyah = tlwh.copy()
    xyah[:, :2] += xyah[:, 2:] / 2
    xyah[:, 2] /= xyah[:, 3]
    return tlwh, xyah


def _xyah(detections):
    """The measurements of a call: a device tensor or an [m,4] array of (x, y, a, h) as it is, `.to_xyah()` of deep_sort Detections, tlwh_to_xyah(.tlwh)
    of other objects."""
    if torch.is_tensor(detections) or isinstance(detections, np.ndarray):
        return detections
    if len(detections) and hasattr(detections[0], "to_xyah"):
        return np.asarray([d.to_xyah() for d in detections], dtype=np.float64).reshape(-1, 4)
    return _measurements(detections)


def _match_stage_tables(time_since_update, confirmed, cascade_depth):
    """Tracker._match (adapters/StrongSORT/deep_sort/tracker.py:226-248) as the row tables of a staged assignment -> (first, again), int32 [n].
    Stages 0 .. depth - 1 are the levels of matching_cascade (level l holds the confirmed tracks with time_since_update == 1 + l), stage `depth` is
    the IoU stage: the unconfirmed tracks, and again the confirmed tracks with time_since_update == 1 that the cascade left unmatched.  A confirmed
    track older than the cascade is deep takes part in nothing (-1).  cascade_depth=None (opt.woC): every confirmed track in stage 0, IoU stage 1."""
    tsu = np.asarray(time_since_update, dtype=np.int64).reshape(-1)
    conf = np.asarray(confirmed, dtype=bool).reshape(-1)
    if len(tsu) != len(conf):
        raise ValueError("_match_stage_tables: %d time_since_update entries, %d confirmed flags" % (len(tsu), len(conf)))
    depth = 1 if cascade_depth is None else int(cascade_depth)
    if not 0 <= depth < _lib.ASSIGN_STAGES_MAX:
        raise ValueError("a cascade of depth %d: the staged solver takes %d stages, the IoU stage among them" % (depth, _lib.ASSIGN_STAGES_MAX))
    level = np.zeros(len(tsu), dtype=np.int64) if cascade_depth is None else tsu - 1
    first = np.where(conf, np.where((level >= 0) & (level < depth), level, -1), depth)
    again = np.where(conf & (tsu == 1), depth, -1)
    return first.astype(np.int32), again.astype(np.int32)


def _match_order(stage, first, depth):
    """The rows of a frame in the order Tracker._match lists their matches (tracker.py:233-250): by stage - the cascade level by level, then the IoU
    stage -, inside the IoU stage the unconfirmed tracks (first == depth) before the confirmed ones that entered it again (iou_track_candidates,
    :239-241), and by row inside each of these."""
    n = len(stage)
    return np.lexsort((np.arange(n), np.asarray(first[:n]) != depth, stage))


class SortStore:
    """The Kalman state of up to `capacity` StrongSORT tracks on the device (busca_sort_*, busca_track_kalman_initiate / _boxes):
      initiate(slots, dets, det_index)       KalmanFilter.initiate: Track.__init__'s state of a new track - also how a slot is reused
      predict(slots)                         Track.predict in place
      update(slots, dets, det_index, confidence)   the NSA Kalman update of Track.update in place -> device status words
      camera_update(slots, matrix)           Track.camera_update with one 3 x 3 warp
      boxes(slots, tlbr)                     Track.to_tlbr / to_tlwh
      gate_cost(slots, cost, det_xyah, ...)  gate_cost_matrix, the MC blend and the clamp on a cost matrix, one launch -> (device [n,m], status [n])
      iou_cost(slots, det_tlwh, stale, ...)  iou_matching.iou_cost and the clamp, one launch -> device [n,m]
      appearance_round(metric, slots, ...)   the first stage of Tracker._match: appearance.appearance_round on resident state
      iou_round(slots, det_tlwh, ...)        its IoU stage: iou_cost, the clamp and the linear assignment; one copy, of match vectors
      match(metric, slots, ...)              the whole of Tracker._match - cascade, IoU stage, merge - as one staged assignment; ONE copy whatever the depth
      frame(slots, ...)                      a whole frame on the state and the feature rows: camera update, predict, _match, update and initiation as
                                             ONE chain -> SortFrame; needs `feature_dim`
      frame_batch(problems, ...)             the frames of one time step of many sequences that share the store: a list of SortFrameProblem, the same
                                             chain once for all of them -> [SortFrame]
      features / load_features(slots, ...)   the feature rows of the listed slots, out and in
      load / store(slots, tracks)            states from / to objects with `.mean` / `.covariance`, for a tracker that migrates call by call
    `mean` [capacity + 1, 8] and `cov` [capacity + 1, 8, 8] are float64 device tensors in the layout of KalmanStore, allocated at the first call that
    needs them; the slot behind the last is a spare no kernel writes.  Slot lists given as host lists or arrays are checked on the host - the entries
    >= 0 distinct and below `capacity`, ValueError otherwise; a negative entry is skipped.  A slot list given as a device tensor is read in place: it
    is the caller's to keep distinct, and entries outside the capacity are skipped by the kernels and touch no memory.  Detections: an [m,4] host
    array or device tensor of (x, y, a, h) measurements, or objects with `.to_xyah()` or `.tlwh`.  Every call is asynchronous on torch's current
    stream of the device, except that the rounds, match(), frame() and store() wait for their one copy.
    With `feature_dim` = E the store also keeps `feat`, float32 [capacity + 1, E]: one row per slot, the track's features[-1] of
    deep_sort/track.py (the EMA-smoothed, normalised appearance feature), allocated with the state and written by frame()."""

    def __init__(self, capacity, device=None, feature_dim=None):
        if int(capacity) < 0:
            raise ValueError("SortStore(capacity=%d)" % int(capacity))
        if feature_dim is not None and int(feature_dim) < 1:
            raise ValueError("SortStore(feature_dim=%d)" % int(feature_dim))
        self._k = KalmanStore(capacity, device)
        self.capacity, self.dev = self._k.capacity, self._k.dev
        self.feature_dim = None if feature_dim is None else int(feature_dim)
        self.feat = None
        self._lib = None

    # ---- plumbing
    mean = property(lambda self: self._k.mean, lambda self, t: setattr(self._k, "mean", t))
    cov = property(lambda self: self._k.cov, lambda self, t: setattr(self._k, "cov", t))

    def _state(self):
        self._k._state()
        if self.feature_dim is not None and self.feat is None:
            self.feat = torch.zeros(self.capacity + 1, self.feature_dim, dtype=torch.float32, device=self.dev)
        if self._lib is None:
            self._lib = _sort_lib.load()
        return self._lib

    def _slots(self, slots, what):
        """-> (device i32 [n], n); a host list is checked first, before anything is allocated."""
        slot, n = _slots_checked(slots, self.capacity, "SortStore." + what)
        return _small(slot, self.dev, torch.int32), n

    def _where(self):
        return self.dev.index, stream_of(self.dev)

    def _f64(self, x, cols, what):
        """A host array (pinned staging) or device tensor as a contiguous device float64 [k, cols] (cols = 0: [k])."""
        if not torch.is_tensor(x):
            x = np.asarray(x, dtype=np.float64)
        if cols and (x.ndim != 2 or x.shape[1] != cols) and x.size:
            raise ValueError("SortStore.%s takes [m,%d] values, not %s" % (what, cols, tuple(x.shape)))
        t = _small(x, self.dev, torch.float64)
        return t.view(-1, cols) if cols else t

    # ---- the filter
    def initiate(self, slots, detections, det_index=None):
        """KalmanFilter.initiate of detection det_index[i] (None: i) into slot slots[i]: a new track, or a new tenant of an abandoned slot."""
        slot, _ = _slots_checked(slots, self.capacity, "SortStore.initiate")
        self._k.initiate(slot, _xyah(detections), det_index)

    def predict(self, slots):
        """Track.predict of the listed slots in place."""
        slot, n = self._slots(slots, "predict")
        if n == 0:
            return
        lib = self._state()
        _sort_lib.check(lib.busca_sort_predict(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, *self._where()))

    def update(self, slots, detections, det_index=None, confidence=None):
        """KalmanFilter.update(mean, covariance, xyah, confidence) of slot slots[i] with detection j = det_index[i] (None: i), in place -> device
        int32 [n] status words: 1 where the reference raises LinAlgError (that slot keeps its state), which is the caller's to read or not.
        `confidence`: None (0 for all), one number, or one per DETECTION ([m] host array or device tensor) - detection.confidence."""
        slot, n = self._slots(slots, "update")
        z = self._f64(_xyah(detections), 4, "update")
        m = z.shape[0]
        idx = None
        if det_index is not None:
            idx = _small(det_index if torch.is_tensor(det_index) else np.asarray(det_index, dtype=np.int32), self.dev, torch.int32)
            if idx.numel() != n:
                raise ValueError("SortStore.update: %d detection indices for %d slots" % (idx.numel(), n))
        elif n > m:
            raise ValueError("SortStore.update: %d slots for %d detections" % (n, m))
        conf = None
        if confidence is not None:
            if not torch.is_tensor(confidence) and np.ndim(confidence) == 0:
                confidence = np.full(m, float(confidence))
            conf = self._f64(confidence, 0, "update")
            if conf.numel() != m:
                raise ValueError("SortStore.update: %d confidences for %d detections" % (conf.numel(), m))
        status = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return status
        lib = self._state()
        _sort_lib.check(lib.busca_sort_update(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, z.data_ptr(),
                                              None if idx is None else idx.data_ptr(), m, None if conf is None else conf.data_ptr(), status.data_ptr(),
                                              *self._where()))
        return status

    def camera_update(self, slots, matrix):
        """Track.camera_update of the listed slots with the 3 x 3 warp `matrix` (host array or device tensor; what Track.get_matrix returned)."""
        if not torch.is_tensor(matrix):
            matrix = np.asarray(matrix, dtype=np.float64)
        if tuple(matrix.shape) != (3, 3):
            raise ValueError("SortStore.camera_update takes a 3 x 3 matrix, not %s" % (tuple(matrix.shape),))
        slot, n = self._slots(slots, "camera_update")
        if n == 0:
            return
        mat = _small(matrix, self.dev, torch.float64)
        lib = self._state()
        _sort_lib.check(lib.busca_sort_camera_update(self.mean.data_ptr(), self.capacity, slot.data_ptr(), n, mat.data_ptr(), *self._where()))

    def boxes(self, slots, tlbr=True):
        """Track.to_tlbr (to_tlwh with tlbr=False) of the listed slots -> device float64 [n,4]; a skipped entry: a row of NaN."""
        slot, _ = _slots_checked(slots, self.capacity, "SortStore.boxes")
        return self._k.boxes(slot, tlbr)

    # ---- association
    def _gate(self, slot, n, cost, ld_cost, z, mc_lambda, gated_cost, max_distance, out, status=None):
        """busca_sort_gate_cost of n > 0 listed slots and m > 0 measurements into `out` (which may be `cost`) -> device status words [n] (`status`
        if given: a contiguous int32 [n] view the words are written into)."""
        flags = (_sort_lib.MC if mc_lambda is not None else 0) | (_sort_lib.CLAMP if max_distance is not None else 0)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.dev)
        lib = self._state()
        _sort_lib.check(lib.busca_sort_gate_cost(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, z.data_ptr(), z.shape[0],
                                                 cost.data_ptr(), ld_cost, float(gated_cost), flags, 0.0 if mc_lambda is None else float(mc_lambda),
                                                 0.0 if max_distance is None else float(max_distance), out.data_ptr(), status.data_ptr(),
                                                 *self._where()))
        return status

    def gate_cost(self, slots, cost, det_xyah, mc_lambda=None, gated_cost=INFTY_COST, max_distance=None):
        """gate_cost_matrix of the [n,m] matrix `cost` (host array or device tensor, which is left as it is) from the states as they are: `gated_cost`
        where the squared Mahalanobis distance of det_xyah[j] from slots[i]'s projection exceeds 9.4877; with `mc_lambda` every entry then becomes
        mc_lambda * value + (1 - mc_lambda) * distance; with `max_distance` a value above it becomes max_distance + 1e-5 -> (device float64 [n,m],
        device int32 [n] status words: 1 where the projected covariance is not positive definite, that row being NaN).  A skipped slot: a row of
        `gated_cost`, clamped.  One launch."""
        slot, n = self._slots(slots, "gate_cost")
        z = self._f64(_xyah(det_xyah), 4, "gate_cost")
        m = z.shape[0]
        cost = to_dev(cost, self.dev, torch.float64)
        if tuple(cost.shape) != (n, m):
            raise ValueError("SortStore.gate_cost: a %s cost matrix for %d slots and %d detections" % (tuple(cost.shape), n, m))
        out = torch.empty(n, m, dtype=torch.float64, device=self.dev)
        if n == 0 or m == 0:
            return out, torch.zeros(n, dtype=torch.int32, device=self.dev)
        return out, self._gate(slot, n, cost, m, z, mc_lambda, gated_cost, max_distance, out)

    def _stale(self, stale, n, what):
        if stale is None:
            return None
        st = _small(stale if torch.is_tensor(stale) else np.asarray(stale, dtype=np.bool_).astype(np.uint8), self.dev, torch.uint8)
        if st.numel() != n:
            raise ValueError("SortStore.%s: %d `stale` flags for %d slots" % (what, st.numel(), n))
        return st

    def _iou(self, slot, n, st, boxes, max_distance, out=None):
        if out is None:
            out = torch.empty(n, boxes.shape[0], dtype=torch.float64, device=self.dev)
        if n == 0 or boxes.shape[0] == 0:
            return out
        lib = self._state()
        _sort_lib.check(lib.busca_sort_iou_cost(self.mean.data_ptr(), self.capacity, slot.data_ptr(), n, None if st is None else st.data_ptr(),
                                                boxes.data_ptr(), boxes.shape[0], 0 if max_distance is None else _sort_lib.CLAMP,
                                                0.0 if max_distance is None else float(max_distance), out.data_ptr(), *self._where()))
        return out

    def iou_cost(self, slots, det_tlwh, stale=None, max_distance=None):
        """iou_matching.iou_cost of the listed tracks' to_tlwh() against the [m,4] boxes `det_tlwh` -> device float64 [n,m].  `stale`: [n] flags,
        true where time_since_update > 1 - that row is INFTY_COST, as the row of a skipped slot is; `max_distance`: the clamp of min_cost_matching."""
        slot, n = self._slots(slots, "iou_cost")
        return self._iou(slot, n, self._stale(stale, n, "iou_cost"), self._f64(det_tlwh, 4, "iou_cost"), max_distance)

    def appearance_round(self, metric, slots, track_ids, time_since_update, det_features, det_xyah, cascade_depth=None, mc_lambda=None):
        """appearance.appearance_round on resident state: metric.distance of `det_features` [m,E] against the galleries of `track_ids` [n], then gate,
        MC blend and the clamp at metric.matching_threshold in ONE busca_sort_gate_cost launch on that matrix, then busca_linear_assignment - with
        `cascade_depth` once per level of the matching cascade over the tracks with time_since_update == 1 + level, without it (opt.woC) once.  The
        same one device->host copy per level; no state and no matrix crosses.  `slots`, `track_ids`, `time_since_update`: one entry per track.
        -> (matches [(row, detection)], unmatched rows, unmatched detections) with rows indexing `slots`, as appearance_round returns them for
        track_indices = range(n)."""
        slot, n = _slots_checked(slots, self.capacity, "SortStore.appearance_round")
        track_ids = list(track_ids)
        if len(track_ids) != n or (cascade_depth is not None and len(time_since_update) != n):
            raise ValueError("SortStore.appearance_round: %d slots, %d track ids, %d time_since_update entries"
                             % (n, len(track_ids), n if time_since_update is None else len(time_since_update)))
        slot = _small(slot, self.dev, torch.int32)
        z = self._f64(_xyah(det_xyah), 4, "appearance_round")
        m = z.shape[0]
        if n == 0 or m == 0:
            return [], list(range(n)), list(range(m))
        ctx = metric.ctx
        feats = to_dev(det_features, self.dev, torch.float32)
        if feats.shape[0] != m:
            raise ValueError("SortStore.appearance_round: %d feature rows for %d detections" % (feats.shape[0], m))
        cost = metric.distance(feats, track_ids, device=True)
        kstatus = self._gate(slot, n, cost, m, z, mc_lambda, INFTY_COST, metric.matching_threshold, cost)
        limit = metric.matching_threshold + 1e-5
        if cascade_depth is None:
            levels = [list(range(n))]
        else:
            levels = [[r for r in range(n) if time_since_update[r] == 1 + level] for level in range(cascade_depth)]
        matches, cols, checked = [], list(range(m)), False
        for rows in levels:
            if len(cols) == 0:
                break
            if len(rows) == 0:
                continue
            if len(rows) == n and len(cols) == m:
                sub = cost
            else:
                idx = torch.from_numpy(np.asarray(rows + cols, dtype=np.int64)).to(self.dev)     # one upload for both index vectors
                sub = cost.index_select(0, idx[:len(rows)]).index_select(1, idx[len(rows):])
            parts = [_assign_dev(ctx, sub.contiguous(), 1, len(rows), len(cols), limit).view(-1)]
            if not checked:
                parts.append(kstatus)
            host = torch.cat(parts).cpu().numpy()                # one device->host copy: match vectors, solver status, Kalman status words
            if not checked:
                _raise_flagged(host[len(rows) + len(cols) + 1:], "SortStore.appearance_round")
                checked = True
            pairs, _, left = _solved(host, len(rows), len(cols), "SortStore.appearance_round")
            matches += [(rows[r], cols[c]) for r, c in pairs]
            cols = [cols[c] for c in left]
        return matches, list(set(range(n)) - set(k for k, _ in matches)), cols

    def iou_round(self, slots, det_tlwh, max_iou_distance, stale=None, detection_indices=None):
        """The IoU stage of Tracker._match, min_cost_matching(iou_cost, max_iou_distance, ...) on resident state: the cost of the listed tracks
        against det_tlwh[detection_indices] (None: all), clamped, and busca_linear_assignment with the limit max_iou_distance + 1e-5.  Two launches
        and ONE device->host copy of n + m + 1 match words.  -> (matches [(row, detection)], unmatched rows, unmatched detections): rows index
        `slots`, detections are entries of `detection_indices`."""
        slot, n = self._slots(slots, "iou_round")
        st = self._stale(stale, n, "iou_round")
        if detection_indices is not None:
            detection_indices = [int(j) for j in detection_indices]
            if torch.is_tensor(det_tlwh):
                det_tlwh = det_tlwh.to(self.dev).view(-1, 4)[torch.from_numpy(np.asarray(detection_indices, dtype=np.int64)).to(self.dev)]
            else:
                det_tlwh = np.asarray(det_tlwh, dtype=np.float64).reshape(-1, 4)[detection_indices]
        boxes = self._f64(det_tlwh, 4, "iou_round")
        m = boxes.shape[0]
        dets = list(range(m)) if detection_indices is None else detection_indices
        if n == 0 or m == 0:
            return [], list(range(n)), dets
        cost = self._iou(slot, n, st, boxes, max_iou_distance)
        sol = _assign_dev(geometry.default_context(self.dev.index), cost, 1, n, m, max_iou_distance + 1e-5)
        pairs, ua, ub = _solved(sol.cpu().numpy()[0], n, m, "SortStore.iou_round")
        return [(int(r), dets[c]) for r, c in pairs], [int(r) for r in ua], [dets[c] for c in ub]

    def match(self, metric, slots, track_ids, time_since_update, confirmed, det_features, det_xyah, det_tlwh, max_iou_distance, cascade_depth=None,
              mc_lambda=None):
        """Tracker._match (adapters/StrongSORT/deep_sort/tracker.py:214-252) on resident state as ONE staged assignment: metric.distance over all
        n tracks, busca_sort_gate_cost into plane 0 and busca_sort_iou_cost into plane 1 of one [2, n, m] slab, the stage tables of
        _match_stage_tables in one pinned upload, busca_assign_stages, and ONE device->host copy of the match vectors with the Kalman status words
        of the gate behind them - whatever the depth of the cascade; no tensor op and no upload per level.  `slots`, `track_ids`,
        `time_since_update`, `confirmed` (Track.is_confirmed()): one entry per track; `det_features` [m,E], `det_xyah` and `det_tlwh` [m,4]: one
        row per detection.  `cascade_depth`: self.max_age, or None for opt.woC.  Raises LinAlgError where appearance_round on the confirmed tracks
        raises it.  -> (matches [(row, detection)] of the cascade and of the IoU stage in _match's order (_match_order), unmatched rows, unmatched detections); rows
        index `slots`.  appearance_round + iou_round, composed as _match composes them, give the same answer with a copy per populated level."""
        slot, n = _slots_checked(slots, self.capacity, "SortStore.match")
        track_ids = list(track_ids)
        z, boxes = _xyah(det_xyah), det_tlwh
        boxes = boxes if torch.is_tensor(boxes) else np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        m = len(z)
        if not (len(track_ids) == len(time_since_update) == len(confirmed) == n):
            raise ValueError("SortStore.match: %d slots, %d track ids, %d time_since_update entries, %d confirmed flags"
                             % (n, len(track_ids), len(time_since_update), len(confirmed)))
        if len(det_features) != m or len(boxes) != m:
            raise ValueError("SortStore.match: %d feature rows and %d tlwh boxes for %d detections" % (len(det_features), len(boxes), m))
        first, again = _match_stage_tables(time_since_update, confirmed, cascade_depth)
        if n == 0 or m == 0:
            return [], list(range(n)), list(range(m))
        depth = 1 if cascade_depth is None else int(cascade_depth)
        stale = np.asarray(time_since_update).reshape(-1) > 1                  # iou_cost: the row of a track not updated in the last frame is INFTY_COST
        slot = _small(slot, self.dev, torch.int32)
        z = self._f64(z, 4, "match")
        boxes = self._f64(boxes, 4, "match")
        st = self._stale(stale, n, "match")
        ctx = metric.ctx
        feats = to_dev(det_features, self.dev, torch.float32)
        cost = metric.distance(feats, track_ids, device=True)                  # a track without a gallery: a row of +inf, which no stage reads
        slab = torch.empty(1, 2, n, m, dtype=torch.float64, device=self.dev)
        words = 2 * n + m + 1
        out = torch.empty(words + n, dtype=torch.int32, device=self.dev)       # the solver's words | the gate's status words: one copy
        self._gate(slot, n, cost, m, z, mc_lambda, INFTY_COST, metric.matching_threshold, slab[0, 0], out[words:])
        self._iou(slot, n, st, boxes, max_iou_distance, slab[0, 1])
        stages = [(0, metric.matching_threshold + 1e-5)] * depth + [(1, max_iou_distance + 1e-5)]
        _assign_stages_dev(ctx, slab, stages, first, again, None, into=out)
        host = out.cpu().numpy()                                               # the one device->host copy
        conf = np.asarray(confirmed, dtype=bool).reshape(-1)
        if (first[conf] >= 0).any():           # appearance_round gates the confirmed tracks and reads their status words at its first populated level
            _raise_flagged(host[words:] * conf, "SortStore.match")
        if host[words - 1] != 0:
            raise _lib.BuscaError("SortStore.match: the solver ran out of its loop bounds (status %d) - is a cost -inf or a limit infinite?" % int(host[words - 1]))
        r2c, c2r, stage = host[:n], host[n:n + m], host[n + m:2 * n + m]
        rows = [int(r) for r in _match_order(stage, first, depth) if r2c[r] >= 0]
        return [(r, int(r2c[r])) for r in rows], [int(r) for r in np.nonzero(r2c < 0)[0]], [int(j) for j in np.nonzero(c2r < 0)[0]]

    # ---- a whole frame as one chain (busca_sframe.h, libbusca_sframe.so; busca_appearance_cost, busca_assign_stages)
    def _frame_checked(self, slots, time_since_update, confirmed, det_tlwh, det_confidence, det_features, ema_alpha, free_slots, cascade_depth,
                       camera_matrix, predict, what="SortStore.frame"):
        """The host side of frame(), before anything is allocated -> (slot int32 [n], first, again, stale uint8 [n], free int32, tlwh [m,4],
        xyah [m,4], confidences [m] or None, matrix [9] or None)."""
        if self.feature_dim is None:
            raise ValueError("%s needs the feature rows: SortStore(capacity, feature_dim=E)" % what)
        if not APPEAR_E_MIN <= self.feature_dim <= APPEAR_E_MAX or self.feature_dim % 16:
            raise ValueError("%s: feature_dim %d - busca_appearance_cost takes a multiple of 16 in %d .. %d" % (what, self.feature_dim, APPEAR_E_MIN, APPEAR_E_MAX))
        if ema_alpha is None or ema_alpha != ema_alpha:
            raise ValueError("%s needs ema_alpha (opt.EMA_alpha): the feature row is the EMA of deep_sort/track.py:244-248" % what)
        lists = []
        for name, x in (("slots", slots), ("free_slots", free_slots)):
            if torch.is_tensor(x):
                raise ValueError("%s takes host slot lists (%s)" % (what, name))
            lists.append(_slots_checked(x, self.capacity, "%s: %s" % (what, name))[0])
        slot, free = lists
        n = len(slot)
        if (free < 0).any():
            raise ValueError("%s: a free slot is negative" % what)
        taken = np.intersect1d(slot[slot >= 0], free)
        if len(taken):
            raise ValueError("%s: free slot %d is also listed as a track's" % (what, int(taken[0])))
        if not (len(time_since_update) == len(confirmed) == n):
            raise ValueError("%s: %d slots, %d time_since_update entries, %d confirmed flags" % (what, n, len(time_since_update), len(confirmed)))
        tlwh, xyah = _frame_boxes(det_tlwh)
        m = len(tlwh)
        conf = None
        if det_confidence is not None:
            conf = np.asarray(det_confidence, dtype=np.float64).reshape(-1)
            if len(conf) != m:
                raise ValueError("%s: %d confidences for %d detections" % (what, len(conf), m))
        shape = tuple(det_features.shape) if hasattr(det_features, "shape") else np.shape(det_features)
        if m and (len(shape) != 2 or shape[0] != m or shape[1] != self.feature_dim):
            raise ValueError("%s: %s features for %d detections of a store with feature_dim %d" % (what, shape, m, self.feature_dim))
        if n > _lib.ASSIGN_MAX or m > min(_lib.ASSIGN_MAX, _sframe_lib.MAX_DETS):
            raise ValueError("%s: %d tracks and %d detections, the device solver takes at most %d rows and columns" % (what, n, m, _lib.ASSIGN_MAX))
        first, again = _match_stage_tables(time_since_update, confirmed, cascade_depth)
        matrix = None
        if camera_matrix is not None:
            if not predict:
                raise ValueError("%s: the camera update precedes the prediction; with predict=False call camera_update() and predict() yourself" % what)
            if torch.is_tensor(camera_matrix):
                raise ValueError("%s takes a host 3 x 3 camera matrix" % what)
            matrix = np.asarray(camera_matrix, dtype=np.float64)
            if matrix.shape != (3, 3):
                raise ValueError("%s takes a 3 x 3 camera matrix, not %s" % (what, matrix.shape))
            matrix = matrix.reshape(-1)
        stale = (np.asarray(time_since_update, dtype=np.int64).reshape(-1) > 1).astype(np.uint8)
        return slot, first, again, stale, free, tlwh, xyah, conf, matrix

    def frame(self, slots, time_since_update, confirmed, det_tlwh, det_confidence, det_features, max_iou_distance, matching_threshold, ema_alpha,
              free_slots=(), cascade_depth=None, mc_lambda=None, camera_matrix=None, predict=True, apply=True):
        """One Tracker.camera_update / predict / update (adapters/StrongSORT/deep_sort/tracker.py:74-126, 197-252) on resident state as ONE chain on
        the stream: busca_sframe_advance (with `camera_matrix`, Track.camera_update, and then Track.predict - the order of the reference's loop,
        deep_sort_app.py:186-189: the prediction reads the warped height), busca_appearance_cost of `det_features`
        against the feature rows of the listed slots, busca_sframe_cost (both planes of the slab of match(), each row only in the planes its stage
        reads), busca_assign_stages with the stage list and row tables of match(), and - unless `apply` is false - busca_sframe_apply: Track.update of
        every matched track (the EMA feature row, track.py:244-248, then the NSA Kalman update with the detection's confidence) and
        Tracker._initiate_track of every unmatched detection into a free slot (KalmanFilter.initiate and its normalised feature, track.py:85-87)
        -> SortFrame.  Two uploads, five launches and ONE device->host copy of 4 n + 2 m + 1 words whatever the depth of the cascade; the host reads
        the matches after the filter has been enqueued, not before.
          slots, time_since_update, confirmed   host lists, one entry per track in Tracker.tracks order; time_since_update as _match reads it, after
                             Track.predict's increment (match()'s convention); confirmed: Track.is_confirmed()
          det_tlwh           ALL detections of the frame: a host [m,4] array of tlwh boxes or objects with .tlwh; the measurements follow by the
                             operations of Detection.to_xyah.  det_confidence: [m] or None (0 for all)
          det_features       [m, feature_dim] float32; a device tensor is read in place
          matching_threshold, max_iou_distance   metric.matching_threshold and Tracker.max_iou_distance; cascade_depth: Tracker.max_age, None: opt.woC;
                             mc_lambda: opt.MC_lambda or None;  ema_alpha: opt.EMA_alpha
          free_slots         where new tracks go, in the order of their detections; disjoint from the listed tracks (ValueError otherwise).  A
                             detection that finds none left is listed in SortFrame.overflow and nothing is written for it
          predict=False      the states are predicted (and warped) already
        The feature rows are the tracks' own from birth, tentative life included, as the reference's Track keeps them; a listed slot whose row was
        never written (all zero) has NaN appearance costs, which no stage admits.  The reference's BUSCA third round (tracker.py:129-189) matches
        unmatched tracks to their own Kalman candidates and takes no detection, so it commutes with the initiation of new tracks: it works on
        SortFrame.unmatched_tracks through update() afterwards.  Hits, track states and deletion stay on the host.
        Raises LinAlgError where the gate of a row that takes part in the cascade, or an update, finds a projected covariance that is not positive
        definite (that track keeps its Kalman state, its feature row is smoothed all the same, the other tracks are updated) and BuscaError on a
        solver status.  Without detections only the advance happens and nothing is copied; without tracks every detection starts a track."""
        slot, first, again, stale, free, tlwh, xyah, conf, matrix = self._frame_checked(
            slots, time_since_update, confirmed, det_tlwh, det_confidence, det_features, ema_alpha, free_slots, cascade_depth, camera_matrix, predict)
        n, m, n_free, E = len(slot), len(tlwh), len(free), self.feature_dim
        depth = 1 if cascade_depth is None else int(cascade_depth)
        # one pinned upload of every small table: the 16-byte stage records first, then the int32 tables, then the `stale` bytes
        stages = np.zeros(depth + 1, dtype=np.dtype([("plane", "<i4"), ("reserved", "<i4"), ("limit", "<f8")]))
        stages["plane"] = [0] * depth + [1]
        stages["limit"] = [float(matching_threshold) + 1e-5] * depth + [float(max_iou_distance) + 1e-5]
        ints = np.concatenate([slot, first, again, free]).astype(np.int32)
        flags = np.zeros(-(-n // 4) * 4, dtype=np.uint8)
        flags[:n] = stale
        up = h2d_async(np.concatenate([stages.view(np.uint8).reshape(-1), ints.view(np.uint8), flags]), self.dev)
        at = 16 * (depth + 1)
        words = up[at:at + 4 * len(ints)].view(torch.int32)
        d_slot, d_first, d_again, d_free = words[:n], words[n:2 * n], words[2 * n:3 * n], words[3 * n:]
        d_stale = up[at + 4 * len(ints):]
        # one float64 upload: measurements, boxes, confidences, the camera matrix
        parts = ([xyah.reshape(-1), tlwh.reshape(-1)] if m else []) + ([conf] if m and conf is not None else []) + ([matrix] if matrix is not None else [])
        table = small_to_dev(np.concatenate(parts), self.dev, torch.float64) if parts else None
        d_xyah, d_tlwh = (table[:4 * m], table[4 * m:8 * m]) if m else (None, None)
        d_conf = table[8 * m:9 * m] if m and conf is not None else None
        d_matrix = table[table.numel() - 9:] if matrix is not None else None
        self._state()
        flib = _sframe_lib.load()
        where = self._where()
        if predict and n:
            _sframe_lib.check(flib.busca_sframe_advance(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n,
                                                        _lib.ptr(d_matrix), *where))
        if m == 0:
            return SortFrame([], list(range(n)), [], [], [])
        feats = to_dev(det_features, self.dev, torch.float32)
        ctx = geometry.default_context(self.dev.index)
        solved = 2 * n + m + 1                                                 # row_to_col | col_to_row | row_stage | solver status
        out = torch.empty(solved + 2 * n + m, dtype=torch.int32, device=self.dev)      # ... | gate status [n] | update status [n] | new_slot [m]
        slab = torch.empty(1, 2, n, m, dtype=torch.float64, device=self.dev)
        base = out.data_ptr()
        if n:
            cost = torch.empty(n, m, dtype=torch.float64, device=self.dev)
            ctx.check(ctx.lib.busca_appearance_cost(ctx.h, self.feat.data_ptr(), d_slot.data_ptr(), None, n, 1, feats.data_ptr(), m, E, _lib.APPEAR_MIN,
                                                    0, cost.data_ptr(), where[1]))
            _sframe_lib.check(flib.busca_sframe_cost(
                self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n, d_xyah.data_ptr(), d_tlwh.data_ptr(), m,
                d_stale.data_ptr(), cost.data_ptr(), m, INFTY_COST, (_sframe_lib.MC if mc_lambda is not None else 0) | _sframe_lib.CLAMP,
                0.0 if mc_lambda is None else float(mc_lambda), float(matching_threshold), float(max_iou_distance), d_first.data_ptr(),
                d_again.data_ptr(), depth, slab.data_ptr(), base + 4 * solved, *where))
        _assign_stages_dev(ctx, slab, up[:at], d_first, d_again, None, into=out)
        if apply:
            _sframe_lib.check(flib.busca_sframe_apply(
                self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr() if n else None, n, base if n else None, base + 4 * n,
                d_xyah.data_ptr(), _lib.ptr(d_conf), feats.data_ptr(), m, self.feat.data_ptr(), E, float(ema_alpha),
                d_free.data_ptr() if n_free else None, n_free, base + 4 * (solved + 2 * n), base + 4 * (solved + n) if n else None, *where))
        host = (out if apply else out[:solved + n]).cpu().numpy()              # the one device->host copy
        _raise_flagged(host[solved:solved + n], "SortStore.frame")             # the gate's words: only rows of the cascade carry one
        if host[solved - 1] != 0:
            raise _lib.BuscaError("SortStore.frame: the solver ran out of its loop bounds (status %d) - is a cost -inf or a limit infinite?"
                                  % int(host[solved - 1]))
        if apply:
            _raise_flagged(host[solved + n:solved + 2 * n], "SortStore.frame: update")
        r2c, c2r, stage = host[:n], host[n:n + m], host[n + m:2 * n + m]
        rows = [int(r) for r in _match_order(stage, first, depth) if r2c[r] >= 0]
        new = host[solved + 2 * n:] if apply else np.full(m, -1, dtype=np.int32)
        return SortFrame([(r, int(r2c[r])) for r in rows], [int(r) for r in np.nonzero(r2c < 0)[0]], [int(j) for j in np.nonzero(c2r < 0)[0]],
                         [(j, int(new[j])) for j in range(m) if new[j] >= 0], [j for j in range(m) if new[j] == -2])

    # ---- the frames of many sequences as one chain (busca_msframe.h, libbusca_msframe.so; busca_assign_stages over the batch)
    def _frame_batch_checked(self, problems, ema_alpha, cascade_depth, predict):
        """The host side of frame_batch(), before anything is allocated -> ([what _frame_checked returns, per problem], the SortFrameProblems,
        whether the features are device tensors)."""
        what = "SortStore.frame_batch"
        problems = [p if isinstance(p, SortFrameProblem) else SortFrameProblem(*p) for p in problems]
        if len(problems) > _msframe_lib.MAX_BATCH:
            raise ValueError("%s: %d problems, one call takes %d" % (what, len(problems), _msframe_lib.MAX_BATCH))
        checked, on_device = [], None
        for k, p in enumerate(problems):
            name = "%s: problem %d" % (what, k)
            try:
                c = self._frame_checked(p.slots, p.time_since_update, p.confirmed, p.det_tlwh, p.det_confidence, p.det_features, ema_alpha,
                                        p.free_slots, cascade_depth, p.camera_matrix, predict, what=name)
            except ValueError as e:
                if name in str(e):
                    raise
                raise ValueError("%s: %s" % (name, e)) from None
            if len(c[5]):                                                      # one feature table: concatenated on the host, or by one torch.cat
                dev = torch.is_tensor(p.det_features)
                if on_device is None:
                    on_device = dev
                elif on_device != dev:
                    raise ValueError("%s: host and device det_features in one batch (the earlier problems gave %s)"
                                     % (name, "device tensors" if on_device else "host arrays"))
            checked.append(c)
        if len(checked) > 1:                                                   # one launch serves them all: what two problems share, two workgroups race on
            rows = np.concatenate([c[0] for c in checked])
            taken = np.concatenate([rows[rows >= 0]] + [c[4] for c in checked])
            if len(np.unique(taken)) != len(taken):
                slots, count = np.unique(taken, return_counts=True)
                raise ValueError("%s: the tracks and the free slots must be distinct across the whole batch (slot %d is listed twice)"
                                 % (what, int(slots[count > 1][0])))
        return checked, problems, bool(on_device)

    def frame_batch(self, problems, max_iou_distance, matching_threshold, ema_alpha, cascade_depth=None, mc_lambda=None, predict=True, apply=True):
        """frame() of every SortFrameProblem(slots, time_since_update, confirmed, det_tlwh, det_confidence, det_features, free_slots, camera_matrix)
        of a list - the frames of one time step of many sequences that share this store - as ONE chain on the stream -> [SortFrame], each what
        frame() returns for that problem alone, the states and feature rows bit for bit what the frames one after the other leave.  Whatever the
        number of problems: one pinned upload of every small table, one float64 upload of the detection tables and the camera matrices, the
        feature table (host arrays concatenated and uploaded once, device tensors by one torch.cat), busca_msframe_advance, busca_msframe_cost
        (which forms the appearance entries of its tiles itself: no appearance launch, no [n, m] matrix), busca_assign_stages over the batch with
        its `dims`, busca_msframe_apply, and ONE device->host copy of B (4 N + 2 M + 1) words, N and M the largest track and detection counts.
        The thresholds, `ema_alpha`, `mc_lambda` and `cascade_depth` are the batch's, as the solver's stage table is; the camera matrix is the
        problem's.  A problem with det_confidence=None has confidence 0.  The tracks and the free slots must be distinct across the whole batch
        (ValueError, before anything is allocated).  An empty list gives []; without any detection only the advance happens and nothing is
        copied; a problem without tracks starts a track per detection.  Raises LinAlgError (a gate or an update) and BuscaError (a solver status)
        naming the problem, after the whole batch has been applied.  For a single sequence frame() is the shorter route."""
        checked, problems, on_device = self._frame_batch_checked(problems, ema_alpha, cascade_depth, predict)
        B = len(checked)
        if B == 0:
            return []
        what = "SortStore.frame_batch"
        W, E = _msframe_lib.PROBLEM_WORDS, self.feature_dim
        depth = 1 if cascade_depth is None else int(cascade_depth)
        n_k, m_k, f_k = ([len(c[i]) for c in checked] for i in (0, 5, 4))
        N, M = max(n_k), max(m_k)
        n_total, m_total, f_total = sum(n_k), sum(m_k), sum(f_k)
        with_matrix = [k for k, c in enumerate(checked) if c[8] is not None]
        table = np.zeros((B, W), dtype=np.int32)                               # row_begin, n_k, det_begin, m_k, free_begin, n_free_k, matrix_k
        table[:, 1], table[:, 3], table[:, 5], table[:, 6] = n_k, m_k, f_k, -1
        table[1:, 0:6:2] = np.cumsum(table[:-1, 1:6:2], axis=0)
        table[with_matrix, 6] = np.arange(len(with_matrix))
        first, again = (np.full((B, N), -1, dtype=np.int32) for _ in range(2))  # padded for the solver; the kernels read the concatenated lists
        for k, c in enumerate(checked):
            first[k, :n_k[k]], again[k, :n_k[k]] = c[1], c[2]
        # one pinned upload of every small table: the 16-byte stage records first, then the int32 tables, then the `stale` bytes
        stages = np.zeros(depth + 1, dtype=np.dtype([("plane", "<i4"), ("reserved", "<i4"), ("limit", "<f8")]))
        stages["plane"] = [0] * depth + [1]
        stages["limit"] = [float(matching_threshold) + 1e-5] * depth + [float(max_iou_distance) + 1e-5]
        parts = [np.concatenate([c[0] for c in checked]), table.reshape(-1), table[:, 1:4:2].reshape(-1), first.reshape(-1), again.reshape(-1),
                 np.concatenate([c[1] for c in checked]), np.concatenate([c[2] for c in checked]), np.concatenate([c[4] for c in checked])]
        ints = np.concatenate(parts).astype(np.int32)
        flags = np.zeros(-(-n_total // 4) * 4, dtype=np.uint8)
        flags[:n_total] = np.concatenate([c[3] for c in checked])
        up = h2d_async(np.concatenate([stages.view(np.uint8).reshape(-1), ints.view(np.uint8), flags]), self.dev)
        at = 16 * (depth + 1)
        d_slot, d_table, d_dims, d_first, d_again, d_first_rows, d_again_rows, d_free = up[at:at + 4 * len(ints)].view(torch.int32).split([len(p) for p in parts])
        d_stale = up[at + 4 * len(ints):]
        # one float64 upload: measurements, boxes, confidences (zeros where a problem gives none), the camera matrices
        with_conf = m_total > 0 and any(c[7] is not None for c in checked)
        cols = []
        if m_total:
            cols = [c[6].reshape(-1) for c in checked] + [c[5].reshape(-1) for c in checked]
            if with_conf:
                cols += [np.zeros(m) if c[7] is None else c[7] for m, c in zip(m_k, checked)]
        cols += [checked[k][8] for k in with_matrix]
        dets = small_to_dev(np.concatenate(cols), self.dev, torch.float64) if cols else None
        d_xyah, d_tlwh = (dets[:4 * m_total], dets[4 * m_total:8 * m_total]) if m_total else (None, None)
        d_conf = dets[8 * m_total:9 * m_total] if with_conf else None
        d_matrices = dets[dets.numel() - 9 * len(with_matrix):] if with_matrix else None
        self._state()
        mlib = _msframe_lib.load()
        where = self._where()
        if predict and n_total:
            _msframe_lib.check(mlib.busca_msframe_advance(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n_total, m_total,
                                                          f_total, _lib.ptr(d_matrices), len(with_matrix), d_table.data_ptr(), B, N, M, *where))
        if M == 0:
            return [SortFrame([], list(range(n)), [], [], []) for n in n_k]
        # the feature table: one upload, or one concatenation on the device
        rows = [p.det_features for p, m in zip(problems, m_k) if m]
        if on_device:
            feats = [to_dev(r, self.dev, torch.float32) for r in rows]
            feats = feats[0] if len(feats) == 1 else torch.cat(feats)
        else:
            feats = to_dev(np.concatenate([np.asarray(r, dtype=np.float32) for r in rows]), self.dev, torch.float32)
        ctx = geometry.default_context(self.dev.index)
        solved = B * (2 * N + M + 1)                                           # row_to_col [B,N] | col_to_row [B,M] | row_stage [B,N] | solver status [B]
        out = torch.empty(solved + B * (2 * N + M), dtype=torch.int32, device=self.dev)      # ... | gate status [B,N] | update status [B,N] | new_slot [B,M]
        slab = torch.empty(B, 2, N, M, dtype=torch.float64, device=self.dev)
        base = out.data_ptr()
        if N:
            _msframe_lib.check(mlib.busca_msframe_cost(
                self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n_total, d_xyah.data_ptr(), d_tlwh.data_ptr(),
                feats.data_ptr(), m_total, f_total, len(with_matrix), d_stale.data_ptr(), self.feat.data_ptr(), E, INFTY_COST,
                (_msframe_lib.MC if mc_lambda is not None else 0) | _msframe_lib.CLAMP, 0.0 if mc_lambda is None else float(mc_lambda),
                float(matching_threshold), float(max_iou_distance), d_first_rows.data_ptr(), d_again_rows.data_ptr(), depth, d_table.data_ptr(), B, N, M,
                slab.data_ptr(), base + 4 * solved, *where))
        _assign_stages_dev(ctx, slab, up[:at], d_first, d_again, d_dims, into=out)
        if apply:
            _msframe_lib.check(mlib.busca_msframe_apply(
                self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr() if n_total else None, n_total, base if N else None,
                base + 4 * B * N, d_xyah.data_ptr(), _lib.ptr(d_conf), feats.data_ptr(), m_total, self.feat.data_ptr(), E, float(ema_alpha),
                d_free.data_ptr() if f_total else None, f_total, len(with_matrix), d_table.data_ptr(), B, N, M, base + 4 * (solved + 2 * B * N),
                base + 4 * (solved + B * N) if N else None, *where))
        host = (out if apply else out[:solved + B * N]).cpu().numpy()          # the one device->host copy
        # the words of problem k are the corner (n_k, m_k) of its blocks: the kernels write nothing else, and nothing else is read
        r2c, c2r, stage, status = np.split(host[:solved], [B * N, B * (N + M), B * (2 * N + M)])
        r2c, c2r, stage = r2c.reshape(B, N), c2r.reshape(B, M), stage.reshape(B, N)
        gate = host[solved:solved + B * N].reshape(B, N)
        flagged, new = (host[solved + B * N:solved + 2 * B * N].reshape(B, N), host[solved + 2 * B * N:].reshape(B, M)) if apply else (None, None)
        for k, (n, m) in enumerate(zip(n_k, m_k)):                             # in the order frame() raises, problem by problem
            name = "%s: problem %d" % (what, k)
            if n and m:                                                        # the cost kernel writes the words of the problems that have a tile
                _raise_flagged(gate[k, :n], name)
            if status[k] != 0:
                raise _lib.BuscaError("%s: the solver ran out of its loop bounds (status %d) - is a cost -inf or a limit infinite?" % (name, int(status[k])))
            if apply and m:
                _raise_flagged(flagged[k, :n], name + ": update")
        frames = []
        for k, (n, m) in enumerate(zip(n_k, m_k)):
            if m == 0:
                frames.append(SortFrame([], list(range(n)), [], [], []))
                continue
            r, c, st = r2c[k, :n], c2r[k, :m], stage[k, :n]
            rows = [int(i) for i in _match_order(st, checked[k][1], depth) if r[i] >= 0]
            started = new[k, :m] if apply else np.full(m, -1, dtype=np.int32)
            frames.append(SortFrame([(i, int(r[i])) for i in rows], [int(i) for i in np.nonzero(r < 0)[0]], [int(j) for j in np.nonzero(c < 0)[0]],
                                    [(j, int(started[j])) for j in range(m) if started[j] >= 0], [j for j in range(m) if started[j] == -2]))
        return frames

    def features(self, slots):
        """The feature rows of the listed slots -> device float32 [n, feature_dim]; a negative entry gives the spare slot's row."""
        slot, n = _slots_checked(slots, self.capacity, "SortStore.features")
        if self.feature_dim is None:
            raise ValueError("SortStore.features: the store keeps no feature rows (feature_dim)")
        self._state()
        return self.feat.index_select(0, self._feature_rows(slot))

    def load_features(self, slots, rows):
        """The [n, feature_dim] `rows` (host array or device tensor) into the feature rows of the listed slots as they are - not normalised: for a
        tracker that migrates, and for tests.  A negative entry is parked in the spare slot."""
        slot, n = _slots_checked(slots, self.capacity, "SortStore.load_features")
        if self.feature_dim is None:
            raise ValueError("SortStore.load_features: the store keeps no feature rows (feature_dim)")
        shape = tuple(rows.shape) if hasattr(rows, "shape") else np.shape(rows)
        if shape != (n, self.feature_dim):
            raise ValueError("SortStore.load_features: %s rows for %d slots of %d values" % (shape, n, self.feature_dim))
        rows = to_dev(rows, self.dev, torch.float32)
        self._state()
        if n:
            self.feat.index_copy_(0, self._feature_rows(slot), rows)

    def _feature_rows(self, slot):
        if torch.is_tensor(slot):
            idx = slot.to(device=self.dev, dtype=torch.int64)
            return torch.where((idx < 0) | (idx > self.capacity), self.capacity, idx)
        return small_to_dev(np.where(slot < 0, self.capacity, slot).astype(np.int64), self.dev, torch.int64)

    # ---- objects in and out
    def load(self, slots, tracks):
        """The states of objects with `.mean` [8] / `.covariance` [8,8] into their slots (one upload)."""
        slot, _ = _slots_checked(slots, self.capacity, "SortStore.load")
        self._k.load(slot, tracks)

    def store(self, slots, tracks):
        """The states of the listed slots into the objects' `.mean` / `.covariance` (one device->host copy)."""
        slot, _ = _slots_checked(slots, self.capacity, "SortStore.store")
        self._k.store(slot, tracks)
