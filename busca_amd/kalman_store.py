"""ByteTrack's Kalman state resident on the device: the means and covariances of all tracks stay in two device tensors over `capacity` slots, and
every step names the slots it serves.  Fronts include/busca_track.h (libbusca_track.so, bound by _track_lib) and, for the rounds of several sequences
at once, include/busca_rounds.h (libbusca_rounds.so, bound by _rounds_lib), for a whole frame as one chain include/busca_frame.h
(libbusca_frame.so, bound by _frame_lib), and for the frames of many sequences as one chain include/busca_mframe.h (libbusca_mframe.so, bound by
_mframe_lib); restates what kalman.py restates -
adapters/ByteTrack/yolox/tracker/kalman_filter.py, matching.py:132-186, byte_tracker.py:50-61,67,78,109,142-163 - without the objects: no state
crosses PCIe in either direction, and the cost matrix of an association round is one launch."""
import collections

import numpy as np
import torch

from . import _frame_lib, _lib, _mframe_lib, _rounds_lib, _track_lib, geometry
from ._xfer import h2d_async, small_to_dev, stream_of
from .assignment import _assign_dev, _assign_stages_dev, _empty_triple, _solved, _triple
from .ghost_motion import _slots_checked
from .kalman import _measurements, _raise_flagged, _set_states
from .track_boxes import _tlbrs

# the detections of a call on the device: tlbr [m,4], xyah [m,4], score [m] or None - views of one uploaded table
DeviceDetections = collections.namedtuple("DeviceDetections", "tlbr xyah score m")
# one sequence's association round in a batch (cost_batch, round_batch): a host slot list and what round() takes beside it
RoundProblem = collections.namedtuple("RoundProblem", "slots detections det_scores not_tracked", defaults=(None, None))
# what KalmanStore.frame returns: the matches of the three rounds as (row, detection) - rows index pool_slots (first, second) or unconfirmed_slots
# (unconfirmed), detections the list as given, each list ascending by row -, the pool rows no round matched (those that are Tracked, then the lost
# ones: byte_tracker.py:364), the unconfirmed rows left over, the tracks started as (detection, slot), the detections that would have started one but
# found the store full, and the class of every detection (0 first round, 1 second round, 2 neither)
ByteFrame = collections.namedtuple("ByteFrame", "first second unconfirmed unmatched_pool unmatched_unconfirmed new_tracks overflow det_class")
FRAME_STAGES = 3               # first round, second round, unconfirmed round
# one sequence's frame in a batch (frame_batch): what frame() takes of the sequence itself - the thresholds belong to the batch
FrameProblem = collections.namedtuple("FrameProblem", "pool_slots lost unconfirmed_slots detections det_scores free_slots", defaults=((),))


assert (_rounds_lib.FUSE_MOTION, _rounds_lib.ONLY_POSITION, _rounds_lib.GATE_ONLY) == (_track_lib.FUSE_MOTION, _track_lib.ONLY_POSITION, _track_lib.GATE_ONLY)


def _scores(det_scores, m):
    sc = np.asarray(det_scores, dtype=np.float64).reshape(-1)
    if len(sc) != m:
        raise ValueError("KalmanStore: %d scores for %d detections" % (len(sc), m))
    return sc


def _small(x, dev, dtype):
    """_xfer.small_to_dev; an empty table needs no staging."""
    if not torch.is_tensor(x) and np.size(x) == 0:
        return torch.empty(0, dtype=dtype, device=dev)
    return small_to_dev(x, dev, dtype)


def _frame_classes(det_scores, track_thresh, low_thresh=0.1):
    """The round of every detection by the comparisons of byte_tracker.py:244-249, made by numpy on the scores as given -> uint8 [m]: 0 where
    score > track_thresh (first round), 1 where score > low_thresh and score < track_thresh (second round), 2 elsewhere - a score equal to
    track_thresh, or not above low_thresh, belongs to neither round."""
    scores = np.asarray(det_scores).reshape(-1)
    remain = scores > track_thresh
    second = np.logical_and(scores > low_thresh, scores < track_thresh)
    cls = np.full(len(scores), _frame_lib.CLASS_NONE, dtype=np.uint8)
    cls[second] = _frame_lib.CLASS_SECOND
    cls[remain] = _frame_lib.CLASS_FIRST
    return cls


def _frame_row_tables(lost, n_pool, n_unconfirmed):
    """The row tables of a frame's staged assignment -> (first, again) int32 [n_pool + n_unconfirmed], (lost) bool [n_pool].  Stage 0 is the first
    round (every pool row), stage 1 the second (again the pool rows that are Tracked), stage 2 the round of the unconfirmed tracks."""
    lost = np.asarray(lost, dtype=np.bool_).reshape(-1)
    if len(lost) != n_pool:
        raise ValueError("KalmanStore.frame: %d `lost` flags for %d pool slots" % (len(lost), n_pool))
    first = np.concatenate([np.zeros(n_pool, dtype=np.int32), np.full(n_unconfirmed, 2, dtype=np.int32)])
    again = np.concatenate([np.where(lost, -1, 1).astype(np.int32), np.full(n_unconfirmed, -1, dtype=np.int32)])
    return first, again, lost


def _stage_records(match_thresh, second_thresh, unconfirmed_thresh):
    """The stage table of a frame's staged assignment as bytes: rounds 1 and 3 read plane 0 of the slab, round 2 plane 1."""
    stages = np.zeros(FRAME_STAGES, dtype=np.dtype([("plane", "<i4"), ("reserved", "<i4"), ("limit", "<f8")]))
    stages["plane"] = [0, 1, 0]
    stages["limit"] = [float(match_thresh), float(second_thresh), float(unconfirmed_thresh)]
    return stages.view(np.uint8).reshape(-1)


def _byte_frame(r2c, stage, new, n_pool, lost, cls):
    """The ByteFrame of one problem from its words of the solver (row_to_col, row_stage [n]) and of the filter (new_slot [m])."""
    n, m = len(r2c), len(new)
    matched = [i for i in range(n) if r2c[i] >= 0]
    left = [i for i in range(n_pool) if r2c[i] < 0]
    return ByteFrame([(i, int(r2c[i])) for i in matched if i < n_pool and stage[i] == 0],
                     [(i, int(r2c[i])) for i in matched if i < n_pool and stage[i] == 1],
                     [(i - n_pool, int(r2c[i])) for i in matched if i >= n_pool],
                     [i for i in left if not lost[i]] + [i for i in left if lost[i]],      # the Tracked rows no round matched, then the lost ones (:364)
                     [i - n_pool for i in range(n_pool, n) if r2c[i] < 0],
                     [(j, int(new[j])) for j in range(m) if new[j] >= 0], [j for j in range(m) if new[j] == -2], cls)


def _frame_detections(detections):
    """The detections of frame() on the host -> (measurements [m,4], boxes [m,4]).  Objects give tlwh_to_xyah(.tlwh) and .tlbr, as everywhere; a
    host [m,4] array is taken as (x, y, a, h) measurements, exactly, and the boxes follow as STrack.tlbr derives them from a state."""
    if torch.is_tensor(detections) or isinstance(detections, DeviceDetections):
        raise ValueError("KalmanStore.frame takes detection objects with .tlwh and .tlbr, or a host [m,4] array of measurements")
    xyah = _measurements(detections)
    if not isinstance(detections, np.ndarray):
        return xyah, _tlbrs(detections)
    wh = np.stack([xyah[:, 2] * xyah[:, 3], xyah[:, 3]], 1)
    tl = xyah[:, :2] - wh / 2
    return xyah, np.concatenate([tl, wh + tl], 1)


class KalmanStore:
    """The Kalman state of up to `capacity` tracks on the device (busca_track_kalman_*, busca_track_round_cost):
      initiate(slots, dets)          KalmanFilter.initiate: STrack.activate's state of a new track - also how a slot is reused
      predict(slots, not_tracked)    STrack.multi_predict in place
      update(slots, dets, det_index) KalmanFilter.update in place -> device status words
      boxes(slots)                   STrack.tlbr / tlwh
      cost(slots, dets, ...)         the cost matrix of one association round, one launch -> (device [n,m], device status [n])
      round(slots, dets, thresh)     predict, cost and the linear assignment -> (matches, u_track, u_detection); one small device->host copy
      detections_batch / cost_batch / round_batch(problems, ...)   the same for the rounds of many sequences that share the store: a list of
                                     RoundProblem, one launch per step and one copy back whatever its length (busca_rounds_cost)
      frame(pool, lost, unconfirmed, dets, scores, ...)   a whole BYTETracker.update on the state: predict, the three rounds as one staged
                                     assignment, update and initiation -> ByteFrame; four launches and one copy home whatever the track count
      frame_batch(problems, ...)     the frames of one time step of many sequences that share the store: a list of FrameProblem, the same four
                                     launches and one copy home whatever its length (busca_mframe_cost, busca_mframe_apply) -> [ByteFrame]
      load / store(slots, stracks)   states from / to objects with `.mean` / `.covariance`, for a tracker that migrates call by call
    `mean` [capacity + 1, 8] and `cov` [capacity + 1, 8, 8] are float64 device tensors, allocated at the first call that needs them; the slot behind
    the last is a spare no kernel writes (the kernels are told `capacity`), where load / store park the negative entries of a slot list.
    Slot lists given as host lists or arrays are checked on the host - the entries >= 0 distinct and below `capacity`, ValueError otherwise; a negative
    entry is skipped.  A slot list given as a device tensor is not read back: it is the caller's to keep distinct, and entries outside the capacity
    are skipped by the kernels and touch no memory.  Detections: objects with `.tlwh` (and `.tlbr` for cost / round), a host [m,4] array or device
    tensor of (x, y, a, h) measurements where only those are needed, or what detections() returned.  Every call is asynchronous on torch's
    current stream of the device, except that round(), round_batch(), frame(), frame_batch(), load() of nothing and store() wait for their one copy."""

    def __init__(self, capacity, device=None):
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("KalmanStore(capacity=%d)" % capacity)
        self.capacity = capacity
        self.dev = torch.device("cuda", 0 if device is None else (device.index or 0) if isinstance(device, torch.device) else int(device))
        self.mean = self.cov = None
        self._lib = None

    # ---- plumbing
    def _state(self):
        if self.mean is None:
            self.mean = torch.zeros(self.capacity + 1, 8, dtype=torch.float64, device=self.dev)
            self.cov = torch.zeros(self.capacity + 1, 8, 8, dtype=torch.float64, device=self.dev)
        if self._lib is None:
            self._lib = _track_lib.load()
        return self._lib

    def _slots(self, slots, what):
        """-> (device i32 [n], n); a host list is checked first, before anything is allocated."""
        slot, n = _slots_checked(slots, self.capacity, "KalmanStore." + what)
        return _small(slot, self.dev, torch.int32), n

    def _where(self):
        return self.dev.index, stream_of(self.dev)

    def detections(self, detections, det_scores=None, boxes=True):
        """The detections of one or more calls in one upload -> DeviceDetections.  `detections`: objects with `.tlwh` and (`boxes`) `.tlbr`, or a host
        [m,4] array of (x, y, a, h) measurements (then there are no boxes: enough for initiate and update)."""
        if isinstance(detections, DeviceDetections):
            return detections
        if torch.is_tensor(detections):
            z = detections.to(device=self.dev, dtype=torch.float64).contiguous().view(-1, 4)
            return DeviceDetections(None, z, None, z.shape[0])
        xyah = _measurements(detections)
        m = xyah.shape[0]
        boxes = boxes and not isinstance(detections, np.ndarray)
        if m == 0:
            none = torch.empty(0, 4, dtype=torch.float64, device=self.dev)
            return DeviceDetections(none if boxes else None, none, None, 0)
        return self._det_table(xyah, _tlbrs(detections) if boxes else None, None if det_scores is None else _scores(det_scores, m))

    def _det_table(self, xyah, tlbr, scores):
        """One float64 upload of m > 0 measurements, their boxes (or None) and scores (or None) -> DeviceDetections of its views."""
        m = xyah.shape[0]
        parts = [xyah.reshape(-1)] + ([] if tlbr is None else [tlbr.reshape(-1)]) + ([] if scores is None else [scores])
        table = small_to_dev(np.concatenate(parts), self.dev, torch.float64)
        score_at = 4 * m if tlbr is None else 8 * m
        return DeviceDetections(None if tlbr is None else table[4 * m:8 * m].view(m, 4), table[:4 * m].view(m, 4),
                                None if scores is None else table[score_at:score_at + m], m)

    def detections_batch(self, list_of_detections, list_of_scores=None, boxes=True):
        """The detections of several sequences as ONE table in one upload -> (DeviceDetections of the concatenation, host int32 [B + 1] `begin`):
        sequence k's detections are rows begin[k] .. begin[k + 1] - 1, so one later update / initiate of all sequences indexes the table with
        det_index + begin[k].  Each entry is what detections() takes from the host; boxes are kept when every entry is a list of objects.
        `list_of_scores`: None, or one score vector per sequence - given for all sequences or for none, ValueError otherwise."""
        B = len(list_of_detections)
        scores = None
        if list_of_scores is not None:
            if len(list_of_scores) != B:
                raise ValueError("KalmanStore.detections_batch: %d score vectors for %d detection lists" % (len(list_of_scores), B))
            given = [sc is not None for sc in list_of_scores]
            if any(given) != all(given):
                raise ValueError("KalmanStore.detections_batch: scores are given for all problems or for none (problem %d has none)" % given.index(False))
            scores = list_of_scores if B and given[0] else None
        xyah = [_measurements(d) for d in list_of_detections]
        begin = np.zeros(B + 1, dtype=np.int32)
        begin[1:] = np.cumsum([z.shape[0] for z in xyah])
        m = int(begin[-1])
        boxes = boxes and not any(isinstance(d, np.ndarray) for d in list_of_detections)
        if scores is not None:
            scores = np.concatenate([_scores(sc, z.shape[0]) for sc, z in zip(scores, xyah)])
        if m == 0:
            none = torch.empty(0, 4, dtype=torch.float64, device=self.dev)
            return DeviceDetections(none if boxes else None, none, None, 0), begin
        tlbr = np.concatenate([_tlbrs(d) for d in list_of_detections]) if boxes else None
        return self._det_table(np.concatenate(xyah), tlbr, scores), begin

    def _pairs(self, slots, detections, det_index, what):
        slot, n = self._slots(slots, what)
        det = self.detections(detections, boxes=False)
        idx = None
        if det_index is not None:
            idx = _small(det_index if torch.is_tensor(det_index) else np.asarray(det_index, dtype=np.int32), self.dev, torch.int32)
            if idx.numel() != n:
                raise ValueError("KalmanStore.%s: %d detection indices for %d slots" % (what, idx.numel(), n))
        elif n > det.m:
            raise ValueError("KalmanStore.%s: %d slots for %d detections" % (what, n, det.m))
        return slot, n, det, idx

    # ---- the filter
    def initiate(self, slots, detections, det_index=None):
        """KalmanFilter.initiate of detection det_index[i] (None: i) into slot slots[i]: a new track, or a new tenant of an abandoned slot."""
        slot, n, det, idx = self._pairs(slots, detections, det_index, "initiate")
        if n == 0:
            return
        lib = self._state()
        _track_lib.check(lib.busca_track_kalman_initiate(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, det.xyah.data_ptr(),
                                                         None if idx is None else idx.data_ptr(), det.m, *self._where()))

    def predict(self, slots, not_tracked=None):
        """STrack.multi_predict of the listed slots in place; not_tracked[i] true: mean[7] of that track is zeroed first (state != Tracked)."""
        slot, n = self._slots(slots, "predict")
        self._predict(slot, n, not_tracked)

    def _predict(self, slot, n, not_tracked):
        nt = None
        if not_tracked is not None:
            nt = _small(not_tracked if torch.is_tensor(not_tracked) else np.asarray(not_tracked, dtype=np.bool_).astype(np.uint8), self.dev, torch.uint8)
            if nt.numel() != n:
                raise ValueError("KalmanStore.predict: %d `not_tracked` flags for %d slots" % (nt.numel(), n))
        if n == 0:
            return
        lib = self._state()
        _track_lib.check(lib.busca_track_kalman_predict(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(),
                                                        None if nt is None else nt.data_ptr(), n, *self._where()))

    def update(self, slots, detections, det_index=None):
        """KalmanFilter.update of slot slots[i] with detection det_index[i] (None: i), in place -> device int32 [n] status words: 1 where the
        reference raises LinAlgError (that slot keeps its state), which is the caller's to read or not."""
        slot, n, det, idx = self._pairs(slots, detections, det_index, "update")
        status = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return status
        lib = self._state()
        _track_lib.check(lib.busca_track_kalman_update(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, det.xyah.data_ptr(),
                                                       None if idx is None else idx.data_ptr(), det.m, status.data_ptr(), *self._where()))
        return status

    def boxes(self, slots, tlbr=True):
        """STrack.tlbr (tlwh with tlbr=False) of the listed slots -> device float64 [n,4]; a skipped entry: a row of NaN."""
        slot, n = self._slots(slots, "boxes")
        out = torch.empty(n, 4, dtype=torch.float64, device=self.dev)
        if n == 0:
            return out
        lib = self._state()
        _track_lib.check(lib.busca_track_kalman_boxes(self.mean.data_ptr(), self.capacity, slot.data_ptr(), n, int(bool(tlbr)), out.data_ptr(), *self._where()))
        return out

    # ---- association
    def cost(self, slots, detections, det_scores=None, fuse_motion=False, only_position=False, lambda_=0.98, gate_only=False):
        """The cost matrix of one association round from the states as they are (after predict): iou_distance of the tracks' boxes, fuse_score with
        `det_scores`, matching.fuse_motion with `fuse_motion` (`gate_only`: gate_cost_matrix, no blend) -> (device float64 [n,m], device int32 [n]
        status words: 1 where the projected covariance is not positive definite, that row being NaN).  A skipped slot: a row of +inf.  One launch."""
        slot, n = self._slots(slots, "cost")
        return self._cost(slot, n, self.detections(detections, det_scores), fuse_motion, only_position, lambda_, gate_only)

    @staticmethod
    def _flags(det, fuse_motion, only_position, gate_only):
        """The flag word of busca_track_round_cost / busca_rounds_cost (one set of values: busca_rounds.h takes busca_track.h's)."""
        if fuse_motion and gate_only:
            raise ValueError("KalmanStore.cost: fuse_motion and gate_only exclude each other")
        if det.tlbr is None:
            raise ValueError("KalmanStore.cost: the detections carry no boxes (objects with .tlbr and .tlwh are needed)")
        flags = (_track_lib.FUSE_MOTION if fuse_motion else 0) | (_track_lib.GATE_ONLY if gate_only else 0)
        return flags | _track_lib.ONLY_POSITION if flags and only_position else flags

    def _cost(self, slot, n, det, fuse_motion, only_position, lambda_, gate_only=False):
        flags = self._flags(det, fuse_motion, only_position, gate_only)
        out = torch.empty(n, det.m, dtype=torch.float64, device=self.dev)
        if n == 0 or det.m == 0:
            return out, torch.zeros(n, dtype=torch.int32, device=self.dev)
        status = torch.empty(n, dtype=torch.int32, device=self.dev)
        lib = self._state()
        _track_lib.check(lib.busca_track_round_cost(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), n, det.tlbr.data_ptr(),
                                                    det.xyah.data_ptr(), None if det.score is None else det.score.data_ptr(), det.m, flags, float(lambda_),
                                                    out.data_ptr(), status.data_ptr(), *self._where()))
        return out, status

    def round(self, slots, detections, thresh, det_scores=None, fuse_motion=False, only_position=False, lambda_=0.98, not_tracked=None, predict=True):
        """One whole association round, assignment.associate_round on resident state: predict (unless `predict` is false: the states are predicted
        already), the cost matrix, linear_assignment(cost, thresh) -> (matches, u_track, u_detection) with rows indexing `slots`.  Three launches;
        ONE device->host copy of n + m + 1 match words and n status words - no state and no matrix crosses.  Raises LinAlgError where
        associate_round does, after the prediction of every listed track."""
        slot, n = self._slots(slots, "round")
        det = self.detections(detections, det_scores)
        if predict:
            self._predict(slot, n, not_tracked)
        if n == 0 or det.m == 0:
            return _empty_triple(n, det.m)
        cost, status = self._cost(slot, n, det, fuse_motion, only_position, lambda_)
        sol = _assign_dev(geometry.default_context(self.dev.index), cost, 1, n, det.m, thresh)
        host = torch.cat([sol.view(-1), status]).cpu().numpy()
        _raise_flagged(host[n + det.m + 1:], "KalmanStore.round")
        return _solved(host[:n + det.m + 1].astype(np.int64), n, det.m, "KalmanStore.round")

    # ---- the rounds of many sequences in one launch each (busca_rounds.h, libbusca_rounds.so)
    def _batch_checked(self, problems, what, distinct):
        """The host side of a batch, before anything is allocated -> (RoundProblems, the concatenated slot list int32 [n_total], its begin [B + 1],
        the concatenated `not_tracked` flags uint8 [n_total] or None).  Each slot list is checked as round() checks it; `distinct`: and the entries
        >= 0 across the whole batch, which one predict launch would race on otherwise."""
        problems = [p if isinstance(p, RoundProblem) else RoundProblem(*p) for p in problems]
        if len(problems) > _rounds_lib.MAX_BATCH:
            raise ValueError("KalmanStore.%s: %d problems, one call takes %d" % (what, len(problems), _rounds_lib.MAX_BATCH))
        lists = []
        for k, p in enumerate(problems):
            if torch.is_tensor(p.slots):
                raise ValueError("KalmanStore.%s takes host slot lists (problem %d)" % (what, k))
            lists.append(_slots_checked(p.slots, self.capacity, "KalmanStore.%s: problem %d" % (what, k))[0])
        begin = np.zeros(len(problems) + 1, dtype=np.int32)
        begin[1:] = np.cumsum([len(s) for s in lists])
        slots = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32)
        if distinct and len(problems) > 1:
            live = slots[slots >= 0]
            if len(np.unique(live)) != len(live):
                raise ValueError("KalmanStore.%s: with predict the slots >= 0 must be distinct across the whole batch" % what)
        nt = None
        if any(p.not_tracked is not None for p in problems):
            nt = np.zeros(len(slots), dtype=np.uint8)
            for k, p in enumerate(problems):
                if p.not_tracked is not None:
                    flags = np.asarray(p.not_tracked, dtype=np.bool_).reshape(-1)
                    if len(flags) != len(lists[k]):
                        raise ValueError("KalmanStore.%s: problem %d has %d `not_tracked` flags for %d slots" % (what, k, len(flags), len(lists[k])))
                    nt[begin[k]:begin[k + 1]] = flags
        return problems, slots, begin, nt

    def _batch_upload(self, problems, slots, begin, nt):
        """The two uploads of a batch: the detections (detections_batch) and ONE int32 table - the slot list, the problem rows of busca_rounds_cost,
        the solver's dims, the status words (zero: a problem without detections has no tile to write them) and, packed four to a word, the
        `not_tracked` flags -> (views of the table: slot, rows, dims, status, flags or None; DeviceDetections; host dims int32 [B,2])."""
        det, dbegin = self.detections_batch([p.detections for p in problems], [p.det_scores for p in problems])
        B, n_total = len(problems), len(slots)
        sizes = [n_total, 4 * B, 2 * B, n_total, 0 if nt is None else (n_total + 3) // 4]
        host = np.zeros(sum(sizes), dtype=np.int32)
        host[:n_total] = slots
        rows, dims = host[n_total:n_total + 4 * B].reshape(B, 4), host[n_total + 4 * B:n_total + 6 * B].reshape(B, 2)
        rows[:, 0], rows[:, 2] = begin[:-1], dbegin[:-1]
        rows[:, 1] = dims[:, 0] = begin[1:] - begin[:-1]
        rows[:, 3] = dims[:, 1] = dbegin[1:] - dbegin[:-1]
        if nt is not None:
            host[n_total + 6 * B + n_total:].view(np.uint8)[:n_total] = nt
        views = list(small_to_dev(host, self.dev, torch.int32).split(sizes))
        views[4] = None if nt is None else views[4].view(torch.uint8)[:n_total]
        return views, det, dims

    def _batch_cost(self, views, det, dims, flags, lambda_):
        """busca_rounds_cost of an uploaded batch -> device float64 [B, N, M] (nothing is launched when every problem is empty)."""
        slot, rows, _, status, _ = views
        B, N, M = len(dims), int(dims[:, 0].max()), int(dims[:, 1].max())
        out = torch.empty(B, N, M, dtype=torch.float64, device=self.dev)
        if N == 0 or M == 0:
            return out
        self._state()
        _rounds_lib.check(_rounds_lib.load().busca_rounds_cost(
            self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, slot.data_ptr(), slot.numel(), det.tlbr.data_ptr(), det.xyah.data_ptr(),
            None if det.score is None else det.score.data_ptr(), det.m, rows.data_ptr(), B, N, M, flags, float(lambda_), out.data_ptr(),
            status.data_ptr(), *self._where()))
        return out

    def cost_batch(self, problems, fuse_motion=False, only_position=False, lambda_=0.98, gate_only=False):
        """cost() of every RoundProblem(slots, detections, det_scores) of a list in ONE launch, from the states as they are -> (device float64
        [B, N, M]: problem k's matrix is [k, :n_k, :m_k], the rest of the slab is not written; host int32 [B,2] of (n_k, m_k); device int32 [n_total]
        status words in the order of the concatenated slot lists).  N and M are the largest n_k and m_k.  Problems may share slots.  Two uploads:
        one int32 table, one float64 table of the detections."""
        problems, slots, begin, _ = self._batch_checked(problems, "cost_batch", False)
        if not problems:
            return torch.empty(0, 0, 0, dtype=torch.float64, device=self.dev), np.zeros((0, 2), dtype=np.int32), torch.empty(0, dtype=torch.int32, device=self.dev)
        views, det, dims = self._batch_upload(problems, slots, begin, None)
        return self._batch_cost(views, det, dims, self._flags(det, fuse_motion, only_position, gate_only), lambda_), dims, views[3]

    def round_batch(self, problems, thresh, fuse_motion=False, only_position=False, lambda_=0.98, predict=True):
        """round() of every RoundProblem(slots, detections, det_scores, not_tracked) of a list -> [(matches, u_track, u_detection)], each what
        round() returns for that problem alone.  Three launches whatever the number of problems - predict on the concatenated slot lists (unless
        `predict` is false), busca_rounds_cost, busca_linear_assignment over the batch - and ONE device->host copy of B * (N + M + 1) match words
        and n_total status words.  The sequences share this store: with `predict` the slots >= 0 must be distinct across the batch (ValueError).
        Raises LinAlgError naming the problem and its track where round() does, after the prediction of every listed track."""
        problems, slots, begin, nt = self._batch_checked(problems, "round_batch", predict)
        if not problems:
            return []
        views, det, dims = self._batch_upload(problems, slots, begin, nt if predict else None)
        flags = self._flags(det, fuse_motion, only_position, False) if det.m else 0
        if predict and len(slots):
            lib = self._state()
            _track_lib.check(lib.busca_track_kalman_predict(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, views[0].data_ptr(),
                                                            None if views[4] is None else views[4].data_ptr(), len(slots), *self._where()))
        B, N, M = len(dims), int(dims[:, 0].max()), int(dims[:, 1].max())
        if not (dims[:, 0] * dims[:, 1]).any():
            return [_empty_triple(int(n), int(m)) for n, m in dims]
        cost = self._batch_cost(views, det, dims, flags, lambda_)
        sol = _assign_dev(geometry.default_context(self.dev.index), cost, B, N, M, thresh, views[2])
        host = torch.cat([sol.view(-1), views[3]]).cpu().numpy()
        sol, status = host[:B * (N + M + 1)].reshape(B, N + M + 1).astype(np.int64), host[B * (N + M + 1):]
        for k in range(B):
            if dims[k, 0] and dims[k, 1]:
                _raise_flagged(status[begin[k]:begin[k + 1]], "KalmanStore.round_batch: problem %d" % k)
        return [_empty_triple(int(n), int(m)) if n == 0 or m == 0 else _triple(sol[k, :n], sol[k, N:N + m], sol[k, N + M], "KalmanStore.round_batch[%d]" % k)
                for k, (n, m) in enumerate(dims)]

    # ---- a whole frame as one chain (busca_frame.h, libbusca_frame.so; busca_assign_stages)
    def _frame_checked(self, pool_slots, lost, unconfirmed_slots, free_slots, detections, det_scores, track_thresh, low_thresh,
                       what="KalmanStore.frame"):
        """The host side of frame(), before anything is allocated -> (rows int32 [n]: pool then unconfirmed, n_pool, first, again, lost, free int32,
        scores float64 [m], classes uint8 [m], measurements [m,4], boxes [m,4]).  `what` names the call (and, from frame_batch, the problem)."""
        lists = []
        for name, x in (("pool_slots", pool_slots), ("unconfirmed_slots", unconfirmed_slots), ("free_slots", free_slots)):
            if torch.is_tensor(x):
                raise ValueError("%s takes host slot lists (%s)" % (what, name))
            lists.append(_slots_checked(x, self.capacity, "%s: %s" % (what, name))[0])
        pool, unconfirmed, free = lists
        if (free < 0).any():
            raise ValueError("%s: a free slot is negative" % what)
        rows = np.concatenate([pool, unconfirmed])
        live = rows[rows >= 0]
        if len(np.unique(live)) != len(live):
            raise ValueError("%s: the slots of pool_slots and unconfirmed_slots together must be distinct" % what)
        taken = np.intersect1d(live, free)
        if len(taken):
            raise ValueError("%s: free slot %d is also listed as a track's" % (what, int(taken[0])))
        xyah, tlbr = _frame_detections(detections)
        m = len(xyah)
        scores = _scores(det_scores, m)
        if len(rows) > _lib.ASSIGN_MAX or m > min(_lib.ASSIGN_MAX, _frame_lib.MAX_DETS):
            raise ValueError("%s: %d tracks and %d detections, the device solver takes at most %d rows and columns" % (what, len(rows), m, _lib.ASSIGN_MAX))
        first, again, lost = _frame_row_tables(lost, len(pool), len(unconfirmed))
        return rows, len(pool), first, again, lost, free, scores, _frame_classes(det_scores, track_thresh, low_thresh), xyah, tlbr

    def frame(self, pool_slots, lost, unconfirmed_slots, detections, det_scores, track_thresh, match_thresh, det_thresh, free_slots=(), mot20=False,
              low_thresh=0.1, second_thresh=0.5, unconfirmed_thresh=0.7, apply=True):
        """The Kalman side of one BYTETracker.update (adapters/ByteTrack/yolox/tracker/byte_tracker.py:244-249, 312-425) on resident state, as ONE
        chain on the stream: STrack.multi_predict of the pool, the cost slab of the three rounds (busca_frame_cost), the three rounds as one staged
        assignment (busca_assign_stages), and - unless `apply` is false - KalmanFilter.update of every matched track and KalmanFilter.initiate of
        every new track into a free slot (busca_frame_apply) -> ByteFrame.  Four launches, two uploads and ONE device->host copy of 3 n + 2 m + 1
        words whatever the track count; the host reads the matches after the filter has been enqueued, not before.
          pool_slots         joint_stracks(tracked_stracks, lost_stracks), in that order;  lost[i]: the state of pool track i is not Tracked
          unconfirmed_slots  the tracks with is_activated false: they are matched but, as in the reference, never predicted
          detections         ALL detections of the frame: objects with .tlwh and .tlbr, or a host [m,4] array of (x, y, a, h) measurements, whose
                             boxes then follow as STrack.tlbr derives them;  det_scores: their scores.  The rounds they belong to follow
                             from the scores as in the reference (_frame_classes): > track_thresh first round, between low_thresh and track_thresh
                             second round, the others - a score equal to track_thresh among them - none
          match_thresh, second_thresh, unconfirmed_thresh   the limits of the three rounds;  mot20: no fuse_score in rounds one and three
          det_thresh         an unmatched first-round detection starts a track unless its score is below this
          free_slots         where new tracks go, in the order of their detections; disjoint from the listed tracks (ValueError otherwise).  A
                             detection that finds none left is listed in ByteFrame.overflow and nothing is written for it
        Rounds 1 and 3 read plane 0 of the slab, round 2 plane 1; a detection is kept out of a round by +inf in that round's plane, which to the
        solver is a column that is not there.  Step 3b of the reference (the BUSCA round) matches tracks to their own Kalman candidates and takes no
        detection away, so it commutes with the round of the unconfirmed tracks: it works on ByteFrame.unmatched_pool afterwards.
        Raises LinAlgError where an update finds a projected covariance that is not positive definite (that track keeps its state, the others are
        updated) and BuscaError on a solver status.  Without detections only the prediction happens and nothing is copied."""
        rows, n_pool, first, again, lost, free, scores, cls, xyah, tlbr = self._frame_checked(pool_slots, lost, unconfirmed_slots, free_slots, detections,
                                                                                  det_scores, track_thresh, low_thresh)
        n, m, n_free = len(rows), len(xyah), len(free)
        # one pinned upload of every small table: the 16-byte stage records first, then the int32 tables, then the `lost` bytes
        ints = np.concatenate([rows, first, again, free]).astype(np.int32)
        flags = np.zeros(-(-n_pool // 4) * 4, dtype=np.uint8)
        flags[:n_pool] = lost
        up = h2d_async(np.concatenate([_stage_records(match_thresh, second_thresh, unconfirmed_thresh), ints.view(np.uint8), flags]), self.dev)
        at = 16 * FRAME_STAGES
        words = up[at:at + 4 * len(ints)].view(torch.int32)
        d_slot, d_first, d_again, d_free = words[:n], words[n:2 * n], words[2 * n:3 * n], words[3 * n:]
        d_lost = up[at + 4 * len(ints):]
        lib = self._state()
        where = self._where()
        if n_pool:
            _track_lib.check(lib.busca_track_kalman_predict(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), d_lost.data_ptr(),
                                                            n_pool, *where))

        if m == 0:
            none = -np.ones(n, dtype=np.int64)
            return _byte_frame(none, none, none[:0], n_pool, lost, cls)
        # one upload of the detection table: measurements, boxes, scores, and the class bytes behind them
        tail = np.zeros(-(-m // 8) * 8, dtype=np.uint8)
        tail[:m] = cls
        table = small_to_dev(np.concatenate([xyah.reshape(-1), tlbr.reshape(-1), scores, tail.view(np.float64)]),
                             self.dev, torch.float64)
        d_xyah, d_tlbr, d_score, d_cls = table[:4 * m], table[4 * m:8 * m], table[8 * m:9 * m], table[9 * m:].view(torch.uint8)
        solved = 2 * n + m + 1                                                 # row_to_col | col_to_row | row_stage | solver status
        out = torch.empty(solved + n + m, dtype=torch.int32, device=self.dev)  # ... | update status [n] | new_slot [m]: one copy
        slab = torch.empty(1, 2, n, m, dtype=torch.float64, device=self.dev)
        flib = _frame_lib.load()
        if n:
            _frame_lib.check(flib.busca_frame_cost(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n, d_tlbr.data_ptr(),
                                                   None if mot20 else d_score.data_ptr(), d_cls.data_ptr(), m, slab.data_ptr(),
                                                   out.data_ptr() + 4 * solved, *where))
        _assign_stages_dev(geometry.default_context(self.dev.index), slab, up[:at], d_first, d_again, None, into=out)
        if apply:
            base = out.data_ptr()
            _frame_lib.check(flib.busca_frame_apply(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr() if n else None, n,
                                                    base if n else None, base + 4 * n, d_xyah.data_ptr(), d_score.data_ptr(), d_cls.data_ptr(), m,
                                                    float(det_thresh), d_free.data_ptr() if n_free else None, n_free, base + 4 * (solved + n),
                                                    base + 4 * solved if n else None, *where))
        host = (out if apply else out[:solved + n]).cpu().numpy()              # the one device->host copy
        if host[solved - 1] != 0:
            raise _lib.BuscaError("KalmanStore.frame: the solver ran out of its loop bounds (status %d) - is a cost -inf or a limit infinite?"
                                  % int(host[solved - 1]))
        _raise_flagged(host[solved:solved + n], "KalmanStore.frame")
        new = host[solved + n:] if apply else np.full(m, -1, dtype=np.int32)
        return _byte_frame(host[:n], host[n + m:2 * n + m], new, n_pool, lost, cls)

    # ---- the frames of many sequences as one chain (busca_mframe.h, libbusca_mframe.so; busca_assign_stages over the batch)
    def _frame_batch_checked(self, problems, track_thresh, low_thresh):
        """The host side of frame_batch(), before anything is allocated -> [what _frame_checked returns, per problem]."""
        what = "KalmanStore.frame_batch"
        problems = [p if isinstance(p, FrameProblem) else FrameProblem(*p) for p in problems]
        if len(problems) > _mframe_lib.MAX_BATCH:
            raise ValueError("%s: %d problems, one call takes %d" % (what, len(problems), _mframe_lib.MAX_BATCH))
        checked = []
        for k, p in enumerate(problems):
            name = "%s: problem %d" % (what, k)
            try:
                checked.append(self._frame_checked(p.pool_slots, p.lost, p.unconfirmed_slots, p.free_slots, p.detections, p.det_scores, track_thresh,
                                                   low_thresh, what=name))
            except ValueError as e:
                if name in str(e):
                    raise
                raise ValueError("%s: %s" % (name, e)) from None
        if len(checked) > 1:                                                   # one launch serves them all: what two problems share, two workgroups race on
            rows = np.concatenate([c[0] for c in checked])
            taken = np.concatenate([rows[rows >= 0]] + [c[5] for c in checked])
            if len(np.unique(taken)) != len(taken):
                slots, count = np.unique(taken, return_counts=True)
                raise ValueError("%s: the tracks and the free slots must be distinct across the whole batch (slot %d is listed twice)"
                                 % (what, int(slots[count > 1][0])))
        return checked

    def frame_batch(self, problems, track_thresh, match_thresh, det_thresh, mot20=False, low_thresh=0.1, second_thresh=0.5, unconfirmed_thresh=0.7,
                    apply=True):
        """frame() of every FrameProblem(pool_slots, lost, unconfirmed_slots, detections, det_scores, free_slots) of a list - the frames of one time
        step of many sequences that share this store - as ONE chain on the stream -> [ByteFrame], each what frame() returns for that problem alone,
        the states bit for bit what the frames one after the other leave.  Whatever the number of problems: one pinned upload of every small table,
        one float64 upload of the concatenated detection table, STrack.multi_predict over all pool rows (busca_track_kalman_predict; the
        unconfirmed rows stand as -1 in its list), busca_mframe_cost, busca_assign_stages over the batch with its `dims`, busca_mframe_apply, and
        ONE device->host copy of B (3 N + 2 M + 1) words, N and M the largest row and detection counts; the host reads the matches after the filter
        has been enqueued.  The thresholds and `mot20` are the batch's, as the solver's stage table is; the rounds of the detections follow from
        each problem's scores.  The tracks and the free slots must be distinct across the whole batch (ValueError, before anything is allocated).
        An empty list gives []; without any detection only the prediction happens and nothing is copied.  Raises BuscaError on a solver status and
        LinAlgError where an update finds a projected covariance that is not positive definite, naming the problem (and the track), after the
        whole batch has been applied.  For a single sequence frame() is the shorter route."""
        checked = self._frame_batch_checked(problems, track_thresh, low_thresh)
        B = len(checked)
        if B == 0:
            return []
        W = _mframe_lib.PROBLEM_WORDS
        n_k, m_k, f_k = ([len(c[i]) for c in checked] for i in (0, 8, 5))
        N, M = max(n_k), max(m_k)
        n_total, m_total, f_total = sum(n_k), sum(m_k), sum(f_k)
        table = np.zeros((B, W), dtype=np.int32)                               # row_begin, n_k, det_begin, m_k, free_begin, n_free_k
        table[:, 1], table[:, 3], table[:, 5] = n_k, m_k, f_k
        table[1:, 0::2] = np.cumsum(table[:-1, 1::2], axis=0)
        first, again = (np.full((B, N), -1, dtype=np.int32) for _ in range(2))
        predict, flags = np.full(n_total, -1, dtype=np.int32), np.zeros(-(-n_total // 4) * 4, dtype=np.uint8)
        for k, (rows, n_pool, fst, agn, lost) in enumerate(c[:5] for c in checked):
            first[k, :n_k[k]], again[k, :n_k[k]] = fst, agn
            at = table[k, 0]
            predict[at:at + n_pool], flags[at:at + n_pool] = rows[:n_pool], lost      # the unconfirmed rows are matched but never predicted: -1
        # one pinned upload of every small table: the 16-byte stage records first, then the int32 tables, then the `lost` bytes
        parts = [np.concatenate([c[0] for c in checked]), predict, table.reshape(-1), table[:, 1::2][:, :2].reshape(-1), first.reshape(-1),
                 again.reshape(-1), np.concatenate([c[5] for c in checked])]
        ints = np.concatenate(parts).astype(np.int32)
        up = h2d_async(np.concatenate([_stage_records(match_thresh, second_thresh, unconfirmed_thresh), ints.view(np.uint8), flags]), self.dev)
        at = 16 * FRAME_STAGES
        d_slot, d_predict, d_table, d_dims, d_first, d_again, d_free = up[at:at + 4 * len(ints)].view(torch.int32).split([len(p) for p in parts])
        d_lost = up[at + 4 * len(ints):]
        lib = self._state()
        where = self._where()
        if any(c[1] for c in checked):
            _track_lib.check(lib.busca_track_kalman_predict(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_predict.data_ptr(),
                                                            d_lost.data_ptr(), n_total, *where))
        none = -np.ones(N, dtype=np.int64)
        if M == 0:
            return [_byte_frame(none[:n], none[:n], none[:0], c[1], c[4], c[7]) for n, c in zip(n_k, checked)]
        # one upload of the detection table: measurements, boxes, scores, and the class bytes behind them
        tail = np.zeros(-(-m_total // 8) * 8, dtype=np.uint8)
        tail[:m_total] = np.concatenate([c[7] for c in checked])
        dets = small_to_dev(np.concatenate([c[8].reshape(-1) for c in checked] + [c[9].reshape(-1) for c in checked] + [c[6] for c in checked]
                                           + [tail.view(np.float64)]), self.dev, torch.float64)
        d_xyah, d_tlbr, d_score, d_cls = dets[:4 * m_total], dets[4 * m_total:8 * m_total], dets[8 * m_total:9 * m_total], dets[9 * m_total:].view(torch.uint8)
        solved = B * (2 * N + M + 1)                                           # row_to_col [B,N] | col_to_row [B,M] | row_stage [B,N] | solver status [B]
        out = torch.empty(solved + B * (N + M), dtype=torch.int32, device=self.dev)      # ... | update status [B,N] | new_slot [B,M]: one copy
        slab = torch.empty(B, 2, N, M, dtype=torch.float64, device=self.dev)
        mlib = _mframe_lib.load()
        base = out.data_ptr()
        if N:
            _mframe_lib.check(mlib.busca_mframe_cost(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr(), n_total, d_tlbr.data_ptr(),
                                                     None if mot20 else d_score.data_ptr(), d_cls.data_ptr(), m_total, f_total, d_table.data_ptr(), B, N, M,
                                                     slab.data_ptr(), base + 4 * solved, *where))
        _assign_stages_dev(geometry.default_context(self.dev.index), slab, up[:at], d_first, d_again, d_dims, into=out)
        if apply:
            _mframe_lib.check(mlib.busca_mframe_apply(self.mean.data_ptr(), self.cov.data_ptr(), self.capacity, d_slot.data_ptr() if n_total else None,
                                                      n_total, base if N else None, base + 4 * B * N, d_xyah.data_ptr(), d_score.data_ptr(),
                                                      d_cls.data_ptr(), m_total, float(det_thresh), d_free.data_ptr() if f_total else None, f_total,
                                                      d_table.data_ptr(), B, N, M, base + 4 * (solved + B * N), base + 4 * solved if N else None, *where))
        host = (out if apply else out[:solved]).cpu().numpy()                  # the one device->host copy
        # the words of problem k are the corner (n_k, m_k) of its blocks: the kernels write nothing else, and nothing else is read
        r2c, _, stage, status = np.split(host[:solved], [B * N, B * (N + M), B * (2 * N + M)])
        r2c, stage = r2c.reshape(B, N), stage.reshape(B, N)
        for k in range(B):
            if status[k] != 0:
                raise _lib.BuscaError("KalmanStore.frame_batch: problem %d: the solver ran out of its loop bounds (status %d) - is a cost -inf or a limit "
                                      "infinite?" % (k, int(status[k])))
        frames = []
        if apply:
            flagged, new = host[solved:solved + B * N].reshape(B, N), host[solved + B * N:].reshape(B, M)
            for k in range(B):
                _raise_flagged(flagged[k, :n_k[k]], "KalmanStore.frame_batch: problem %d" % k)
        for k, c in enumerate(checked):
            started = new[k, :m_k[k]] if apply else np.full(m_k[k], -1, dtype=np.int32)
            frames.append(_byte_frame(r2c[k, :n_k[k]], stage[k, :n_k[k]], started, c[1], c[4], c[7]))
        return frames

    # ---- objects in and out
    def _rows(self, slots, stracks, what):
        slot, n = _slots_checked(slots, self.capacity, "KalmanStore." + what)
        if torch.is_tensor(slot):
            raise ValueError("KalmanStore.%s takes a host slot list" % what)
        if n != len(stracks):
            raise ValueError("KalmanStore.%s: %d slots for %d tracks" % (what, n, len(stracks)))
        return np.where(slot < 0, self.capacity, slot).astype(np.int64), n      # negative entries: the spare slot

    def load(self, slots, stracks):
        """The states of objects with `.mean` [8] / `.covariance` [8,8] into their slots (one upload)."""
        rows, n = self._rows(slots, stracks, "load")
        if n == 0:
            return
        self._state()
        table = np.concatenate([np.asarray([st.mean for st in stracks], dtype=np.float64).reshape(-1),
                                np.asarray([st.covariance for st in stracks], dtype=np.float64).reshape(-1)])
        table = small_to_dev(table, self.dev, torch.float64)
        rows = small_to_dev(rows, self.dev, torch.int64)
        self.mean.index_copy_(0, rows, table[:8 * n].view(n, 8))
        self.cov.index_copy_(0, rows, table[8 * n:].view(n, 8, 8))

    def store(self, slots, stracks):
        """The states of the listed slots into the objects' `.mean` / `.covariance` (one device->host copy)."""
        rows, n = self._rows(slots, stracks, "store")
        if n == 0:
            return
        self._state()
        rows = small_to_dev(rows, self.dev, torch.int64)
        _set_states(stracks, torch.cat([self.mean.index_select(0, rows).view(-1), self.cov.index_select(0, rows).view(-1)]).cpu().numpy())
