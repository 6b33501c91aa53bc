"""GHOST's linear motion model with its state on the device: position rings, the velocity step, the camera-motion warp of stored boxes and the
IoU motion cost.  Fronts include/busca_ghost_motion.h; restates BaseTracker.motion / get_motion_dist / motion_compensation's loop
(adapters/GHOST/src/base_tracker.py:600-712) and Track.add_detection's bookkeeping (adapters/GHOST/src/tracking_utils.py)."""
import numpy as np
import torch

from . import _lib, geometry
from ._xfer import small_to_dev, stream_of, to_dev


def ghost_motion_check_config(motion_cfg, kalman=False):
    """Refuse the motion_config branches (and the Kalman route, tracker_cfg['kalman']) that crash in the reference; returns motion_cfg."""
    if kalman:
        raise ValueError("GHOST's Kalman motion route is refused: the reference calls self.motion(only_vel=True) (tracker.py:381), a parameter "
                         "BaseTracker.motion does not have (TypeError), and src.kalman is not part of the reference tree")
    if motion_cfg.get("center_only", False):
        raise ValueError("GHOST motion_config center_only is refused: the reference crashes in this branch (get_width(track.pos) indexes pos[0, 2] "
                         "on a one-dimensional box: IndexError, base_tracker.py:678-682), so there is nothing to reproduce")
    if motion_cfg.get("approximate", False):
        raise ValueError("GHOST motion(approximate=True) is refused: the reference crashes in this branch (vs is a Python list there and has no "
                         ".mean: AttributeError, base_tracker.py:684-692), so there is nothing to reproduce")
    return motion_cfg


def _slots_checked(slots, capacity, what):
    """A slot list -> (device-ready int32 array or tensor, n).  Host lists are checked here: the entries >= 0 distinct and below `capacity` (negative
    entries are skipped by the kernels); a device tensor is the caller's."""
    if torch.is_tensor(slots):
        return slots, int(slots.numel())
    slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int64).reshape(-1))
    live = slots[slots >= 0]
    if len(live) and int(live.max()) >= capacity:
        raise ValueError("%s: slot %d is beyond the capacity of %d" % (what, int(live.max()), capacity))
    if len(np.unique(live)) != len(live):
        raise ValueError("%s: the slots of one call must be distinct" % what)
    return slots.astype(np.int32), len(slots)


class GhostMotion:
    """The state of GHOST's linear motion model on the device (busca_ghost_motion_*): for `capacity` track slots a ring of the newest `history`
    boxes with their frame numbers (Track.last_pos / past_frames), the current position (Track.pos) and the last velocity (Track.last_v).
      add(slots, boxes, frame)       Track.__init__ / add_detection: pos = box, the box joins the history
      compensate(warp)               motion_compensation's loop: every stored box through warp_pos (pos itself stays, as in the reference)
      step(slots, num_active, n)     BaseTracker.motion(): velocities of the active tracks from their last n positions, pos += v for all
      cost(slots, num_active, dets, n)   step, then get_motion_dist: 1 - IoU, tracks x detections
    The reference keeps the whole history; this keeps `history` rows, which is the same for last_n_frames <= history or tracks no longer than that.
    `box_dtype`: the dtype of the reference's detection boxes.  numpy subtracts two stored positions in float32 when every row of a track's window
    is a float32 array and in float64 otherwise, and every row is float32 once motion compensation has warped it.  One host flag follows that rule
    for all tracks together: the difference is float32 when box_dtype is float32, or when no add() came since the last compensate() of all slots -
    the reference's order within a frame (compensate, step, add).  A step between an add() and the next compensate() of a moving-camera sequence
    takes float64 differences for every track, also those whose rows are all warped.
    Slot lists given as host lists or arrays are checked on the host - the entries >= 0 distinct and below `capacity`, ValueError otherwise.  A slot
    list given as a device tensor is not read back: it is the caller's to keep distinct (duplicates race on that slot, entries outside the capacity
    are skipped by the kernels and touch no memory).  ghost_round hands its own device slot list through when state.slot is None or a tensor."""

    def __init__(self, capacity, history, box_dtype=np.float64, ctx=None):
        capacity, history = int(capacity), int(history)
        if capacity < 0 or history < 2:
            raise ValueError("GhostMotion(capacity=%d, history=%d): a ring needs at least 2 rows" % (capacity, history))
        if np.dtype(box_dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("box_dtype must be float32 or float64, not %r" % (box_dtype,))
        self.ctx, self.dev = geometry.ctx_dev(ctx)
        self.capacity, self.history, self.box32 = capacity, history, np.dtype(box_dtype) == np.dtype(np.float32)
        self.hist = torch.zeros(capacity, history, 4, dtype=torch.float64, device=self.dev)
        self.frames = torch.zeros(capacity, history, dtype=torch.int32, device=self.dev)
        self.count = torch.zeros(capacity, dtype=torch.int32, device=self.dev)
        self.newest = torch.zeros(capacity, dtype=torch.int32, device=self.dev)
        self.pos = torch.zeros(capacity, 4, dtype=torch.float64, device=self.dev)
        self.vel = torch.zeros(capacity, 4, dtype=torch.float64, device=self.dev)
        self.all_warped = False                                   # no add() since the last compensate() of all slots

    @property
    def diff32(self):
        return self.box32 or self.all_warped

    def add(self, slots, boxes, frame, det_index=None, new=None):
        """Detection det_index[i] (None: i) of `boxes` [m,4] tlbr (host array or device tensor) becomes the position of slot slots[i] and joins its
        history with frame number `frame`; new[i] true starts a new track in that slot (history emptied, velocity zero).  Host boxes are rounded to
        `box_dtype` first, as the reference's arrays are; a device tensor is taken as float64 values."""
        slot, k = _slots_checked(slots, self.capacity, "GhostMotion.add")
        if not torch.is_tensor(boxes):
            boxes = np.asarray(boxes, dtype=np.float32 if self.box32 else np.float64).astype(np.float64).reshape(-1, 4)
        boxes = to_dev(boxes, self.dev, torch.float64).view(-1, 4)
        m = boxes.shape[0]
        det = small_to_dev(det_index if det_index is None or torch.is_tensor(det_index) else np.asarray(det_index, dtype=np.int32), self.dev, torch.int32)
        if det is None and k > m:
            raise ValueError("GhostMotion.add: %d slots for %d boxes" % (k, m))
        if det is not None and det.numel() != k:
            raise ValueError("GhostMotion.add: %d detection indices for %d slots" % (det.numel(), k))
        reset = None
        if new is not None:
            reset = small_to_dev(new if torch.is_tensor(new) else np.asarray(new, dtype=np.bool_).astype(np.uint8), self.dev, torch.uint8)
            if reset.numel() != k:
                raise ValueError("GhostMotion.add: %d `new` flags for %d slots" % (reset.numel(), k))
        slot = small_to_dev(slot, self.dev, torch.int32)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_append(c.h, self.hist.data_ptr(), self.frames.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(),
                                                self.pos.data_ptr(), self.vel.data_ptr(), self.capacity, self.history, slot.data_ptr(), _lib.ptr(det),
                                                _lib.ptr(reset), k, boxes.data_ptr(), m, int(frame), stream_of(self.dev)))
        if k:
            self.all_warped = False

    def compensate(self, warp, slots=None):
        """Every stored box of `slots` (None: all) through the [2,3] warp (host float32), as motion_compensation does for every track."""
        warp = np.ascontiguousarray(np.asarray(warp, dtype=np.float32).reshape(6))
        slot, n = (None, 0) if slots is None else _slots_checked(slots, self.capacity, "GhostMotion.compensate")
        slot = small_to_dev(slot, self.dev, torch.int32)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_warp(c.h, self.hist.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(), self.capacity, self.history,
                                              _lib.ptr(slot), n, warp.ctypes.data, stream_of(self.dev)))
        if slots is None:
            self.all_warped = True

    def step(self, slots, num_active, last_n_frames):
        """One motion() step for the tracks in `slots`, ACTIVE TRACKS FIRST (`num_active` of them) -> device float64 [n,4], their positions in
        list order (a negative slot: a row of NaN).  It advances pos: once per frame, as the reference calls motion()."""
        slot, n = _slots_checked(slots, self.capacity, "GhostMotion.step")
        slot = small_to_dev(slot, self.dev, torch.int32)
        out = torch.empty(n, 4, dtype=torch.float64, device=self.dev)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_step(c.h, self.hist.data_ptr(), self.frames.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(),
                                              self.pos.data_ptr(), self.vel.data_ptr(), self.capacity, self.history, slot.data_ptr(), n, int(num_active),
                                              min(int(last_n_frames), 2 ** 31 - 1), int(self.diff32), out.data_ptr(), stream_of(self.dev)))
        return out

    def cost(self, slots, num_active, det_boxes, last_n_frames):
        """step(), then get_motion_dist: 1 - IoU ("+1" pixel convention) of the stepped positions and `det_boxes` [m,4] -> device float64 [n,m],
        tracks x detections (the reference's matrix transposed): the `motion` operand of ghost_cost / ghost_round."""
        pos = self.step(slots, num_active, last_n_frames)
        if not torch.is_tensor(det_boxes):
            det_boxes = np.array(det_boxes, dtype=np.float64).reshape(-1, 4)
        return geometry.pairwise(self.ctx, pos, det_boxes, _lib.PAIR_IOU_COST)
