"""GHOST's appearance state on the device: per track slot a ring of the newest features and the moving-average proxy, kept where ghost_round reads
them.  Fronts no header: ring writes are device tensor ops on torch's current stream, the reads are busca_ghost_proxies / busca_ghost_distance
(include/busca_ghost.h) through ghost_round.  Restates Track.__init__ / add_detection's feature bookkeeping
(adapters/GHOST/src/tracking_utils.py:286-289, 342-343) and the reset of tracks beyond their patience (adapters/GHOST/src/tracker.py:252-255)."""
import numpy as np
import torch

from . import geometry
from ._xfer import small_to_dev, to_dev
from .ghost_motion import _slots_checked


def _ring_append(gallery, count, newest, seen, slot, rows, new):
    """The ring rule on tensors that carry one spare slot behind the last: rows[i] becomes the newest sample of slot[i] (int64; negative entries
    go to the spare slot, whose contents mean nothing).  new[i] (bool or None) empties the slot first.  No synchronising call."""
    spare, budget = gallery.shape[0] - 1, gallery.shape[1]
    s = torch.where(slot < 0, spare, slot)
    c = count[s]
    if new is not None:
        c = torch.where(new, torch.zeros_like(c), c)
        seen[s] = torch.where(new, torch.zeros_like(seen[s]), seen[s])
    row = torch.where(c == 0, torch.zeros_like(c), (newest[s] + 1) % budget)
    gallery[s, row.long()] = rows
    newest[s] = row
    count[s] = torch.clamp(c + 1, max=budget)


class GhostGallery:
    """The feature side of GHOST's Track on the device, for `capacity` track slots: a ring of the newest `budget` features (Track.past_feats), how
    many are stored and where the newest is, and the moving average get_proxy's 'mv_avg' keeps per track (Tracker.mv_avg).
      add(slots, feats)          Track.__init__ / add_detection: the feature joins the slot's ring as its newest sample
      release(slots)             the track is gone (or beyond patience + 5, where the reference empties past_feats): the slot can be reused
      state(active, inactive)    the dict ghost_round takes, ACTIVE TRACKS FIRST
    gallery [capacity,budget,E] float32, count / newest [capacity] int32, mv_avg [capacity,E] float32, mv_seen [capacity] uint8 are device tensors
    (views of storage with one spare slot behind the last, where the writes of skipped entries land).  The ring row of a new sample is 0 for an
    empty slot, else (newest + 1) % budget; count = min(count + 1, budget).  Features are stored as given: GHOST does not normalise them.
    The reference keeps every sample; this keeps `budget` rows, which is the same for windows num <= budget or tracks no longer than that; 'first'
    means the oldest sample still stored.  A GhostMotion of the same capacity shares the slots: state(..., motion=) hands it to ghost_round.
    Slot lists given as host lists or arrays are checked on the host - the entries >= 0 distinct and below `capacity`, ValueError otherwise,
    negative entries skipped.  A slot list given as a device tensor is not read back: it is the caller's to keep distinct and below `capacity`
    (negative entries are skipped).  Everything is ordered on torch's current stream; with all operands on the device no call synchronises."""

    def __init__(self, capacity, budget, E, ctx=None):
        capacity, budget, E = int(capacity), int(budget), int(E)
        if capacity < 0 or budget < 1 or E < 1:
            raise ValueError("GhostGallery(capacity=%d, budget=%d, E=%d): a ring needs at least 1 row of at least 1 value" % (capacity, budget, E))
        self.ctx, self.dev = geometry.ctx_dev(ctx)
        self.capacity, self.budget, self.E = capacity, budget, E
        self._gallery = torch.zeros(capacity + 1, budget, E, dtype=torch.float32, device=self.dev)
        self._count = torch.zeros(capacity + 1, dtype=torch.int32, device=self.dev)
        self._newest = torch.zeros(capacity + 1, dtype=torch.int32, device=self.dev)
        self._mv_avg = torch.zeros(capacity + 1, E, dtype=torch.float32, device=self.dev)
        self._mv_seen = torch.zeros(capacity + 1, dtype=torch.uint8, device=self.dev)
        self.gallery, self.count, self.newest = self._gallery[:capacity], self._count[:capacity], self._newest[:capacity]
        self.mv_avg, self.mv_seen = self._mv_avg[:capacity], self._mv_seen[:capacity]

    def _tables(self, what, k, **cols):
        """The index / flag vectors of one call (each None, a host sequence or a device tensor, `k` entries) as device int64 tensors: the host
        ones travel together, in one upload."""
        out, host = {}, {}
        for name, v in cols.items():
            if v is None:
                out[name] = None
                continue
            if not torch.is_tensor(v):
                v = np.asarray(v).reshape(-1)
                host[name] = v = (v != 0).astype(np.int32) if name == "new" else v.astype(np.int32)
            if (v.numel() if torch.is_tensor(v) else len(v)) != k:
                raise ValueError("%s: %d entries of `%s` for %d slots" % (what, v.numel() if torch.is_tensor(v) else len(v), name, k))
            if torch.is_tensor(v):
                out[name] = v.to(self.dev).view(-1).long()
        if host and k:
            up =small_to_dev(np.stack(list(host.values())), self.dev, torch.int32).view(len(host), k).long()
            out.update({name: up[i] for i, name in enumerate(host)})
        return out

    def add(self, slots, feats, det_index=None, new=None):
        """Row det_index[i] (None: i) of `feats` [m,E] (host array, or device float32 tensor read in place: the ReID output) becomes the newest
        sample of slot slots[i]; new[i] true starts a new track in that slot first (ring emptied, mv_avg forgotten)."""
        slots, k = _slots_checked(slots, self.capacity, "GhostGallery.add")
        feats = to_dev(feats, self.dev, torch.float32)
        if feats.dim() != 2 or feats.shape[1] != self.E:
            raise ValueError("GhostGallery.add takes [m,%d] features, not %s" % (self.E, tuple(feats.shape)))
        if det_index is None and k > feats.shape[0]:
            raise ValueError("GhostGallery.add: %d slots for %d features" % (k, feats.shape[0]))
        t = self._tables("GhostGallery.add", k, slots=slots, det_index=det_index, new=new)
        if k == 0:
            return
        rows = feats[:k] if t["det_index"] is None else feats.index_select(0, t["det_index"])
        _ring_append(self._gallery, self._count, self._newest, self._mv_seen, t["slots"], rows, None if t["new"] is None else t["new"] != 0)

    def release(self, slots):
        """The tracks in `slots` are gone: count = 0 and mv_seen = 0, so the slot reads as empty and can be given to a new track."""
        slots, k = _slots_checked(slots, self.capacity, "GhostGallery.release")
        if k == 0:
            return
        s = self._tables("GhostGallery.release", k, slots=slots)["slots"]
        s = torch.where(s < 0, self.capacity, s)
        self._count.index_fill_(0, s, 0)
        self._mv_seen.index_fill_(0, s, 0)

    def state(self, active, inactive=(), motion=None):
        """The `state` of ghost_round for the tracks in the slots `active` followed by those in `inactive`: the tables themselves (not copies - the
        'mv_avg' proxy updates them), `slot` as one device int32 vector, `num_active`, and `motion_state` = `motion`, a GhostMotion on the same slots."""
        parts = [active, inactive]
        if motion is not None and getattr(motion, "capacity", self.capacity) != self.capacity:
            raise ValueError("GhostGallery.state: the GhostMotion has %d slots, the gallery %d: they share their slots" % (motion.capacity, self.capacity))
        if any(torch.is_tensor(p) for p in parts):
            slot = torch.cat([(p if torch.is_tensor(p) else torch.from_numpy(np.asarray(p, dtype=np.int32).reshape(-1))).to(self.dev).view(-1).to(torch.int32)
                              for p in parts])
            na = int(parts[0].numel()) if torch.is_tensor(parts[0]) else len(parts[0])
        else:
            a, b = (np.asarray(p, dtype=np.int64).reshape(-1) for p in parts)
            host, _ = _slots_checked(np.concatenate([a, b]), self.capacity, "GhostGallery.state")
            slot, na = small_to_dev(host, self.dev, torch.int32), len(a)
        return dict(gallery=self.gallery, count=self.count, newest=self.newest, slot=slot, num_active=na, mv_avg=self.mv_avg, mv_seen=self.mv_seen,
                    motion_state=motion)
