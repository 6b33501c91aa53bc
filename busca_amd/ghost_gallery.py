"""GHOST's appearance state on the device: per track slot a ring of the newest features and the moving-average proxy, kept where ghost_round reads
them.  Fronts include/busca_store.h (libbusca_store.so, bound by _store_lib): a ring write is one busca_store_ring_add launch, a release one
busca_store_release launch, on torch's current stream; the reads are busca_ghost_proxies / busca_ghost_distance (include/busca_ghost.h) and
busca_store_mv_avg through ghost_round.  Restates Track.__init__ / add_detection's feature bookkeeping
(adapters/GHOST/src/tracking_utils.py:286-289, 342-343) and the reset of tracks beyond their patience (adapters/GHOST/src/tracker.py:252-255)."""
import numpy as np
import torch

from . import _store_lib, geometry
from ._lib import ptr
from ._xfer import h2d_async, small_to_dev, stream_of, to_dev
from .ghost_motion import _slots_checked

_FLAG_DTYPES = (torch.uint8, torch.bool)


class GhostGallery:
    """The feature side of GHOST's Track on the device, for `capacity` track slots: a ring of the newest `budget` features (Track.past_feats), how
    many are stored and where the newest is, and the moving average get_proxy's 'mv_avg' keeps per track (Tracker.mv_avg).
      add(slots, feats)          Track.__init__ / add_detection: the feature joins the slot's ring as its newest sample
      release(slots)             the track is gone (or beyond patience + 5, where the reference empties past_feats): the slot can be reused
      state(active, inactive)    the dict ghost_round takes, ACTIVE TRACKS FIRST
    gallery [capacity,budget,E] float32, count / newest [capacity] int32, mv_avg [capacity,E] float32, mv_seen [capacity] uint8 are device tensors
    (views of storage with one spare slot behind the last, which no kernel is told of or writes: a skipped entry touches no memory).  The ring row
    of a new sample is 0 for an empty slot, else (newest + 1) % budget; count = min(count + 1, budget).  Features are stored as given: GHOST does
    not normalise them.
    The reference keeps every sample; this keeps `budget` rows, which is the same for windows num <= budget or tracks no longer than that; 'first'
    means the oldest sample still stored.  A GhostMotion of the same capacity shares the slots: state(..., motion=) hands it to ghost_round.
    Slot lists given as host lists or arrays are checked on the host - the entries >= 0 distinct and below `capacity`, ValueError otherwise,
    negative entries skipped.  A slot list given as a device tensor is not read back: it is the caller's to keep distinct (entries that are
    negative or beyond `capacity` are skipped).  Device operands that already are int32 (slots, det_index) or uint8 / bool (new) are read in place,
    other dtypes converted with one tensor op; host lists travel together in one pinned upload.  add and release are one kernel launch each,
    ordered on torch's current stream; with all operands on the device no call synchronises."""

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
        """The index / flag vectors of one call (each None, a host sequence or a device tensor, `k` entries) as contiguous device tensors, int32 or
        for `new` uint8 / bool: a device tensor of that kind is used as it is, the host ones travel together, in one upload."""
        out, host = {}, {}
        for name, v in cols.items():
            if v is None:
                out[name] = None
                continue
            flag = name == "new"
            if not torch.is_tensor(v):
                v = np.asarray(v).reshape(-1)
                host[name] = v = (v != 0).astype(np.uint8) if flag else v.astype(np.int32)
            if (v.numel() if torch.is_tensor(v) else len(v)) != k:
                raise ValueError("%s: %d entries of `%s` for %d slots" % (what, v.numel() if torch.is_tensor(v) else len(v), name, k))
            if torch.is_tensor(v):
                if flag and v.dtype not in _FLAG_DTYPES:
                    v = v != 0
                if not (v.device == self.dev and v.is_contiguous() and v.dtype in (_FLAG_DTYPES if flag else (torch.int32,))):
                    v = v.to(device=self.dev, dtype=v.dtype if flag else torch.int32).contiguous()
                out[name] = v
        if host and k:
            names = sorted(host, key=lambda name: name == "new")                 # the int32 columns first: each starts on a multiple of 4 bytes
            up, lo = h2d_async(np.concatenate([host[name].view(np.uint8) for name in names]), self.dev), 0
            for name in names:
                out[name] = up[lo:lo + host[name].nbytes].view(torch.uint8 if name == "new" else torch.int32)
                lo += host[name].nbytes
        return out

    def add(self, slots, feats, det_index=None, new=None):
        """Row det_index[i] (None: i) of `feats` [m,E] (host array, or device float32 tensor read in place: the ReID output) becomes the newest
        sample of slot slots[i]; new[i] true starts a new track in that slot first (ring emptied, mv_avg forgotten).  One busca_store_ring_add."""
        slots, k = _slots_checked(slots, self.capacity, "GhostGallery.add")
        feats = to_dev(feats, self.dev, torch.float32)
        if feats.dim() != 2 or feats.shape[1] != self.E:
            raise ValueError("GhostGallery.add takes [m,%d] features, not %s" % (self.E, tuple(feats.shape)))
        if det_index is None and k > feats.shape[0]:
            raise ValueError("GhostGallery.add: %d slots for %d features" % (k, feats.shape[0]))
        t = self._tables("GhostGallery.add", k, slots=slots, det_index=det_index, new=new)
        if k == 0:
            return
        _store_lib.check(_store_lib.load().busca_store_ring_add(
            self._gallery.data_ptr(), self._count.data_ptr(), self._newest.data_ptr(), self._mv_seen.data_ptr(), self.capacity, self.budget, self.E,
            t["slots"].data_ptr(), k, feats.data_ptr(), feats.shape[0], ptr(t["det_index"]), ptr(t["new"]), self.dev.index, stream_of(self.dev)))

    def release(self, slots):
        """The tracks in `slots` are gone: count = 0 and mv_seen = 0, so the slot reads as empty and can be given to a new track.  One
        busca_store_release."""
        slots, k = _slots_checked(slots, self.capacity, "GhostGallery.release")
        if k == 0:
            return
        s = self._tables("GhostGallery.release", k, slots=slots)["slots"]
        _store_lib.check(_store_lib.load().busca_store_release(self._count.data_ptr(), self._mv_seen.data_ptr(), self.capacity, s.data_ptr(), k,
                                                               self.dev.index, stream_of(self.dev)))

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
