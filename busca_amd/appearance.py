"""Appearance association of the ByteTrack-style and DeepSORT-style trackers: cosine gallery cost, the gates on it and StrongSORT's first matching
stage.  Fronts busca_appearance_cost of include/busca_appearance.h; restates matching.embedding_distance / fuse_iou
(adapters/ByteTrack/yolox/tracker/matching.py:113-129,159-170), gate_cost_matrix (adapters/StrongSORT/deep_sort/linear_assignment.py:164-210) and
Tracker._match's first stage (deep_sort/tracker.py:211-236).  nn_matching.py is not in the reference tree: see NearestNeighborDistanceMetric."""
import numpy as np
import torch

from . import _lib, _store_lib, geometry
from ._xfer import dev_of, small_to_dev, stream_of, to_dev
from .assignment import _assign_dev, _solved
from .kalman import _download_with_status, _gate_dev, _gating_dev, _measurements, _raise_flagged, _upload_states
from .track_boxes import _tlbrs

_REDUCE = {"min": _lib.APPEAR_MIN, "mean": _lib.APPEAR_MEAN, "max": _lib.APPEAR_MAX}
INFTY_COST = 1e+5                       # deep_sort/linear_assignment.py:12


def _check_width(g, d):
    if d.shape[0] > 0 and g.shape[0] > 0 and d.shape[1] != g.shape[2]:
        raise ValueError("track features are %d-dimensional, detection features %d-dimensional" % (g.shape[2], d.shape[1]))


def gallery_operands(track_feats, slot, count, dev, what, d=None):
    """The gallery operands of the call `what` on the device -> (g [S,budget,E] f32, slot i32 or None, count i32 or None, n): [n,E] features become
    a gallery of one row per slot; host `slot` / `count` are checked against it (device ones are the caller's) and uploaded.  `d`: the call's
    device detection features, checked with the gallery where the call's message names both."""
    g = to_dev(track_feats, dev, torch.float32)
    if g.dim() == 2:
        g = g.unsqueeze(1)
    if g.dim() != 3 or (d is not None and d.dim() != 2):
        raise ValueError("%s takes [n,E] or [S,budget,E] track features%s" % (what, "" if d is None else " and [m,E] detection features"))
    if d is not None:
        _check_width(g, d)
    S, budget, _ = g.shape
    for name, v, top in (("slot", slot, S), ("count", count, budget + 1)):
        if v is not None and not torch.is_tensor(v) and len(v) and int(np.max(v)) >= top:
            raise ValueError("%s holds %d, beyond the gallery's %d" % (name, int(np.max(v)), top - 1))
    if count is not None and len(count) != S:
        raise ValueError("count has %d entries for %d slots" % (len(count), S))
    slot, count = to_dev(slot, dev, torch.int32, flat=True), to_dev(count, dev, torch.int32, flat=True)
    return g, slot, count, (S if slot is None else slot.numel())


def appearance_cost(track_feats, det_feats, reduce="min", clamp=False, slot=None, count=None, ctx=None):
    """busca_appearance_cost: the cosine distance 1 - <g, d> / sqrt(<g, g> <d, d>) between every track's stored samples and every detection,
    reduced per track ('min' = DeepSORT's nearest neighbour, 'mean', 'max'), float64 on the device.
      track_feats  [n,E] (one vector per track) or [S,budget,E] (a gallery of S slots, `budget` rows each): host array or device tensor
      det_feats    [m,E]
      slot         [n] ints or None: the gallery slot of cost-matrix row i (None: row i is slot i); a negative slot gives a row of +inf
      count        [S] ints or None: the valid rows 0 .. count-1 of every slot (None: all of them); rows beyond are never read
      clamp        max(0, .) of every pair's distance (matching.py:128)
    A device float32 tensor is used as it is, everything else is converted and uploaded.  -> device float64 tensor [n,m]."""
    if reduce not in _REDUCE:
        raise ValueError("reduce must be 'min', 'mean' or 'max', not %r" % (reduce,))
    ctx, dev = geometry.ctx_dev(ctx)
    d = to_dev(det_feats, dev, torch.float32)
    g, slot, count, n = gallery_operands(track_feats, slot, count, dev, "appearance_cost", d)
    budget, E, m = g.shape[1], g.shape[2], d.shape[0]
    out = torch.empty(n, m, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_appearance_cost(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), n, budget, d.data_ptr(), m, E, _REDUCE[reduce],
                                            _lib.APPEAR_CLAMP0 if clamp else 0, out.data_ptr(), stream_of(dev)))
    return out


def _is_array(x):
    return torch.is_tensor(x) or isinstance(x, np.ndarray)


def embedding_distance(tracks, detections, metric="cosine", ctx=None):
    """matching.embedding_distance (adapters/ByteTrack/yolox/tracker/matching.py:113-129): max(0, cosine distance) between the tracks' `.smooth_feat`
    and the detections' `.curr_feat`, [n,m] float64 on the host.  Either side may be an [k,E] array or device tensor instead (ReID features as
    busca_reid_forward* left them in HBM are used in place).  The reference converts its features to float64 first; these are taken as float32,
    which is what the extractor produces.  An empty side gives zeros((n, m)); only 'cosine' exists."""
    if metric != "cosine":
        raise ValueError("embedding_distance: only the 'cosine' metric is implemented, not %r" % (metric,))
    n, m = len(tracks), len(detections)
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    tf = tracks if _is_array(tracks) else np.asarray([t.smooth_feat for t in tracks], dtype=np.float32)
    df = detections if _is_array(detections) else np.asarray([t.curr_feat for t in detections], dtype=np.float32)
    return appearance_cost(tf, df, clamp=True, ctx=ctx).cpu().numpy()


def fuse_iou(cost, tracks, detections, ctx=None):
    """matching.fuse_iou (matching.py:159-170): 1 - (1 - cost) * (1 + (1 - iou_distance(tracks, detections))) / 2, evaluated on the device in the
    reference's order of operations from busca_pairwise's IOU_COST; `cost`: [n,m] host array or device tensor (appearance_cost).  One copy back."""
    n, m = len(tracks), len(detections)
    if n == 0 or m == 0:                                       # `if cost_matrix.size == 0: return cost_matrix`
        return cost.cpu().numpy() if torch.is_tensor(cost) else cost
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(cost, dev, torch.float64).reshape(n, m)
    iou_sim = 1 - geometry.pairwise(ctx, _tlbrs(tracks), _tlbrs(detections), _lib.PAIR_IOU_COST)
    fuse_sim = (1 - cost) * (1 + iou_sim) / 2
    return (1 - fuse_sim).cpu().numpy()


class NearestNeighborDistanceMetric:
    """The object DeepSORT's Tracker holds as `self.metric` (adapters/StrongSORT/deep_sort/tracker.py:211-219), with every track's sample gallery
    resident in HBM: `partial_fit` appends to it, `distance` is one busca_appearance_cost launch over it.

    Parity-unpinned: the upstream nn_matching.py is not part of the reference tree, so this class is restated from the published DeepSORT
    algorithm (Wojke et al. 2017: per target the last `budget` samples, distance = the smallest cosine distance to any of them) and tested
    against a numpy restatement of it, not against the reference's output.

    The gallery is one float32 tensor [slots, ring, E]; a target owns a slot, its samples fill the slot's ring and, with a budget, overwrite
    the oldest (the nearest-neighbour distance does not depend on their order).  Which target owns which slot and how full it is is host
    Python; samples are written with torch indexing.  `budget=None` keeps every sample: the ring doubles when a target fills it."""

    def __init__(self, metric, matching_threshold, budget=None, ctx=None):
        if metric != "cosine":
            raise ValueError("Invalid metric; only 'cosine' is implemented on the device")
        if budget is not None and int(budget) < 1:
            raise ValueError("budget must be at least 1")
        self.matching_threshold = matching_threshold
        self.budget = None if budget is None else int(budget)
        self._ctx = ctx
        self._slot = {}                                     # target -> slot
        self._free = []
        self._total = np.zeros(0, dtype=np.int64)           # samples ever appended to a slot since it was taken
        self._gallery = None                                # device f32 [slots, ring, E]
        self._count_dev = None                              # device i32 [slots]

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = geometry.default_context()
        return self._ctx

    @property
    def samples(self):
        """{target: [k,E] float32 host array of its stored samples}, oldest first - for inspection and tests; one download."""
        if self._gallery is None:
            return {}
        host, ring = self._gallery.cpu().numpy(), self._gallery.shape[1]
        out = {}
        for t, s in self._slot.items():
            tot = int(self._total[s])
            out[t] = host[s, :tot].copy() if tot <= ring else np.roll(host[s], -(tot % ring), axis=0)
        return out

    def _reserve(self, slots, ring, E, dev):
        g = self._gallery
        if g is not None and g.shape[0] >= slots and g.shape[1] >= ring:
            return
        ns = max(slots, 0 if g is None else g.shape[0])
        nr = max(ring, 0 if g is None else g.shape[1])
        new = torch.zeros(ns, nr, E, dtype=torch.float32, device=dev)
        if g is not None:
            new[:g.shape[0], :g.shape[1]] = g
        self._gallery = new
        self._total = np.concatenate([self._total, np.zeros(ns - len(self._total), dtype=np.int64)])

    def _fit_ema(self, features, targets, alpha, dev):
        """partial_fit's EMA route: deep_sort/track.py:244-248 (and :85-87 for a target's first feature) as one busca_store_ema_fit launch
        (include/busca_store.h) on torch's current stream.  The host groups the call's features by target - one upload of the group table - and
        one workgroup per target applies its features in call order, so a target fed several times costs no further launch."""
        f = to_dev(features, dev, torch.float32).reshape(len(targets), -1)
        E = f.shape[1]
        if self._gallery is not None and self._gallery.shape[2] != E:
            raise ValueError("the gallery holds %d-dimensional samples, these have %d dimensions" % (self._gallery.shape[2], E))
        for t in targets:
            if t not in self._slot:
                self._slot[t] = self._free.pop() if self._free else len(self._slot)
        slots_needed = max(self._slot.values()) + 1
        have_s = 0 if self._gallery is None else self._gallery.shape[0]
        if slots_needed > have_s:
            slots_needed = max(slots_needed, 2 * have_s, 16)
        self._reserve(slots_needed, 1, E, dev)
        S, ring = self._gallery.shape[:2]
        groups = {}                                         # slot -> [ring row of the sample it has or -1, the rows of `features` for it in call order]
        for k, t in enumerate(targets):
            s = self._slot[t]
            if s not in groups:
                tot = int(self._total[s])
                groups[s] = [(tot - 1) % ring if tot else -1, []]
                self._total[s] = 1
            groups[s][1].append(k)
        start = np.cumsum([0] + [len(ks) for _, ks in groups.values()])
        g, k = len(groups), len(targets)
        table = small_to_dev(np.concatenate([list(groups), [old for old, _ in groups.values()], start, [j for _, ks in groups.values() for j in ks]])
                             .astype(np.int32), dev, torch.int32)      # one upload: group_slot [g], group_old_row [g], group_start [g + 1], src [k]
        _store_lib.check(_store_lib.load().busca_store_ema_fit(
            self._gallery.data_ptr(), S, ring, E, f.data_ptr(), k, table.data_ptr(), table[g:].data_ptr(), table[2 * g:].data_ptr(),
            table[3 * g + 1:].data_ptr(), g, k, alpha, dev.index, stream_of(dev)))

    def partial_fit(self, features, targets, active_targets, ema_alpha=None):
        """Append feature k, L2-normalised (in float64, stored as float32; deep_sort/track.py:244 stores normalised features), to the samples of
        targets[k]; keep each target's last `budget`; drop every target that is not in `active_targets` and free its slot.
        `ema_alpha` (StrongSORT's opt.EMA with opt.EMA_alpha, deep_sort/track.py:244-248): the target's slot holds ONE row instead.  With
        feature = f / ||f||, a target that has a sample replaces it by smooth / ||smooth||, smooth = ema_alpha * old + (1 - ema_alpha) * feature; a
        target without one stores feature (track.py:85-87).  Float32 in that order, one busca_store_ema_fit launch; `features` may be the device tensor
        appearance_round was given.  Several features for one target in one call are applied in call order.  `budget` is ignored under EMA.
        Use a metric with `ema_alpha` throughout or not at all (a gallery of several samples collapses to its newest one at the first EMA call)."""
        targets = list(np.asarray(targets).reshape(-1).tolist()) if not isinstance(targets, list) else targets
        dev = dev_of(self.ctx)
        if len(targets) and ema_alpha is not None:
            self._fit_ema(features, targets, float(ema_alpha), dev)
        elif len(targets):
            f = to_dev(features, dev, torch.float32).reshape(len(targets), -1).to(torch.float64)
            f = (f / torch.sqrt((f * f).sum(1, keepdim=True))).to(torch.float32)
            E = f.shape[1]
            if self._gallery is not None and self._gallery.shape[2] != E:
                raise ValueError("the gallery holds %d-dimensional samples, these have %d dimensions" % (self._gallery.shape[2], E))
            per = {}
            for k, t in enumerate(targets):
                per.setdefault(t, []).append(k)
            for t in per:
                if t not in self._slot:
                    self._slot[t] = self._free.pop() if self._free else len(self._slot)
            slots_needed = max(self._slot.values()) + 1
            have_s = 0 if self._gallery is None else self._gallery.shape[0]
            have_r = 0 if self._gallery is None else self._gallery.shape[1]
            if self.budget is not None:
                ring = self.budget
            else:
                need = max(int(self._total[self._slot[t]]) if self._slot[t] < len(self._total) else 0 for t in per)
                need += max(len(v) for v in per.values())
                ring = max(have_r, 4)
                while ring < need:
                    ring *= 2
            if slots_needed > have_s:
                slots_needed = max(slots_needed, 2 * have_s, 16)
            self._reserve(slots_needed, ring, E, dev)
            ring = self._gallery.shape[1]
            src, ds, dr = [], [], []
            for t, ks in per.items():
                s = self._slot[t]
                tot = int(self._total[s])
                skip = max(0, len(ks) - ring)               # more than a ring's worth in one call: the oldest would be overwritten at once
                for i, k in enumerate(ks):
                    if i >= skip:
                        src.append(k)
                        ds.append(s)
                        dr.append((tot + i) % ring)
                self._total[s] = tot + len(ks)
            idx = torch.from_numpy(np.asarray([src, ds, dr], dtype=np.int64)).to(dev)       # one upload for the three index vectors
            self._gallery[idx[1], idx[2]] = f[idx[0]]
        active = set(np.asarray(active_targets).reshape(-1).tolist()) if not isinstance(active_targets, (set, list, tuple)) else set(active_targets)
        for t in [t for t in self._slot if t not in active]:
            s = self._slot.pop(t)
            self._total[s] = 0
            self._free.append(s)
        if self._gallery is not None:
            self._count_dev = torch.from_numpy(np.minimum(self._total, self._gallery.shape[1]).astype(np.int32)).to(dev)

    def distance(self, features, targets, device=False):
        """[len(targets), len(features)] float64: the smallest cosine distance between each target's stored samples and each feature.  A target
        without samples gives a row of +inf.  `features`: host array or device tensor [m,E]; `device=True` leaves the matrix on the device."""
        targets = list(np.asarray(targets).reshape(-1).tolist()) if not isinstance(targets, list) else targets
        n, m = len(targets), len(features)
        dev = dev_of(self.ctx)
        if n == 0 or m == 0 or self._gallery is None:
            out = torch.full((n, m), float("inf"), dtype=torch.float64, device=dev)
        else:
            slot = np.asarray([self._slot.get(t, -1) for t in targets], dtype=np.int32)
            out = appearance_cost(self._gallery, features, "min", slot=slot, count=self._count_dev, ctx=self.ctx)
        return out if device else out.cpu().numpy()


def _xyah_of(detections, detection_indices):
    """[m,4] float64 measurements of detections[detection_indices]: `.to_xyah()` where a detection has it (deep_sort), tlwh_to_xyah(.tlwh) otherwise."""
    dets = [detections[i] for i in detection_indices]
    if len(dets) and hasattr(dets[0], "to_xyah"):
        return np.asarray([d.to_xyah() for d in dets], dtype=np.float64).reshape(-1, 4)
    return _measurements(dets)


def _gate_mc_dev(ctx, cost, tracks, detections, track_indices, detection_indices, gated_cost, mc_lambda):
    """Device part of gate_cost_matrix_mc -> (gated [n,m] device matrix, Kalman status words [n])."""
    dev = dev_of(ctx)
    mean, cov = _upload_states([tracks[i] for i in track_indices], dev)
    gate, status = _gating_dev(ctx, mean, cov, torch.from_numpy(_xyah_of(detections, detection_indices)).to(dev), False, 0)
    return _gate_dev(cost, gate, False, None if mc_lambda is None else float(mc_lambda), float(gated_cost)), status


def gate_cost_matrix_mc(cost, tracks, detections, track_indices, detection_indices, gated_cost=INFTY_COST, mc_lambda=None, ctx=None):
    """gate_cost_matrix (adapters/StrongSORT/deep_sort/linear_assignment.py:164-210): entry (i, j) whose squared Mahalanobis distance between
    tracks[track_indices[i]] and detections[detection_indices[j]] (busca_kalman_gating on the tracks' `mean` / `covariance`) exceeds
    chi2inv95[4] = 9.4877 becomes `gated_cost`; then with `mc_lambda` (opt.MC, opt.MC_lambda) EVERY entry - the gated ones too, as in the
    reference - becomes mc_lambda * cost + (1 - mc_lambda) * distance.  `cost`: [n,m] host array or device tensor.  Returns a new host array."""
    n, m = len(track_indices), len(detection_indices)
    if n == 0 or m == 0:
        return cost.cpu().numpy() if torch.is_tensor(cost) else cost
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(cost, dev, torch.float64).reshape(n, m)
    out, status = _gate_mc_dev(ctx, cost, tracks, detections, track_indices, detection_indices, gated_cost, mc_lambda)
    return _download_with_status(out, status, "gate_cost_matrix_mc")


def appearance_round(metric, tracks, detections, track_indices, detection_indices=None, cascade_depth=None, mc_lambda=None, ctx=None, det_features=None):
    """The first stage of Tracker._match (adapters/StrongSORT/deep_sort/tracker.py:214-236) without leaving the device: metric.distance of the
    detections' `.feature` against the gallery of the tracks' `.track_id` -> gate_cost_matrix_mc -> the clamp of min_cost_matching at
    metric.matching_threshold -> busca_linear_assignment.  `metric`: a NearestNeighborDistanceMetric.  Without `cascade_depth` (opt.woC) that is
    one problem and one device->host copy of the match vectors and status words; with it, the matching cascade: per level one device row / column
    gather of the same matrix, one solve and one copy.  The [n,m] matrix never crosses.  `det_features`: the features of ALL `detections` as an
    [len(detections),E] array or device tensor, instead of their `.feature`.  Returns what matching_cascade returns."""
    track_indices = list(track_indices)
    detection_indices = list(range(len(detections))) if detection_indices is None else list(detection_indices)
    n, m = len(track_indices), len(detection_indices)
    if n == 0 or m == 0:
        return [], track_indices, detection_indices
    ctx = ctx or metric.ctx
    dev = dev_of(ctx)
    if det_features is None:
        feats = to_dev(np.asarray([detections[i].feature for i in detection_indices], dtype=np.float32), dev, torch.float32)
    else:
        feats = to_dev(det_features, dev, torch.float32)
        if detection_indices != list(range(feats.shape[0])):
            feats = feats[torch.from_numpy(np.asarray(detection_indices, dtype=np.int64)).to(dev)]
    cost = metric.distance(feats, [tracks[i].track_id for i in track_indices], device=True)
    cost, kstatus = _gate_mc_dev(ctx, cost, tracks, detections, track_indices, detection_indices, INFTY_COST, mc_lambda)
    limit = metric.matching_threshold + 1e-5
    cost = torch.where(cost > metric.matching_threshold, limit, cost)
    if cascade_depth is None:
        levels = [list(range(n))]
    else:
        levels = [[r for r, k in enumerate(track_indices) if tracks[k].time_since_update == 1 + level] for level in range(cascade_depth)]
    matches, cols, checked = [], list(range(m)), False
    for rows in levels:
        if len(cols) == 0:
            break
        if len(rows) == 0:
            continue
        if len(rows) == n and len(cols) == m:
            sub = cost
        else:
            idx = torch.from_numpy(np.asarray(rows + cols, dtype=np.int64)).to(dev)          # one upload for both index vectors
            sub = cost.index_select(0, idx[:len(rows)]).index_select(1, idx[len(rows):])
        parts = [_assign_dev(ctx, sub.contiguous(), 1, len(rows), len(cols), limit).view(-1)]
        if not checked:
            parts.append(kstatus)
        host = torch.cat(parts).cpu().numpy()                    # one device->host copy: match vectors, solver status, Kalman status words
        if not checked:
            _raise_flagged(host[len(rows) + len(cols) + 1:], "appearance_round")
            checked = True
        pairs, _, left = _solved(host, len(rows), len(cols), "appearance_round")
        matches += [(track_indices[rows[r]], detection_indices[cols[c]]) for r, c in pairs]
        cols = [cols[c] for c in left]
    unmatched_tracks = list(set(track_indices) - set(k for k, _ in matches))
    return matches, unmatched_tracks, [detection_indices[c] for c in cols]
