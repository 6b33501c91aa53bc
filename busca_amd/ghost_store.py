"""GHOST's frame on resident track state as one chain.  Fronts include/busca_gframe.h (libbusca_gframe.so, bound by _gframe_lib) around the proxy
and distance launches of ghost_round (include/busca_ghost.h) and busca_linear_assignment; restates Tracker._track without the BUSCA round
(adapters/GHOST/src/tracker.py:203-261): motion_compensation's loop and BaseTracker.motion (base_tracker.py:600-698), get_hungarian_* and
solve_hungarian (tracker.py:306-480), assign_act_inact_same_time / assign_separatly (tracker.py:597-682) and Track.add_detection / Track.__init__
(tracking_utils.py:254-370)."""
from collections import namedtuple

import numpy as np
import torch

from . import _gframe_lib, _lib, _mgframe_lib, geometry
from ._xfer import h2d_async, stream_of, to_dev
from .ghost import (GHOST_LIMIT, _GHOST_PROXY, _GHOST_REDUCE, _ghost_appearance, _ghost_blend_plan, _ghost_mv_avg_table, _ghost_threshold_plan, ghost_check_config,
                    ghost_thresholds)
from .ghost_gallery import GhostGallery
from .ghost_motion import GhostMotion, _slots_checked, ghost_motion_check_config

APPEAR_E_MIN, APPEAR_E_MAX = 16, 2048      # BUSCA_APPEAR_E_MIN / _MAX: the feature widths busca_ghost_distance takes (multiples of 16)

GhostFrame = namedtuple("GhostFrame", "matches new overflow unassigned_active unassigned_inactive thresholds dist")
GhostFrame.__doc__ = """What GhostStore.frame returns.
  matches              [(track row, detection)] sorted by track row: the rows index `active` followed by `inactive`
  new                  [(detection, slot)]: the tracks started, in detection order
  overflow             the detections that would have started a track but found no free slot left
  unassigned_active    the rows of active tracks without a detection: what the BUSCA round works on afterwards
  unassigned_inactive  the rows of in-patience inactive tracks without a detection
  thresholds           (act, inact) as the filter read them
  dist                 the device cost matrix in ghost_round's orientation ([detections, tracks]; with assign_separately the list [dist_act,
                       dist_inact], dist_inact None without active tracks - its entries of assigned detections are NaN); None without a round"""


def _no_frame(n_active, n_inactive, thresholds=(float("inf"), float("inf"))):
    return GhostFrame([], [], [], list(range(n_active)), list(range(n_active, n_active + n_inactive)), thresholds, None)


class GhostStore:
    """GHOST's Track state on the device for `capacity` track slots: one GhostGallery (feature rings, mv_avg) and one GhostMotion (position rings,
    position, velocity) on the same slots, exposed as `.gallery` and `.motion` - add / release / state / compensate keep working, and the BUSCA round
    and the releases go through them - and frame(), Tracker._track as one chain on the stream."""

    def __init__(self, capacity, budget, E, history, box_dtype=np.float64, ctx=None):
        self.ctx, self.dev = geometry.ctx_dev(ctx)
        self.gallery = GhostGallery(capacity, budget, E, ctx=self.ctx)
        self.motion = GhostMotion(capacity, history, box_dtype=box_dtype, ctx=self.ctx)
        self.capacity, self.budget, self.E, self.history = self.gallery.capacity, self.gallery.budget, self.gallery.E, self.motion.history

    def _frame_checked(self, active, inactive, idle, free_slots, det_feats, det_boxes, det_conf, labels, warp, thresholds, cfg, what="GhostStore.frame"):
        """The host side of frame(), before anything is allocated, enqueued or written -> the plan as a dict."""
        cfg = ghost_check_config(dict(cfg or {}))
        mcfg, blend, alpha = _ghost_blend_plan(cfg)
        ghost_motion_check_config(mcfg, cfg.get("kalman", False))
        at, it, every, data_act, data_inact = _ghost_threshold_plan(cfg)
        act, inact = cfg.get("avg_act", {}), cfg.get("avg_inact", {})
        each = inact.get("proxy") == "each_sample"
        if not each:
            for entry, name in ((act, "avg_act"), (inact, "avg_inact")):
                proxy = entry.get("proxy", "last")
                if not entry.get("do", False) or proxy == "last" or entry.get("num", "all") == "first":
                    continue
                if proxy == "mv_avg":
                    _ghost_mv_avg_table(dict(mv_avg=self.gallery.mv_avg, mv_seen=self.gallery.mv_seen), entry, name)
                    float(entry["num"])
                elif proxy == "mode" or proxy not in _GHOST_PROXY:
                    raise NotImplementedError("%s: %s proxy %r is not built on the device" % (what, name, proxy))
        last_n = min(int(mcfg.get("last_n_frames", 100000000)), 2 ** 31 - 1)
        if blend and last_n < 2:
            raise ValueError("%s: last_n_frames = %d; at least 2" % (what, last_n))
        lists = []
        for name, x in (("active", active), ("inactive", inactive), ("idle", idle), ("free_slots", free_slots)):
            if torch.is_tensor(x):
                raise ValueError("%s takes host slot lists (%s)" % (what, name))
            x = np.asarray(x, dtype=np.int64).reshape(-1)
            if (x < 0).any():
                raise ValueError("%s: a slot of `%s` is negative" % (what, name))
            lists.append(x)
        listed = _slots_checked(np.concatenate(lists[:3]), self.capacity, "%s: active, inactive and idle together" % what)[0]
        free = _slots_checked(lists[3], self.capacity, "%s: free_slots" % what)[0]
        taken = np.intersect1d(listed, free)
        if len(taken):
            raise ValueError("%s: free slot %d is also listed as a track's" % (what, int(taken[0])))
        na, ni = len(lists[0]), len(lists[1])
        n = na + ni
        if not APPEAR_E_MIN <= self.E <= APPEAR_E_MAX or self.E % 16:
            raise ValueError("%s: E %d - busca_ghost_distance takes a multiple of 16 in %d .. %d" % (what, self.E, APPEAR_E_MIN, APPEAR_E_MAX))
        shape = tuple(det_feats.shape) if hasattr(det_feats, "shape") else np.shape(det_feats)
        if torch.is_tensor(det_boxes):
            raise ValueError("%s takes host detection boxes" % what)
        boxes = np.asarray(det_boxes, dtype=np.float32 if self.motion.box32 else np.float64).astype(np.float64)
        if boxes.size == 0:
            boxes = boxes.reshape(0, 4)
        if boxes.ndim != 2 or boxes.shape[1] != 4:
            raise ValueError("%s takes [m,4] tlbr detection boxes, not %s" % (what, boxes.shape))
        m = len(boxes)
        if m and (len(shape) != 2 or shape[0] != m or shape[1] != self.E):
            raise ValueError("%s: %s features for %d detections of a store with E %d" % (what, shape, m, self.E))
        if n > _lib.ASSIGN_MAX or m > min(_lib.ASSIGN_MAX, _gframe_lib.MAX_DETS):
            raise ValueError("%s: %d tracks and %d detections, the device solver takes at most %d rows and columns" % (what, n, m, _lib.ASSIGN_MAX))
        conf = None
        if det_conf is not None:
            conf = np.asarray(det_conf).reshape(-1)
            if len(conf) != m:
                raise ValueError("%s: %d confidences for %d detections" % (what, len(conf), m))
        tl = dl = None
        if labels is not None:
            tl, dl = (np.asarray(x, dtype=np.int32).reshape(-1) for x in labels)
            if len(tl) != n or len(dl) != m:
                raise ValueError("%s: %d track labels and %d detection labels for %d tracks and %d detections" % (what, len(tl), len(dl), n, m))
            if not (each and cfg.get("nan_over_classes", True)):       # as in the reference only the each_sample route masks classes
                tl = dl = None
        if warp is not None and not torch.is_tensor(warp):
            warp = np.asarray(warp, dtype=np.float32)
            if warp.size != 6:
                raise ValueError("%s takes a [2,3] warp, not %s" % (what, warp.shape))
            warp = np.ascontiguousarray(warp.reshape(6))
        elif warp is not None and not (warp.is_cuda and warp.dtype == torch.float32 and warp.numel() == 6 and warp.is_contiguous()):
            raise ValueError("%s: a device warp is a contiguous float32 tensor of 6 values" % what)
        if thresholds is not None and not (torch.is_tensor(thresholds) and thresholds.is_cuda and thresholds.dtype == torch.float64
                                           and thresholds.numel() == 2 and thresholds.is_contiguous()):
            raise ValueError("%s: thresholds is a contiguous device float64 tensor of 2 values" % what)
        fixed = np.asarray([float("inf") if isinstance(v, str) or v is None else float(v) for v in (at, it)], dtype=np.float64)
        return dict(cfg=cfg, blend=blend, alpha=alpha, every=every, data_act=data_act, data_inact=data_inact, each=each, last_n=last_n, listed=listed,
                    free=free, na=na, n=n, n_idle=len(lists[2]), boxes=boxes, m=m, conf=conf, tl=tl, dl=dl, warp=warp, fixed=fixed,
                    nan_first=bool(cfg.get("nan_first", False)), sep=bool(cfg.get("assign_separately", False)),
                    new_track_conf=cfg.get("new_track_conf", 0.0))

    def frame(self, active, inactive, det_feats, det_boxes, frame, cfg, det_conf=None, idle=(), free_slots=(), labels=None, warp=None, thresholds=None,
              apply=True):
        """Tracker._track (adapters/GHOST/src/tracker.py:203-261) without the BUSCA round on resident state, as ONE chain on torch's current stream:
        one pinned upload of every small table (slots, free slots, may_start, labels, warp, fixed thresholds), one float64 upload of the boxes,
        busca_gframe_advance (the warp of every listed track's stored boxes and BaseTracker.motion in one launch), the proxy and distance launches
        of ghost_round, with data-driven thresholds the class mask and busca_ghost_thresholds, busca_gframe_cost (class mask, motion blend,
        nan_first in one pass, in place), busca_linear_assignment with ghost_round's limit, busca_gframe_keep (the filter of
        assign_act_inact_same_time), with assign_separately a second solve on the inactive block and a second keep, busca_gframe_apply
        (Track.add_detection of every assigned track, Track.__init__ of every detection that starts one) and ONE device->host copy:
        track_det | det_track | det_slot | solver status words (| thr when it was computed on the device).  The host reads the matches after the state
        update has been enqueued, not before.  -> GhostFrame.
          active, inactive   host slot lists: self.tracks, and the inactive tracks with inactive_count <= inact_patience (curr_it); the rows of the
                             cost matrix, ACTIVE TRACKS FIRST
          idle               the inactive tracks beyond inact_patience: warped and stepped, never matched
          det_feats          [m,E] float32; a device tensor is read in place.  det_boxes: host [m,4] tlbr, rounded to the store's box_dtype
          frame              the frame number the rings store (Track.past_frames)
          cfg                the reference's tracker_cfg as ghost_round takes it, with 'new_track_conf'
          det_conf           [m] or None (every unassigned detection may start a track)
          free_slots         where new tracks go, in the order of their detections; disjoint from the listed tracks (ValueError otherwise)
          labels             (track_labels [n], det_labels [m]) or None; as in the reference only the each_sample route masks classes
          warp               the [2,3] camera warp of this frame (host float32, or a device float32 tensor of 6 values), or None
          thresholds         a device float64 [2] tensor that receives (act, inact) as the filter read them (one more small copy on the stream)
          apply=False        stop after the filter: no state is written after the step
        The listed slots - active, inactive and idle together - must be all the live tracks of the store: motion_compensation warps every track.
        Quirks of the reference that are kept:
          - no detections: get_hungarian_* is never called, so motion() does not run - the warp happens, no step, nothing is copied home
          - no active and no in-patience inactive track: every detection starts a track whatever its confidence (tracker.py:209-218), and no step
            runs.  Otherwise a detection starts a track only when it was not assigned and conf > new_track_conf: `may_start` is that numpy
            comparison on det_conf as given, made on the host
          - motion_step runs for ALL inactive tracks, also those beyond inact_patience (base_tracker.py:696-698): `idle`
          - the step's differences are float32 when the boxes are, or when every stored row has been warped: with a warp this call sets
            motion.all_warped as compensate() of all slots does, and an applied detection clears it as add() does
          - assign_separately without active tracks never matches an inactive track (dist_inact = None, tracker.py:406-409)
          - the filter is `<` while nan_first is `<=`: a matched pair whose cost equals its threshold is not assigned, and with assign_separately
            its detection stays available to the inactive tracks
          - a class-masked entry makes update_thresholds' mean NaN, in the reference too: with 'every' / 'tbd' and mixed classes nothing is kept
          - with assign_separately the reference writes the second stage's tr_ids at the compacted detection index (tracker.py:633 with the list of
            :674) while add_detection gets the right detection: `matches` names the detection that was added
          - use_bism, non-cosine distances, center_only, approximate, the Kalman route and proxy 'mode' are refused, before anything is enqueued
        Raises BuscaError on a solver status (the state update has been enqueued by then)."""
        p = self._frame_checked(active, inactive, idle, free_slots, det_feats, det_boxes, det_conf, labels, warp, thresholds, cfg)
        na, n, n_idle, m, sep, blend = p["na"], p["n"], p["n_idle"], p["m"], p["sep"], p["blend"]
        n_all, n_free = n + n_idle, len(p["free"])
        g, mo, dev = self.gallery, self.motion, self.dev
        flib = _gframe_lib.load()
        where = (dev.index, stream_of(dev))
        data = p["data_act"] or p["data_inact"]
        round_ = n > 0 and m > 0
        # ---- one pinned upload: float64 thresholds, float32 warp, the int32 tables, the may_start bytes
        host_warp = p["warp"] if isinstance(p["warp"], np.ndarray) else None
        if n == 0:
            may = np.ones(m, dtype=np.uint8)
        elif p["conf"] is None:
            may = np.ones(m, dtype=np.uint8)
        else:
            may = (p["conf"] > p["new_track_conf"]).astype(np.uint8)
        minus = np.full(max(n, m) if m and (n == 0 or (sep and na == 0)) else 0, -1, dtype=np.int32)
        ints = [p["listed"], p["free"], minus] + ([p["tl"], p["dl"]] if p["tl"] is not None and round_ else [])
        ints = np.concatenate(ints).astype(np.int32)
        parts = [p["fixed"].view(np.uint8), (host_warp if host_warp is not None else np.zeros(6, dtype=np.float32)).view(np.uint8), ints.view(np.uint8), may]
        up = h2d_async(np.concatenate(parts), dev)
        d_fixed = up[:16].view(torch.float64)
        d_warp = None if p["warp"] is None else (up[16:40].view(torch.float32) if host_warp is not None else p["warp"])
        words = up[40:40 + 4 * len(ints)].view(torch.int32)
        d_listed, d_free = words[:n_all], words[n_all:n_all + n_free]
        d_minus = words[n_all + n_free:n_all + n_free + len(minus)]
        d_tl = d_dl = None
        if p["tl"] is not None and round_:
            at = n_all + n_free + len(minus)
            d_tl, d_dl = words[at:at + n], words[at + n:at + n + m]
        d_may = up[40 + 4 * len(ints):]
        if d_warp is not None:
            mo.all_warped = True                                   # every live track is listed: compensate() of all slots
        step = blend and round_
        rings = (mo.hist.data_ptr(), mo.frames.data_ptr(), mo.count.data_ptr(), mo.newest.data_ptr(), mo.pos.data_ptr(), mo.vel.data_ptr())
        pos = torch.empty(n_all, 4, dtype=torch.float64, device=dev) if step else None
        if n_all and (step or d_warp is not None):
            _gframe_lib.check(flib.busca_gframe_advance(*rings, self.capacity, self.history, d_listed.data_ptr(), n_all, n_all if step else 0,
                                                        na if step else 0, p["last_n"], int(mo.diff32), _lib.ptr(d_warp), _lib.ptr(pos), *where))
        if m == 0:
            return _no_frame(na, n - na)
        d_boxes = h2d_async(p["boxes"].reshape(-1), dev)           # the one float64 upload
        feats = to_dev(det_feats, dev, torch.float32)
        ctx = self.ctx
        # the words that go home: [thr as 4 words, when computed here] | track_det [n] | det_track [m] | det_slot [m] | solver status [2]
        head = 4 if data and round_ else 0
        out = torch.empty(head + n + 2 * m + 2, dtype=torch.int32, device=dev)
        base = out.data_ptr() + 4 * head
        p_track_det, p_det_track, p_det_slot, p_status = base, base + 4 * n, base + 4 * (n + m), base + 4 * (n + 2 * m)
        d_status = out[head + n + 2 * m:]
        d_status.zero_()
        cost = None
        d_thr = d_fixed
        if n == 0:                                                 # no track to match: every column is unassigned (that vector is not sent home)
            p_det_track = d_minus.data_ptr()
        else:
            if data:
                d_thr = out[:4].view(torch.float64)
                d_thr.copy_(d_fixed)
            state = dict(mv_avg=g.mv_avg, mv_seen=g.mv_seen)
            app, each = _ghost_appearance(ctx, state, g.gallery, d_listed[:n], g.count, g.newest, n, na, feats, p["cfg"])
            if data:
                if d_tl is not None:                               # solve_hungarian sees the class-masked matrix
                    _gframe_lib.check(flib.busca_gframe_cost(app.data_ptr(), None, None, n, m, 0.0, d_tl.data_ptr(), d_dl.data_ptr(), na, None,
                                                             app.data_ptr(), *where))
                    d_tl = d_dl = None
                k_act, k_inact = (0.0, 2.0) if p["every"] else (0.5, 1.0)
                if p["data_act"] and p["data_inact"]:
                    ghost_thresholds(app, na, k_act, k_inact, out=d_thr, ctx=ctx)
                elif na > 0:                                       # the active threshold only: over the active rows alone
                    ghost_thresholds(app[:na], na, k_act, k_inact, out=d_thr, ctx=ctx)
            cost = app
            if d_tl is not None or blend or p["nan_first"]:
                _gframe_lib.check(flib.busca_gframe_cost(app.data_ptr(), _lib.ptr(pos) if blend else None, d_boxes.data_ptr(), n, m, p["alpha"],
                                                         _lib.ptr(d_tl), _lib.ptr(d_dl), na, d_thr.data_ptr() if p["nan_first"] else None,
                                                         cost.data_ptr(), *where))
            scratch = torch.empty(2 * (n + m), dtype=torch.int32, device=dev)
            sp = scratch.data_ptr()

            def solve(lo, hi, k):                                  # rows lo .. hi - 1 of the contiguous matrix are a [hi - lo, m] problem
                r2c, c2r = sp + 4 * k * (n + m), sp + 4 * (k * (n + m) + n)
                ctx.check(ctx.lib.busca_linear_assignment(ctx.h, cost.data_ptr() + 8 * lo * m, 1, hi - lo, m, None, float(GHOST_LIMIT), r2c, c2r, None, None,
                                                          p_status + 4 * k, where[1]))
                return r2c, c2r

            def keep(lo, hi, r2c, c2r, merge, mask_from):
                _gframe_lib.check(flib.busca_gframe_keep(cost.data_ptr(), n, m, lo, hi, na, r2c, c2r, d_thr.data_ptr(), p_track_det, p_det_track, merge,
                                                         mask_from, *where))
            if not sep:
                keep(0, n, *solve(0, n, 0), 0, -1)
            elif na == 0:                                          # dist_inact = None: no inactive track is matched
                keep(0, n, d_minus.data_ptr(), d_minus.data_ptr(), 0, -1)
            else:
                keep(0, na, *solve(0, na, 0), 0, na if n > na else -1)
                if n > na:
                    keep(na, n, *solve(na, n, 1), 1, -1)
        if apply:
            _gframe_lib.check(flib.busca_gframe_apply(
                *rings, self.history, g._gallery.data_ptr(), g._count.data_ptr(), g._newest.data_ptr(), g._mv_seen.data_ptr(), self.budget, self.E,
                self.capacity, d_listed.data_ptr() if n else None, n, p_track_det if n else None, p_det_track, feats.data_ptr(), d_boxes.data_ptr(), m,
                int(frame), d_may.data_ptr(), d_free.data_ptr() if n_free else None, n_free, p_det_slot, *where))
        if thresholds is not None:
            thresholds.copy_(d_thr)
        host = out.cpu().numpy()                                   # the one device->host copy
        thr = tuple(float(x) for x in (host[:4].view(np.float64) if head else p["fixed"]))
        body = host[head:]
        track_det, det_track, det_slot, status = body[:n], body[n:n + m], body[n + m:n + 2 * m], body[n + 2 * m:]
        if status.any():
            raise _lib.BuscaError("GhostStore.frame: the solver ran out of its loop bounds (status %s) - is a cost -inf?" % status.tolist())
        if n == 0:
            det_track = np.full(m, -1, dtype=np.int32)
        matches = [(int(i), int(track_det[i])) for i in range(n) if track_det[i] >= 0]
        new, overflow = [], []
        if apply:
            new = [(j, int(det_slot[j])) for j in range(m) if det_track[j] < 0 and det_slot[j] >= 0]
            overflow = [j for j in range(m) if det_slot[j] == -2]
            if matches or new:
                mo.all_warped = False                              # an add() since the last warp
        dist = None
        if cost is not None:
            dist = [cost[:na].T, cost[na:].T if na > 0 else None] if sep else cost.T
        return GhostFrame(matches, new, overflow, [i for i in range(na) if track_det[i] < 0], [i for i in range(na, n) if track_det[i] < 0], thr, dist)

    # ---- the frames of many sequences as one chain (busca_mgframe.h, libbusca_mgframe.so; busca_linear_assignment over the batch)
    @staticmethod
    def all_warped_after(problem, frame):
        """What a sequence carries to its next GhostFrameProblem.all_warped: every stored row has been warped - this step had a warp, or the
        sequence came in all warped - and no detection was added since (GhostMotion.all_warped of a tracker of its own)."""
        return bool((problem.warp is not None or problem.all_warped) and not (frame.matches or frame.new))

    def _frame_batch_checked(self, problems, cfg):
        """The host side of frame_batch(), before anything is allocated -> ([the plan of _frame_checked, per problem], the GhostFrameProblems, whether
        the features are device tensors)."""
        what = "GhostStore.frame_batch"
        problems = [p if isinstance(p, GhostFrameProblem) else GhostFrameProblem(*p) for p in problems]
        if len(problems) > _mgframe_lib.MAX_BATCH:
            raise ValueError("%s: %d problems, one call takes %d" % (what, len(problems), _mgframe_lib.MAX_BATCH))
        plans, on_device = [], None
        for k, p in enumerate(problems):
            name = "%s: problem %d" % (what, k)
            try:
                c = self._frame_checked(p.active, p.inactive, p.idle, p.free_slots, p.det_feats, p.det_boxes, p.det_conf, p.labels, p.warp, None, cfg,
                                        what=name)
                if not -2 ** 31 <= int(p.frame) < 2 ** 31:
                    raise ValueError("%s: frame %r is no int32" % (name, p.frame))
            except (ValueError, NotImplementedError) as e:
                if name in str(e):
                    raise
                raise type(e)("%s: %s" % (name, e)) from None
            if c["m"]:                                             # one feature table: concatenated on the host, or by one torch.cat
                dev = torch.is_tensor(p.det_feats)
                if on_device is None:
                    on_device = dev
                elif on_device != dev:
                    raise ValueError("%s: host and device det_feats in one batch (the earlier problems gave %s)"
                                     % (name, "device tensors" if on_device else "host arrays"))
            plans.append(c)
        if len(plans) > 1:                                         # one launch serves them all: what two problems share, two workgroups race on
            taken = np.concatenate([c["listed"] for c in plans] + [c["free"] for c in plans])
            if len(np.unique(taken)) != len(taken):
                slots, count = np.unique(taken, return_counts=True)
                raise ValueError("%s: the tracks and the free slots must be distinct across the whole batch (slot %d is listed twice)"
                                 % (what, int(slots[count > 1][0])))
        if plans and plans[0]["each"]:                             # what busca_mgframe_distance would refuse, before anything is written
            inact = plans[0]["cfg"].get("avg_inact", {})
            reduce = inact.get("num", 2)
            reduce = reduce.lower() if isinstance(reduce, str) else reduce
            if reduce not in _GHOST_REDUCE:
                raise ValueError("%s: avg_inact['num'] must be 'min', 'mean', 'max', 'midrange', 'median' or 1 .. 5, not %r" % (what, reduce))
            if _GHOST_REDUCE[reduce] == _lib.GHOST_MEDIAN and self.budget > _mgframe_lib.MEDIAN_BUDGET_MAX:
                raise ValueError("%s: the median takes a budget of at most %d, not %d" % (what, _mgframe_lib.MEDIAN_BUDGET_MAX, self.budget))
        if plans and plans[0]["sep"]:
            rows = max(c["na"] for c in plans) + max(c["n"] - c["na"] for c in plans)
            if rows > _lib.ASSIGN_MAX:
                raise ValueError("%s: with assign_separately the slab has %d rows (the most active plus the most inactive tracks of a problem), the "
                                 "device solver takes at most %d" % (what, rows, _lib.ASSIGN_MAX))
        return plans, problems, bool(on_device)

    def frame_batch(self, problems, cfg, apply=True):
        """frame() of every GhostFrameProblem(active, inactive, det_feats, det_boxes, frame, det_conf, idle, free_slots, labels, warp, all_warped) of a
        list - the frames of one time step of many sequences that share this store - as ONE chain on torch's current stream -> [GhostFrame], each
        what frame() returns for that problem on a store loaded alike whose motion.all_warped was the problem's `all_warped`; both rings are bit for
        bit what the frames one after the other leave.  `cfg` is the batch's.  Whatever the number of problems: one pinned upload of every small table
        (problem table, slots, free slots, labels, may_start, host warps, fixed thresholds, both `dims` tables), one float64 upload of all boxes,
        one concatenation each where the features or the warps are device tensors, busca_mgframe_advance, the proxy launches of frame() on the whole
        slot list (ordered group-wise: every problem's active tracks, then every problem's inactive ones, then the idle ones), busca_mgframe_distance
        into the padded [B, R, M] slab, with data-driven thresholds the class mask and busca_mgframe_thresholds, busca_mgframe_cost, ONE batched
        busca_linear_assignment with its `dims` (two with assign_separately, the second on the inactive rows, which start at the same slab row in
        every problem), busca_mgframe_keep (twice with assign_separately), busca_mgframe_apply and ONE device->host copy:
        [thr per problem, when computed on the device] | track_det | det_track | det_slot | solver status words.
        Every check of frame() runs per problem and names it; the tracks and the free slots must be distinct across the whole batch, the features all
        host arrays or all device tensors, and the slab within the solver's limit (ValueError, before anything is allocated, uploaded or written).
        Every quirk frame() documents is kept per problem: a problem without detections is warped only, one without active and in-patience
        inactive tracks starts a track per detection and is not stepped.
        GhostMotion.all_warped is one flag for the whole store, and in the reference it belongs to one sequence: a problem carries its own
        `all_warped` (its step's differences are float32 when the boxes are, when it has a warp, or when it says so), this call does not read
        motion.all_warped and leaves it False, and all_warped_after(problem, frame) is what the caller carries to the sequence's next step.
        An empty list gives [].  Raises BuscaError on a solver status naming the problem (the state update has been enqueued by then).  For a single
        sequence frame() is the shorter route."""
        plans, problems, on_device = self._frame_batch_checked(problems, cfg)
        B = len(plans)
        if B == 0:
            return []
        what = "GhostStore.frame_batch"
        first = plans[0]                                           # what the cfg decides is the batch's
        sep, blend, each = first["sep"], first["blend"], first["each"]
        data = first["data_act"] or first["data_inact"]
        g, mo, dev = self.gallery, self.motion, self.dev
        mlib = _mgframe_lib.load()
        where = (dev.index, stream_of(dev))
        # ---- the problem table.  A problem without detections is warped only: its tracks are listed as idle rows; the others keep their groups
        m_k = [c["m"] for c in plans]
        na_k = [c["na"] if c["m"] else 0 for c in plans]
        ni_k = [c["n"] - c["na"] if c["m"] else 0 for c in plans]
        nidle_k = [len(c["listed"]) - na - ni for c, na, ni in zip(plans, na_k, ni_k)]
        f_k = [len(c["free"]) for c in plans]
        round_k = [na + ni > 0 and m > 0 for na, ni, m in zip(na_k, ni_k, m_k)]
        A, I, D = sum(na_k), sum(ni_k), sum(nidle_k)
        n_total, m_total, f_total = A + I + D, sum(m_k), sum(f_k)
        N, M, L = max(na + ni for na, ni in zip(na_k, ni_k)), max(m_k), max(len(c["listed"]) for c in plans)
        NA = max(na_k)
        R, inact_row = (NA + max(ni_k), NA) if sep else (N, -1)
        host_warps = [k for k, c in enumerate(plans) if isinstance(c["warp"], np.ndarray)]
        dev_warps = [k for k, c in enumerate(plans) if torch.is_tensor(c["warp"])]
        W = _mgframe_lib.PROBLEM_WORDS
        table = np.zeros((B, W), dtype=np.int32)
        table[:, 1], table[:, 3], table[:, 5], table[:, 7], table[:, 9], table[:, 10] = na_k, ni_k, nidle_k, m_k, f_k, -1
        table[:, 0] = np.cumsum([0] + na_k[:-1])
        table[:, 2] = A + np.cumsum([0] + ni_k[:-1])
        table[:, 4] = A + I + np.cumsum([0] + nidle_k[:-1])
        table[:, 6] = np.cumsum([0] + m_k[:-1])
        table[:, 8] = np.cumsum([0] + f_k[:-1])
        table[host_warps, 10] = np.arange(len(host_warps))
        table[dev_warps, 10] = len(host_warps) + np.arange(len(dev_warps))
        table[:, 11] = [int(p.frame) for p in problems]
        table[:, 12] = [(_mgframe_lib.DIFF32 if mo.box32 or c["warp"] is not None or p.all_warped else 0) | (_mgframe_lib.STEP if blend and r else 0)
                        for c, p, r in zip(plans, problems, round_k)]
        listed = [np.concatenate([c["listed"][:na] for c, na in zip(plans, na_k)]),
                  np.concatenate([c["listed"][na:na + ni] for c, na, ni in zip(plans, na_k, ni_k)]),
                  np.concatenate([c["listed"][na + ni:] for c, na, ni in zip(plans, na_k, ni_k)])]
        with_labels = each and any(c["tl"] is not None and r for c, r in zip(plans, round_k))
        tl = dl = np.zeros(0, dtype=np.int32)
        if with_labels:                                            # a problem without labels has one class: nothing of it is masked
            tl = np.concatenate([c["tl"][:na] if c["tl"] is not None and r else np.zeros(na, np.int32) for c, na, r in zip(plans, na_k, round_k)]
                                + [c["tl"][na:] if c["tl"] is not None and r else np.zeros(ni, np.int32) for c, na, ni, r in zip(plans, na_k, ni_k, round_k)])
            dl = np.concatenate([c["dl"] if c["tl"] is not None and r else np.zeros(m, np.int32) for c, m, r in zip(plans, m_k, round_k)])
        may = []
        for c, na, ni in zip(plans, na_k, ni_k):
            if na + ni == 0 or c["conf"] is None:
                may.append(np.ones(c["m"], dtype=np.uint8))
            else:
                may.append((c["conf"] > c["new_track_conf"]).astype(np.uint8))
        dims1 = np.stack([na_k if sep else [na + ni for na, ni in zip(na_k, ni_k)], m_k], axis=1)
        dims2 = np.stack([[ni if na else 0 for na, ni in zip(na_k, ni_k)], m_k], axis=1)
        # ---- one pinned upload: float64 thresholds [B, 2], float32 host warps, the int32 tables, the may_start bytes
        fixed = np.tile(first["fixed"], B)
        warps = np.concatenate([plans[k]["warp"] for k in host_warps]) if host_warps else np.zeros(0, dtype=np.float32)
        parts = [table.reshape(-1), listed[0], listed[1], listed[2], np.concatenate([c["free"] for c in plans]), tl, dl, dims1.reshape(-1),
                 dims2.reshape(-1)]
        ints = np.concatenate(parts).astype(np.int32)
        up = h2d_async(np.concatenate([fixed.view(np.uint8), warps.view(np.uint8), ints.view(np.uint8), np.concatenate(may)]), dev)
        at = 16 * B
        d_fixed = up[:at].view(torch.float64)
        d_warps = up[at:at + 4 * len(warps)].view(torch.float32) if host_warps else None
        at += 4 * len(warps)
        d_table, d_act, d_inact, d_idle, d_free, d_tl, d_dl, d_dims1, d_dims2 = up[at:at + 4 * len(ints)].view(torch.int32).split([len(x) for x in parts])
        d_listed = up[at + 4 * W * B:at + 4 * (W * B + n_total)].view(torch.int32)
        d_may = up[at + 4 * len(ints):]
        if dev_warps:                                              # one concatenation: the uploaded host warps, then the device ones
            d_warps = torch.cat(([d_warps] if host_warps else []) + [plans[k]["warp"].reshape(6) for k in dev_warps])
        n_warps = len(host_warps) + len(dev_warps)
        mo.all_warped = False                                      # a sequence's flag travels with its problems (all_warped_after)
        rings = (mo.hist.data_ptr(), mo.frames.data_ptr(), mo.count.data_ptr(), mo.newest.data_ptr(), mo.pos.data_ptr(), mo.vel.data_ptr())
        tail = (self.capacity, d_listed.data_ptr() if n_total else None, n_total, m_total, f_total, n_warps, d_table.data_ptr(), B, N, M, L, R, inact_row)
        stepped = blend and any(round_k)
        pos = None
        if n_total and (stepped or n_warps):
            pos = torch.empty(n_total, 4, dtype=torch.float64, device=dev)
            _mgframe_lib.check(mlib.busca_mgframe_advance(*rings, self.capacity, self.history, d_listed.data_ptr(), n_total, m_total, f_total,
                                                          _lib.ptr(d_warps), n_warps, d_table.data_ptr(), B, N, M, L, R, inact_row, first["last_n"],
                                                          pos.data_ptr(), *where))
        if M == 0:
            return [_no_frame(c["na"], c["n"] - c["na"]) for c in plans]
        d_boxes = h2d_async(np.concatenate([c["boxes"].reshape(-1) for c in plans]), dev)      # the one float64 upload
        rows = [p.det_feats for p, m in zip(problems, m_k) if m]
        if on_device:
            feats = [to_dev(r, dev, torch.float32) for r in rows]
            feats = feats[0] if len(feats) == 1 else torch.cat(feats)
        else:
            feats = to_dev(np.concatenate([np.asarray(r, dtype=np.float32) for r in rows]), dev, torch.float32)
        ctx = self.ctx
        # the words that go home: [thr [B, 2] as 4 B words, when computed here] | track_det [B, R] | det_track [B, M] | det_slot [B, M] | solver status [2, B]
        head = 4 * B if data and any(round_k) else 0
        out = torch.empty(head + B * (R + 2 * M) + 2 * B, dtype=torch.int32, device=dev)
        base = out.data_ptr() + 4 * head
        p_track_det, p_det_track, p_det_slot, p_status = base, base + 4 * B * R, base + 4 * B * (R + M), base + 4 * B * (R + 2 * M)
        out[head + B * (R + 2 * M):].zero_()
        d_thr = d_fixed
        slab = None
        scratch = torch.empty(2 * B * (R + M), dtype=torch.int32, device=dev)
        sp = scratch.data_ptr()
        if any(round_k):
            if head:
                d_thr = out[:head].view(torch.float64)
                d_thr.copy_(d_fixed)
            slab = torch.empty(B, R, M, dtype=torch.float64, device=dev)
            E = self.E

            def distance(rows, reduce, lo, hi):                    # the tracks lo .. hi - 1 of the matched rows: a whole group, or both
                groups = (1 if lo == 0 else 0) | (2 if hi == A + I else 0)
                if rows is None:
                    args = (g.gallery.data_ptr(), g.count.data_ptr(), self.capacity, 0, self.budget)
                else:                                              # row i of `rows` is list row lo + i: the table indexed as the slot list starts lo rows before it
                    args = (rows.data_ptr() - 4 * E * lo, None, n_total, 1, 1)
                _mgframe_lib.check(mlib.busca_mgframe_distance(*args, feats.data_ptr(), E, _GHOST_REDUCE[reduce.lower() if isinstance(reduce, str) else reduce],
                                                               groups, *tail, slab.data_ptr(), *where))
            state = dict(mv_avg=g.mv_avg, mv_seen=g.mv_seen)
            _ghost_appearance(ctx, state, g.gallery, d_listed[:A + I], g.count, g.newest, A + I, A, feats, first["cfg"], distance=distance)
            p_tl, p_dl = (d_tl.data_ptr(), d_dl.data_ptr()) if with_labels else (None, None)
            if data:
                if with_labels:                                    # solve_hungarian sees the class-masked matrix
                    _mgframe_lib.check(mlib.busca_mgframe_cost(slab.data_ptr(), None, None, 0.0, p_tl, p_dl, None, *tail, *where))
                    p_tl = p_dl = None
                k_act, k_inact = (0.0, 2.0) if first["every"] else (0.5, 1.0)
                _mgframe_lib.check(mlib.busca_mgframe_thresholds(slab.data_ptr(), k_act, k_inact, 3 if first["data_act"] and first["data_inact"] else 1,
                                                                 *tail, d_thr.data_ptr(), *where))
            if p_tl is not None or blend or first["nan_first"]:
                _mgframe_lib.check(mlib.busca_mgframe_cost(slab.data_ptr(), _lib.ptr(pos) if blend else None, d_boxes.data_ptr(), first["alpha"], p_tl, p_dl,
                                                           d_thr.data_ptr() if first["nan_first"] else None, *tail, *where))

        def solve(k, row, dims):                                   # the rows from slab row `row` on of every problem: [dims[k, 0], m_k] problems
            r2c, c2r = sp + 4 * k * B * (R + M), sp + 4 * (k * B * (R + M) + B * R)
            if slab is not None:
                ctx.check(ctx.lib.busca_linear_assignment(ctx.h, slab.data_ptr() + 8 * row * M, B, R, M, dims.data_ptr(), float(GHOST_LIMIT), r2c, c2r,
                                                          None, None, p_status + 4 * k * B, where[1]))
            return r2c, c2r

        def keep(stage, r2c, c2r, merge, mask):
            _mgframe_lib.check(mlib.busca_mgframe_keep(_lib.ptr(slab), r2c, c2r, d_thr.data_ptr(), p_track_det, p_det_track, stage, merge, mask, *tail,
                                                       *where))
        if not sep:
            keep(0, *solve(0, 0, d_dims1), 0, 0)
        else:
            keep(1, *solve(0, 0, d_dims1), 0, 1 if R > NA else 0)
            if R > NA:
                keep(2, *solve(1, NA, d_dims2), 1, 0)
        if apply:
            _mgframe_lib.check(mlib.busca_mgframe_apply(
                *rings, self.history, g._gallery.data_ptr(), g._count.data_ptr(), g._newest.data_ptr(), g._mv_seen.data_ptr(), self.budget, self.E,
                p_track_det if R else None, p_det_track, feats.data_ptr(), d_boxes.data_ptr(), d_may.data_ptr(), d_free.data_ptr() if f_total else None,
                *tail, p_det_slot, *where))
        host = out.cpu().numpy()                                   # the one device->host copy
        body = host[head:]
        track_det, det_track, det_slot = body[:B * R].reshape(B, R), body[B * R:B * (R + M)].reshape(B, M), body[B * (R + M):B * (R + 2 * M)].reshape(B, M)
        status = body[B * (R + 2 * M):].reshape(2, B)
        for k in range(B):                                         # in the order frame() raises, problem by problem
            if status[:, k].any():
                raise _lib.BuscaError("%s: problem %d: the solver ran out of its loop bounds (status %s) - is a cost -inf?"
                                      % (what, k, status[:, k].tolist()))
        frames = []
        for k, c in enumerate(plans):
            na, ni, m = na_k[k], ni_k[k], m_k[k]
            n = na + ni
            if m == 0:
                frames.append(_no_frame(c["na"], c["n"] - c["na"]))
                continue
            thr = tuple(float(x) for x in (host[4 * k:4 * k + 4].view(np.float64) if head and round_k[k] else c["fixed"]))
            # the words of problem k are its corner of the blocks: the kernels write nothing else, and nothing else is read
            td = np.concatenate([track_det[k, :na], track_det[k, NA:NA + ni]]) if sep else track_det[k, :n]
            dt, ds = det_track[k, :m], det_slot[k, :m]
            matches = [(int(i), int(td[i])) for i in range(n) if td[i] >= 0]
            new, overflow = [], []
            if apply:
                new = [(j, int(ds[j])) for j in range(m) if dt[j] < 0 and ds[j] >= 0]
                overflow = [j for j in range(m) if ds[j] == -2]
            dist = None
            if round_k[k]:
                dist = [slab[k, :na, :m].T, slab[k, NA:NA + ni, :m].T if na > 0 else None] if sep else slab[k, :n, :m].T
            frames.append(GhostFrame(matches, new, overflow, [i for i in range(na) if td[i] < 0], [i for i in range(na, n) if td[i] < 0], thr, dist))
        return frames


GhostFrameProblem = namedtuple("GhostFrameProblem", "active inactive det_feats det_boxes frame det_conf idle free_slots labels warp all_warped",
                               defaults=(None, (), (), None, None, False))
GhostFrameProblem.__doc__ = """One sequence's frame of GhostStore.frame_batch: the arguments of GhostStore.frame with their meaning there, and
  all_warped   every stored row of this sequence has been warped since its last detection was added: what GhostStore.all_warped_after returned
               for its previous step (False at the start) - GhostMotion.all_warped, per sequence"""
