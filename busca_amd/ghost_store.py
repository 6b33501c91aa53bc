"""GHOST's frame on resident track state as one chain.  Fronts include/busca_gframe.h (libbusca_gframe.so, bound by _gframe_lib) around the proxy
and distance launches of ghost_round (include/busca_ghost.h) and busca_linear_assignment; restates Tracker._track without the BUSCA round
(adapters/GHOST/src/tracker.py:203-261): motion_compensation's loop and BaseTracker.motion (base_tracker.py:600-698), get_hungarian_* and
solve_hungarian (tracker.py:306-480), assign_act_inact_same_time / assign_separatly (tracker.py:597-682) and Track.add_detection / Track.__init__
(tracking_utils.py:254-370)."""
from collections import namedtuple

import numpy as np
import torch

from . import _gframe_lib, _lib, geometry
from ._xfer import h2d_async, stream_of, to_dev
from .ghost import (GHOST_LIMIT, _GHOST_PROXY, _ghost_appearance, _ghost_blend_plan, _ghost_mv_avg_table, _ghost_threshold_plan, ghost_check_config,
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

    def _frame_checked(self, active, inactive, idle, free_slots, det_feats, det_boxes, det_conf, labels, warp, thresholds, cfg):
        """The host side of frame(), before anything is allocated, enqueued or written -> the plan as a dict."""
        what = "GhostStore.frame"
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
