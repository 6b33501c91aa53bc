"""GHOST's association on the device: proxy distances, per-track proxies, data-driven thresholds, the entrywise cost rules and the whole round.
Fronts include/busca_ghost.h (and busca_linear_assignment for the solve); restates adapters/GHOST/src/tracker.py:272-480,
tracking_utils.py:63-126 (get_proxy) and base_tracker.py:101-106,495-531,713-731."""
import numpy as np
import torch

from . import _lib, _store_lib, geometry
from ._xfer import stream_of, to_dev
from .appearance import _check_width, gallery_operands
from .assignment import _assign_dev
from .ghost_motion import ghost_motion_check_config

_GHOST_REDUCE = {"min": _lib.GHOST_MIN, "mean": _lib.GHOST_MEAN, "max": _lib.GHOST_MAX, "midrange": _lib.GHOST_MIDRANGE, "median": _lib.GHOST_MEDIAN,
                 1: _lib.GHOST_MIN, 2: _lib.GHOST_MEAN, 3: _lib.GHOST_MAX, 4: _lib.GHOST_MIDRANGE, 5: _lib.GHOST_MEDIAN}      # tracker_cfg['avg_inact']['num']
_GHOST_PROXY = {"last": _lib.GHOST_PROXY_LAST, "first": _lib.GHOST_PROXY_FIRST, "mean": _lib.GHOST_PROXY_MEAN, "meannorm": _lib.GHOST_PROXY_MEANNORM,
                "median": _lib.GHOST_PROXY_MEDIAN}
GHOST_LIMIT = 8192.0                    # the solver's limit in ghost_round: costs are <= 2 and n, m <= 2048, so one more match always beats any cost


def ghost_distance(track_feats, det_feats, reduce="mean", slot=None, count=None, out=None, ctx=None):
    """busca_ghost_distance: GHOST's proxy_dist (adapters/GHOST/src/tracker.py:278-296) for every track at once - the cosine distance between every
    stored sample of a track and every detection, reduced per track.  `reduce`: 'min', 'mean', 'max', 'midrange' ((max + min) / 2) or 'median'
    (np.median), or the reference's tracker_cfg['avg_inact']['num'] 1 .. 5.  Operands as appearance_cost; 'median' takes a budget of at most 256.
    -> device float64 tensor [n,m], tracks x detections: GHOST's [detections, tracks] matrix is its `.T`.  `out`: a contiguous device [n,m] float64
    tensor (or row block of one) to write into."""
    if isinstance(reduce, str):
        reduce = reduce.lower()
    if reduce not in _GHOST_REDUCE:
        raise ValueError("reduce must be 'min', 'mean', 'max', 'midrange', 'median' or GHOST's num 1 .. 5, not %r" % (reduce,))
    ctx, dev = geometry.ctx_dev(ctx)
    g, slot, count, n = gallery_operands(track_feats, slot, count, dev, "ghost_distance")
    d = to_dev(det_feats, dev, torch.float32)
    if d.dim() != 2:
        raise ValueError("ghost_distance takes [m,E] detection features")
    _check_width(g, d)
    budget, E, m = g.shape[1], g.shape[2], d.shape[0]
    if out is None:
        out = torch.empty(n, m, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (n, m) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 [%d,%d] device tensor" % (n, m))
    ctx.check(ctx.lib.busca_ghost_distance(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), n, budget, d.data_ptr(), m, E, _GHOST_REDUCE[reduce],
                                           out.data_ptr(), stream_of(dev)))
    return out


def ghost_proxies(gallery, mode="mean", window=0, slot=None, count=None, newest=None, ctx=None):
    """busca_ghost_proxies: get_proxy (adapters/GHOST/src/tracking_utils.py:63-126) - one vector per track from its stored samples.
      gallery  [S,budget,E] float32, a ring of `budget` rows per slot; slot / count as appearance_cost
      newest   [S] ints or None: the ring row of every slot's newest sample (None: count - 1)
      mode     'last', 'first' (the oldest stored sample), 'mean', 'meannorm', 'median' (torch.median: the lower one)
      window   the newest `window` samples take part (tracker_cfg['avg_*']['num']); 0 or 'all', or more than a track has: all of them
    torch.mode and the stateful 'mv_avg' are not built here (mv_avg is `mv_avg * a + last * (1 - a)` on a per-track table: ghost_round runs it
    on the table of GhostGallery.state).
    -> device float32 tensor [n,E]; a track without samples gets a row of NaN."""
    if mode in ("mode", "mv_avg"):
        raise NotImplementedError("ghost_proxies: the %r proxy is not built on the device (torch.mode has no kernel here; mv_avg is a stateful "
                                  "moving average - keep it a tensor op of the caller's)" % (mode,))
    if mode not in _GHOST_PROXY:
        raise ValueError("mode must be one of %s, not %r" % (sorted(_GHOST_PROXY), mode))
    window = 0 if window in (None, "all") else int(window)
    ctx, dev = geometry.ctx_dev(ctx)
    g, slot, count, n = gallery_operands(gallery, slot, count, dev, "ghost_proxies")
    S, budget, E = g.shape
    if newest is not None and len(newest) != S:
        raise ValueError("newest has %d entries for %d slots" % (len(newest), S))
    newest = to_dev(newest, dev, torch.int32, flat=True)
    out = torch.empty(n, E, dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.busca_ghost_proxies(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), _lib.ptr(newest), n, budget, E, _GHOST_PROXY[mode], window,
                                          out.data_ptr(), stream_of(dev)))
    return out


def ghost_thresholds(cost, num_active, k_act, k_inact, out=None, ctx=None):
    """busca_ghost_thresholds: update_thresholds (adapters/GHOST/src/base_tracker.py:495-531) on a tracks x detections device matrix whose first
    `num_active` rows are the active tracks: (mean - k_act * std of those rows, mean - k_inact * std of the others), np.std's population std; the
    reference's k are (0, 2) with 'every' and (0.5, 1) with 'tbd'.  -> device float64 tensor [2], never synchronised: hand it to ghost_cost as it is.
    A group without rows keeps its entry of `out` (a new tensor starts at +inf, a threshold nothing exceeds)."""
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(cost, dev, torch.float64)
    n, m = cost.shape
    if out is None:
        out = torch.full((2,), float("inf"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_ghost_thresholds(ctx.h, cost.data_ptr(), n, m, int(num_active), float(k_act), float(k_inact), out.data_ptr(), stream_of(dev)))
    return out


def ghost_cost(app, motion=None, alpha=0.0, track_labels=None, det_labels=None, num_active=None, thr=None, ctx=None):
    """busca_ghost_combine: the entrywise rest of GHOST's cost matrix on a tracks x detections matrix, in the reference's order - entries whose
    track and detection labels differ become NaN (nan_over_classes, tracker.py:272-275 / :299-302), then (1 - alpha) * app + alpha * motion
    (combine_motion_appearance with combi 'sum_<alpha>', base_tracker.py:713-731), then entries that are not <= thr[0] (the first `num_active` rows)
    / thr[1] (the others) become NaN (nan_first, tracker.py:392-396).  Every part is optional.  `thr`: two numbers or a device float64 [2] tensor
    (ghost_thresholds).  -> a new device float64 tensor [n,m]."""
    ctx, dev = geometry.ctx_dev(ctx)
    app = to_dev(app, dev, torch.float64)
    n, m = app.shape
    if motion is not None:
        motion = to_dev(motion, dev, torch.float64)
        if tuple(motion.shape) != (n, m):
            raise ValueError("the motion cost is %s, the appearance cost %s: both are tracks x detections" % (tuple(motion.shape), (n, m)))
    if (track_labels is None) != (det_labels is None):
        raise ValueError("track_labels and det_labels go together")
    tl, dl = to_dev(track_labels, dev, torch.int32, flat=True), to_dev(det_labels, dev, torch.int32, flat=True)
    if tl is not None and (tl.numel() != n or dl.numel() != m):
        raise ValueError("%d track labels and %d detection labels for a %d x %d matrix" % (tl.numel(), dl.numel(), n, m))
    if thr is not None and not torch.is_tensor(thr):
        thr = np.asarray(thr, dtype=np.float64).reshape(2)
    thr = to_dev(thr, dev, torch.float64)
    out = torch.empty(n, m, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_ghost_combine(ctx.h, app.data_ptr(), _lib.ptr(motion), n, m, float(alpha), _lib.ptr(tl), _lib.ptr(dl),
                                          n if num_active is None else int(num_active), _lib.ptr(thr), out.data_ptr(), stream_of(dev)))
    return out


def ghost_check_config(cfg):
    """Refuse the tracker_cfg branches that do not work in the reference either, and the ones that are not built; returns cfg."""
    if cfg.get("use_bism", False):
        raise ValueError("GHOST use_bism is refused: the reference crashes in this branch (bisoftmax already returns a numpy array and dist() calls "
                         ".numpy() on it, base_tracker.py:105-106), so there is nothing to reproduce")
    if cfg.get("distance", "cosine") != "cosine":
        raise ValueError("GHOST distance %r is refused: only 'cosine' works in the reference (the other branch applies F.pairwise_distance to the "
                         "broadcast [m, E, g] tensor, takes the norm over the gallery axis and returns [m, E], base_tracker.py:101)" % (cfg["distance"],))
    return cfg


def _ghost_get(state, name, default=None):
    return state.get(name, default) if isinstance(state, dict) else getattr(state, name, default)


def _ghost_mv_avg_table(state, entry, what):
    """The (mv_avg, mv_seen) tensors of `state` for a group whose proxy is 'mv_avg'; refuses what cannot run before anything is written."""
    table, seen = _ghost_get(state, "mv_avg"), _ghost_get(state, "mv_seen")
    if table is None or seen is None:
        raise NotImplementedError("ghost_round: %s proxy 'mv_avg' needs the per-track table `mv_avg` / `mv_seen` in `state`: build the state "
                                  "with GhostGallery.state" % what)
    if entry.get("num", "all") == "all":
        raise ValueError("ghost_round: %s proxy 'mv_avg' takes a number as 'num': with 'all' the reference raises TypeError "
                         "(mv_avg[i] * 'all', tracking_utils.py:88)" % what)
    return table, seen


def _ghost_mv_avg_rows(ctx, g, count, newest, slot, a, table, seen, num_active=None):
    """get_proxy's 'mv_avg' branch (tracking_utils.py:83-89) on the state's own table: a track seen before gets mv_avg * a + last * (1 - a), a new
    one its newest sample, and either way that vector becomes the track's mv_avg.  `a`: the weight of the group, or (a_act, a_inact) for the
    first `num_active` rows and the others - one pass over both groups.  One busca_store_mv_avg launch on torch's current stream (include/
    busca_store.h): it reads the newest ring row itself and blends in float32 in the reference's order - two products and one sum, each rounded,
    nothing contracted, the weights (float)a and (float)(1 - a) as torch forms them from a Python scalar - so the bits are torch CPU's.  A row with
    a skipped slot or without samples is NaN and leaves the table untouched.  No synchronising call; the valid slots of a call are distinct."""
    if not (torch.is_tensor(table) and torch.is_tensor(seen) and table.device == g.device and seen.device == g.device and table.dtype == torch.float32
            and tuple(table.shape) == (g.shape[0], g.shape[2]) and tuple(seen.shape) == (g.shape[0],)
            and seen.dtype in (torch.uint8, torch.bool) and table.is_contiguous() and seen.is_contiguous()):
        raise ValueError("ghost_round: mv_avg / mv_seen must be the device tensors of GhostGallery.state: float32 [%d,%d] and [%d] flags"
                         % (g.shape[0], g.shape[2], g.shape[0]))
    n = slot.numel()
    a_act, a_inact = a if isinstance(a, tuple) else (a, a)
    out = torch.empty(n, g.shape[2], dtype=torch.float32, device=g.device)
    _store_lib.check(_store_lib.load().busca_store_mv_avg(
        g.data_ptr(), _lib.ptr(count), _lib.ptr(newest), table.data_ptr(), seen.data_ptr(), g.shape[0], g.shape[1], g.shape[2], slot.data_ptr(), n,
        n if num_active is None else int(num_active), float(a_act), float(a_inact), out.data_ptr(), g.device.index, stream_of(g.device)))
    return out


def _ghost_proxy_rows(ctx, g, count, newest, slot, entry, what, state=None):
    """get_proxy's choice for one group of tracks (tracker_cfg['avg_act'] / ['avg_inact']) -> device [k,E] float32."""
    proxy, num = entry.get("proxy", "last"), entry.get("num", "all")
    if not entry.get("do", False) or proxy == "last":            # without 'do', track.feats: the newest sample
        mode, window = "last", 0
    elif num == "first":
        mode, window = "first", 0
    elif proxy == "mv_avg":
        table, seen = _ghost_mv_avg_table(state, entry, what)
        return _ghost_mv_avg_rows(ctx, g, count, newest, slot, float(num), table, seen)
    elif proxy == "mode" or proxy not in _GHOST_PROXY:
        raise NotImplementedError("ghost_round: %s proxy %r is not built on the device" % (what, proxy))
    else:
        mode, window = proxy, (0 if num == "all" else int(num))
    return ghost_proxies(g, mode, window, slot=slot, count=count, newest=newest, ctx=ctx)


def _ghost_threshold_plan(cfg):
    """tracker_cfg's two thresholds -> (act, inact, every, data_act, data_inact): the entries as given, whether 'every' rules, and which of the
    two is computed from the frame's distances.  Raises what ghost_round raises for entries the reference cannot run."""
    at, it = cfg.get("act_reid_thresh"), cfg.get("inact_reid_thresh")
    every, tbd = at == "every", at == "tbd"
    for name, v in (("act_reid_thresh", at), ("inact_reid_thresh", it)):
        if isinstance(v, str) and v not in ("every", "tbd"):
            raise ValueError("%s must be a number, 'every' or 'tbd', not %r" % (name, v))
    data_act, data_inact = every or tbd, every or it == "tbd"
    if it == "tbd" and not (every or tbd):
        raise ValueError("inact_reid_thresh 'tbd' needs act_reid_thresh 'tbd' or 'every': the reference leaves it a string otherwise (base_tracker.py:515-531)")
    return at, it, every, data_act, data_inact


def _ghost_blend_plan(cfg):
    """tracker_cfg['motion_config'] -> (motion_config, whether the motion cost is blended in, its weight alpha of combi 'sum_<alpha>')."""
    mcfg = cfg.get("motion_config", {})
    blend = bool(mcfg.get("apply_motion_model", False))
    alpha = 0.0
    if blend:
        combi = str(mcfg.get("combi", ""))
        if "sum" not in combi:
            raise NotImplementedError("ghost_round: motion_config combi %r is not built; only 'sum_<alpha>'" % (combi,))
        alpha = float(combi.split("_")[-1])
    return mcfg, blend, alpha


def _ghost_appearance(ctx, state, g, slot, count, newest, n, na, d, cfg, distance=None):
    """The first half of ghost_round, which GhostStore.frame runs too: the proxy and distance launches of both groups of tracks -> (app, each): the
    device float64 [n,m] appearance matrix, tracks x detections, and whether the per-sample route ran.  `slot`: device int32 [n], ACTIVE TRACKS
    FIRST; `d`: device float32 [m,E].  Both groups' mv_avg entries are checked before either writes its table.
    `distance(rows, reduce, lo, hi)`: what receives the distance launch of the tracks lo .. hi - 1 - `rows` their [hi - lo, E] proxy vectors, or None:
    their samples in the gallery, reduced with `reduce` - in place of busca_ghost_distance into `app` (which is then None): GhostStore.frame_batch
    writes the diagonal blocks of a batch with it."""
    dev = g.device
    act, inact = cfg.get("avg_act", {}), cfg.get("avg_inact", {})
    each = inact.get("proxy") == "each_sample"
    app = None
    if distance is None:
        app = torch.empty(n, d.shape[0], dtype=torch.float64, device=dev)

        def distance(rows, reduce, lo, hi):
            if rows is None:
                ghost_distance(g, d, reduce, slot=slot[lo:hi], count=count, out=app[lo:hi], ctx=ctx)
            else:
                ghost_distance(rows, d, reduce, out=app[lo:hi], ctx=ctx)
    def kind(entry):                                              # what a group of tracks runs: its rows depend on nothing else
        if each:
            return ("samples", inact.get("num", 2)) if entry.get("do", False) else ("last",)
        return ("proxy", entry.get("proxy", "last"), entry.get("num", "all")) if entry.get("do", False) else ("last",)
    for entry, what in ((act, "avg_act"), (inact, "avg_inact")):  # both groups' mv_avg entries are checked before either writes its table
        if kind(entry)[:2] == ("proxy", "mv_avg") and entry.get("num", "all") != "first":
            _ghost_mv_avg_table(state, entry, what)
    groups = ((0, n, inact, "avg_inact"),) if kind(act) == kind(inact) else ((0, na, act, "avg_act"), (na, n, inact, "avg_inact"))      # one launch where both groups run the same
    if len(groups) == 2 and kind(act)[:2] == kind(inact)[:2] == ("proxy", "mv_avg") and "first" not in (act.get("num"), inact.get("num")):
        # both groups blend, each with its own weight: one pass over all rows instead of two
        rows = _ghost_mv_avg_rows(ctx, g, count, newest, slot, (float(act["num"]), float(inact["num"])), *_ghost_mv_avg_table(state, act, "avg_act"), num_active=na)
        distance(rows, "min", 0, n)
        groups = ()
    for lo, hi, entry, what in groups:
        if hi == lo:
            continue
        if each and entry.get("do", False):                       # proxy_dist over the track's samples; both groups reduce with avg_inact['num']
            distance(None, inact.get("num", 2), lo, hi)
        else:                                                     # one vector per track (last_frame, or get_proxy), then the plain cosine distance
            entry = {"do": False} if each else entry
            distance(_ghost_proxy_rows(ctx, g, count, newest, slot[lo:hi], entry, what, state), "min", lo, hi)
    return app, each


def ghost_round(state, det_feats, labels=None, motion=None, cfg=None, sep=None, thresholds=None, ctx=None, det_boxes=None):
    """GHOST's association round without leaving the device: get_hungarian_each_sample / get_hungarian_with_proxy + solve_hungarian
    (adapters/GHOST/src/tracker.py:306-480) from the tracks' sample galleries and the detections' features in HBM to the matches on the host.
      state       the tracks: a dict or object with `gallery` [S,budget,E] float32 (host array or device tensor), `count` [S] and `newest` [S] (or None,
                  as ghost_proxies), `slot` [n] or None - the gallery slot of track i, ACTIVE TRACKS FIRST - and `num_active`; GhostGallery.state
                  builds it, with the tables `mv_avg` [S,E] / `mv_seen` [S] the 'mv_avg' proxy reads AND UPDATES, once per group per call
      det_feats   [m,E] float32, host array or device tensor
      labels      (track_labels [n], det_labels [m]) or None; as in the reference only the each_sample route masks classes
      motion      [n,m] tracks x detections motion cost (host array or device tensor); needed when motion_config['apply_motion_model'],
                  unless `state` carries `motion_state`, a GhostMotion whose slots are the gallery's, and `det_boxes` [m,4] tlbr is given: the round
                  then runs the motion model itself (GhostMotion.cost with motion_config['last_n_frames']; it advances the positions, so once
                  per frame, as the reference calls motion() in its round)
      cfg         the reference's tracker_cfg: 'avg_act' / 'avg_inact' {'do', 'num', 'proxy'}, 'act_reid_thresh' / 'inact_reid_thresh' (numbers,
                  'every' or 'tbd'), 'nan_first', 'assign_separately', 'motion_config' {'apply_motion_model', 'combi': 'sum_<alpha>'},
                  'distance', 'use_bism'.  avg_inact['proxy'] == 'each_sample' selects the per-sample route, whose reduction is avg_inact['num'] 1 .. 5
      sep         overrides cfg['assign_separately']: solve the active tracks only, as solve_hungarian does
      thresholds  a device float64 [2] tensor to hold (act, inact): fixed thresholds are written into it, data-driven ones computed into it on
                  the device - a 'tbd' caller reads it back once and passes numbers from then on
    -> (dist, row, col): `dist` the device cost matrix in GHOST's [detections, tracks] orientation (a transposed view; with `sep` the list
    [dist_act, dist_inact] the reference returns, dist_inact None without active tracks), `row` / `col` the matched detection / track indices as
    host int arrays, sorted by detection.  One device->host copy of n + m + 1 ints; the post-filters assign_act_inact_same_time / assign_separatly
    stay host code reading `row`, `col` and `dist`.

    The solve is busca_linear_assignment with limit 8192: every cost is <= 2 and there are at most 2048 rows, so a matching with one more pair
    always wins and among those the cheapest does - a maximum-cardinality minimum-cost matching over the non-NaN entries (NaN is never
    admissible).  The reference calls lapsolver.solve_dense, whose behaviour on a matrix with infeasible rows is third-party and unpinned here: where
    every detection can be matched the two agree; elsewhere this is the documented rule."""
    cfg = ghost_check_config(dict(cfg or {}))
    ctx, dev = geometry.ctx_dev(ctx)
    g, slot, count, n = gallery_operands(_ghost_get(state, "gallery"), _ghost_get(state, "slot"), _ghost_get(state, "count"), dev, "ghost_round")
    newest = to_dev(_ghost_get(state, "newest"), dev, torch.int32, flat=True)
    na = _ghost_get(state, "num_active")
    na = n if na is None else int(na)
    if not 0 <= na <= n:
        raise ValueError("num_active %d outside 0 .. %d" % (na, n))
    d = to_dev(det_feats, dev, torch.float32)
    m = d.shape[0]
    sep = bool(cfg.get("assign_separately", False)) if sep is None else bool(sep)
    empty = np.empty(0, dtype=np.int64)
    if n == 0 or m == 0:
        return torch.empty(m, n, dtype=torch.float64, device=dev), empty, empty
    if slot is None:
        slot = torch.arange(n, dtype=torch.int32, device=dev)
    app, each = _ghost_appearance(ctx, state, g, slot, count, newest, n, na, d, cfg)
    tl = dl = None
    if each and labels is not None and cfg.get("nan_over_classes", True):
        tl, dl = labels
    at, it, every, data_act, data_inact = _ghost_threshold_plan(cfg)
    mcfg, blend, alpha = _ghost_blend_plan(cfg)
    if blend:
        mstate = _ghost_get(state, "motion_state")
        if motion is None and mstate is not None and det_boxes is not None:
            ghost_motion_check_config(mcfg, cfg.get("kalman", False))
            mslot = _ghost_get(state, "slot")
            motion = mstate.cost(slot if mslot is None or torch.is_tensor(mslot) else mslot, na, det_boxes, mcfg.get("last_n_frames", 100000000))
        if motion is None:
            raise ValueError("motion_config applies a motion model: pass the [n,m] motion cost")
    nan_first = bool(cfg.get("nan_first", False))
    thr = None
    if nan_first or data_act or data_inact:
        fixed = [float("inf") if isinstance(v, str) or v is None else float(v) for v in (at, it)]
        host_thr = torch.from_numpy(np.asarray(fixed, dtype=np.float64))
        if thresholds is None:
            thr = host_thr.to(dev)
        else:
            thr = thresholds
            thr.copy_(host_thr)
    if data_act or data_inact:
        if tl is not None:                                        # solve_hungarian sees the class-masked matrix
            app = ghost_cost(app, track_labels=tl, det_labels=dl, ctx=ctx)
            tl = dl = None
        k_act, k_inact = (0.0, 2.0) if every else (0.5, 1.0)
        if data_act and data_inact:
            ghost_thresholds(app, na, k_act, k_inact, out=thr, ctx=ctx)
        elif na > 0:                                              # the active threshold only: over the active rows alone
            ghost_thresholds(app[:na], na, k_act, k_inact, out=thr, ctx=ctx)
    if tl is not None or blend or nan_first:
        cost = ghost_cost(app, motion if blend else None, alpha, tl, dl, na, thr if nan_first else None, ctx=ctx)
    else:
        cost = app
    rows = na if sep else n
    if rows == 0:
        row = col = empty
    else:
        sol = _assign_dev(ctx, cost, 1, rows, m, GHOST_LIMIT).cpu().numpy()[0]      # the leading `rows` rows of the contiguous matrix are a [rows,m] problem
        if sol[rows + m] != 0:
            raise _lib.BuscaError("ghost_round: the solver ran out of its loop bounds (status %d) - is a cost -inf?" % int(sol[rows + m]))
        c2r = sol[rows:rows + m].astype(np.int64)
        row = np.nonzero(c2r >= 0)[0]
        col = c2r[row]
    if sep:
        return [cost[:na].T, cost[na:].T if na > 0 else None], row, col
    return cost.T, row, col
