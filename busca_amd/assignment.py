"""Linear assignment on the device and the association rounds that end in it.  Fronts busca_linear_assignment of include/busca_assign.h and
busca_assign_stages of include/busca_assign_stages.h (a chain of assignment problems in one launch);
restates matching.linear_assignment (adapters/ByteTrack/yolox/tracker/matching.py:39-50, lap.lapjv) and min_cost_matching / matching_cascade
(adapters/StrongSORT/deep_sort/linear_assignment.py:15-162).  A device cost matrix is never downloaded: only the match vectors cross."""
import numpy as np
import torch

from . import _lib, geometry
from ._xfer import h2d_async, small_to_dev, stream_of, to_dev
from .kalman import _download_round, _predicted_cost_dev


def _assign_dev(ctx, cost, batch, n, m, limit, dims=None):
    """busca_linear_assignment on a device [batch, n, m] tensor -> device i32 [batch, n + m + 1]: per problem row_to_col, col_to_row and
    the status word, laid out for one copy."""
    if n > _lib.ASSIGN_MAX or m > _lib.ASSIGN_MAX:
        raise ValueError("linear assignment of %d x %d: the device solver takes at most %d rows and columns" % (n, m, _lib.ASSIGN_MAX))
    dev = cost.device
    r2c = torch.empty(batch, n, dtype=torch.int32, device=dev)
    c2r = torch.empty(batch, m, dtype=torch.int32, device=dev)
    status = torch.zeros(batch, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.busca_linear_assignment(ctx.h, cost.data_ptr(), batch, n, m, None if dims is None else dims.data_ptr(), float(limit),
                                              r2c.data_ptr(), c2r.data_ptr(), None, None, status.data_ptr(), stream_of(dev)))
    return torch.cat([r2c, c2r, status.view(batch, 1)], 1)


def _triple(x, y, status, what):
    """matching.linear_assignment's return value (matching.py:44-50) of the two match vectors."""
    if status != 0:
        raise _lib.BuscaError("%s: the solver ran out of its loop bounds (status %d) - is a cost -inf or the limit infinite?" % (what, int(status)))
    rows = np.nonzero(x >= 0)[0]
    matches = np.stack([rows, x[rows]], 1).astype(int) if len(rows) else np.empty((0, 2), dtype=int)
    return matches, np.where(x < 0)[0], np.where(y < 0)[0]


def _empty_triple(n, m):
    return np.empty((0, 2), dtype=int), tuple(range(n)), tuple(range(m))      # matching.py:40-41


def _solved(sol, n, m, what):
    """_triple of one downloaded problem: n row matches, m column matches, the status word."""
    return _triple(sol[:n], sol[n:n + m], sol[n + m], what)


def linear_assignment(cost_matrix, thresh, ctx=None):
    """matching.linear_assignment (adapters/ByteTrack/yolox/tracker/matching.py:39-50; lap.lapjv(cost, extend_cost=True, cost_limit=thresh))
    on the GPU: the partial matching of pairs with cost < thresh that minimises the sum of (cost - thresh).  `cost_matrix`: [n,m] host
    array or device tensor (geometry.pairwise) - a device matrix is never downloaded.  -> (matches [k,2] int sorted by row,
    unmatched_a, unmatched_b) as ndarrays; one device->host copy of n + m + 1 ints."""
    n, m = cost_matrix.shape
    if n == 0 or m == 0:
        return _empty_triple(n, m)
    ctx, dev = geometry.ctx_dev(ctx)
    return _solved(_assign_dev(ctx, to_dev(cost_matrix, dev, torch.float64), 1, n, m, thresh).cpu().numpy()[0], n, m, "linear_assignment")


def linear_assignment_batch(cost_matrices, thresh, ctx=None):
    """linear_assignment of every matrix of a list (host arrays or device tensors, shapes may differ) in ONE launch and one copy back:
    the matrices go into one [batch, max n, max m] slab (the padding is NaN and never read) with their sizes beside them."""
    shapes = [tuple(c.shape) for c in cost_matrices]
    if not shapes:
        return []
    n, m = max(s[0] for s in shapes), max(s[1] for s in shapes)
    if n == 0 or m == 0:
        return [_empty_triple(*s) for s in shapes]
    ctx, dev = geometry.ctx_dev(ctx)
    if any(torch.is_tensor(c) for c in cost_matrices):
        slab = torch.full((len(shapes), n, m), float("nan"), dtype=torch.float64, device=dev)
        for k, c in enumerate(cost_matrices):
            slab[k, :shapes[k][0], :shapes[k][1]] = to_dev(c, dev, torch.float64)
    else:
        host = np.full((len(shapes), n, m), np.nan, dtype=np.float64)
        for k, c in enumerate(cost_matrices):
            host[k, :shapes[k][0], :shapes[k][1]] = c
        slab = torch.from_numpy(host).to(dev)                                  # one upload
    dims = torch.from_numpy(np.asarray(shapes, dtype=np.int32).reshape(-1, 2)).to(dev)
    out = _assign_dev(ctx, slab, len(shapes), n, m, thresh, dims).cpu().numpy()
    res = []
    for k, (nk, mk) in enumerate(shapes):
        res.append(_empty_triple(nk, mk) if nk == 0 or mk == 0 else
                   _triple(out[k, :nk], out[k, n:n + mk], out[k, n + m], "linear_assignment_batch[%d]" % k))
    return res


def _stage_tables_dev(stages, first, again, dev):
    """The three tables of busca_assign_stages as device pointers: the host ones go up in ONE pinned, asynchronous copy (the 16-byte stage records
    first, so that every part stays aligned), device tensors are read in place.  -> (n_stages, stages ptr, first ptr, again ptr or None, the
    tensors to keep alive behind the launch, the number of `first` entries)."""
    keep, ptrs, host = [], {}, []
    if torch.is_tensor(stages):
        stages = stages.to(dev).contiguous()
        nbytes = stages.numel() * stages.element_size()
        if nbytes % 16:
            raise ValueError("assign_stages: a device stage table holds 16-byte records {int32 plane, int32 0, float64 limit}, not %d bytes" % nbytes)
        n_stages = nbytes // 16
        keep.append(stages)
        ptrs["stages"] = stages.data_ptr()
    else:
        recs = [(int(p), float(lim)) for p, lim in stages]
        n_stages = len(recs)
        table = np.zeros(n_stages, dtype=np.dtype([("plane", "<i4"), ("reserved", "<i4"), ("limit", "<f8")]))
        table["plane"] = [p for p, _ in recs]
        table["limit"] = [lim for _, lim in recs]
        host.append(("stages", table.view(np.uint8).reshape(-1)))
    if not 1 <= n_stages <= _lib.ASSIGN_STAGES_MAX:
        raise ValueError("assign_stages: %d stages, 1 .. %d are supported" % (n_stages, _lib.ASSIGN_STAGES_MAX))
    count = None
    for name, x in (("first", first), ("again", again)):
        if x is None:
            ptrs[name] = None
        elif torch.is_tensor(x):
            x = x.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(x)
            ptrs[name] = x.data_ptr()
            count = x.numel() if name == "first" else count
        else:
            x = np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1))
            host.append((name, x.view(np.uint8)))
            count = x.size if name == "first" else count
    if host:
        up = h2d_async(np.concatenate([b for _, b in host]), dev)
        keep.append(up)
        off = 0
        for name, b in host:
            ptrs[name] = up.data_ptr() + off
            off += b.size
    return n_stages, ptrs["stages"], ptrs["first"], ptrs["again"], keep, count


def _assign_stages_dev(ctx, cost, stages, first, again, dims, into=None):
    """busca_assign_stages on a device [batch, planes, n, m] tensor -> flat device i32 tensor row_to_col [batch, n] | col_to_row [batch, m] |
    row_stage [batch, n] | status [batch].  `into`: a contiguous device int32 tensor whose first batch (2 n + m + 1) words receive that instead (a
    caller that sends more words home in the same copy)."""
    batch, planes, n, m = cost.shape
    if n > _lib.ASSIGN_MAX or m > _lib.ASSIGN_MAX:
        raise ValueError("staged assignment of %d x %d: the device solver takes at most %d rows and columns" % (n, m, _lib.ASSIGN_MAX))
    dev = cost.device
    n_stages, p_stages, p_first, p_again, keep, count = _stage_tables_dev(stages, first, again, dev)
    if count != batch * n:
        raise ValueError("assign_stages: %d `first` entries for %d problems of %d rows" % (count, batch, n))
    if again is not None and (again.numel() if torch.is_tensor(again) else np.size(again)) != batch * n:
        raise ValueError("assign_stages: `again` has not %d entries" % (batch * n))
    words = batch * (2 * n + m + 1)
    out = torch.empty(words, dtype=torch.int32, device=dev) if into is None else into
    if batch == 0 or n == 0 or m == 0:                           # nothing is launched: every row and column unmatched, status 0
        out[:words - batch] = -1
        out[words - batch:words] = 0
        return out
    base, o_c2r, o_stage, o_status = out.data_ptr(), 4 * batch * n, 4 * batch * (n + m), 4 * batch * (2 * n + m)
    ctx.check(ctx.lib.busca_assign_stages(ctx.h, cost.data_ptr(), planes, batch, n, m, None if dims is None else dims.data_ptr(), p_stages, n_stages,
                                          p_first, p_again, base, base + o_c2r, base + o_stage, base + o_status, stream_of(dev)))
    del keep                                                     # the caching allocator keeps the blocks until the stream has passed the launch
    return out


def assign_stages(ctx, cost, stages, first, again=None, dims=None):
    """busca_assign_stages (include/busca_assign_stages.h): a chain of assignment problems over one set of rows and columns in ONE launch - stage s
    is linear_assignment, with that stage's limit, of the rows that take part in it against the columns the earlier stages left, ties included.
      cost    device float64 [planes, n, m] or [batch, planes, n, m] (a host array is uploaded)
      stages  a list of (plane, limit) pairs, or a device tensor of 16-byte records {int32 plane, int32 0, float64 limit}; 1 .. 128 stages
      first   [n] / [batch, n] int32: the stage a row takes part in; `again`: the stage it takes part in once more if it is still unmatched then.
              A value outside 0 .. len(stages) - 1, or an again <= first, means never
      dims    None or int32 [batch, 2]: the valid corner of each problem, as in linear_assignment_batch
    Host tables go up in one pinned, asynchronous copy; device tensors are read in place.  Nothing is downloaded: -> a flat device int32 tensor
    row_to_col [batch, n] | col_to_row [batch, m] | row_stage [batch, n] | status [batch] (0 solved, 1 a loop bound ran out, 2 a plane index
    outside the slab; with 1 or 2 that problem's outputs are all -1) - one copy for the caller."""
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(cost, dev, torch.float64)
    if cost.dim() == 3:
        cost = cost.unsqueeze(0)
    if cost.dim() != 4:
        raise ValueError("assign_stages takes a [planes, n, m] or [batch, planes, n, m] cost tensor, not %s" % (tuple(cost.shape),))
    if dims is not None:
        dims = small_to_dev(dims if torch.is_tensor(dims) else np.asarray(dims, dtype=np.int32), dev, torch.int32)
        if dims.numel() != 2 * cost.shape[0]:
            raise ValueError("assign_stages: %d `dims` entries for %d problems" % (dims.numel(), cost.shape[0]))
    return _assign_stages_dev(ctx, cost, stages, first, again, dims)


def min_cost_matching(distance_metric, max_distance, tracks, detections, track_indices=None, detection_indices=None, ctx=None):
    """min_cost_matching (adapters/StrongSORT/deep_sort/linear_assignment.py:15-85) with the solver on the GPU: the metric's matrix (host
    array or device tensor) is clamped on the device (> max_distance becomes max_distance + 1e-5, :61) and solved with that value as the
    limit, so a clamped pair is never matched - the pairs the reference drops afterwards (:80-82).  -> (matches [(track_idx,
    detection_idx)], unmatched_tracks, unmatched_detections) as lists."""
    if track_indices is None:
        track_indices = np.arange(len(tracks))
    if detection_indices is None:
        detection_indices = np.arange(len(detections))
    if len(detection_indices) == 0 or len(track_indices) == 0:
        return [], track_indices, detection_indices  # Nothing to match.
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(distance_metric(tracks, detections, track_indices, detection_indices), dev, torch.float64)
    n, m = cost.shape
    limit = max_distance + 1e-5
    cost = torch.where(cost > max_distance, limit, cost)
    pairs, ua, ub = _solved(_assign_dev(ctx, cost, 1, n, m, limit).cpu().numpy()[0], n, m, "min_cost_matching")
    return ([(track_indices[r], detection_indices[c]) for r, c in pairs], [track_indices[r] for r in ua], [detection_indices[c] for c in ub])


def matching_cascade(distance_metric, max_distance, cascade_depth, tracks, detections, track_indices=None, detection_indices=None, woC=False, ctx=None):
    """matching_cascade (deep_sort/linear_assignment.py:88-162) on tracking.min_cost_matching: level l = 0 .. cascade_depth - 1 matches the tracks
    with time_since_update == 1 + l against the detections the earlier levels left over; `woC` (opt.woC) matches all tracks in one problem instead.
    -> (matches, unmatched_tracks, unmatched_detections); unmatched_tracks comes from a set, as in the reference."""
    if track_indices is None:
        track_indices = list(range(len(tracks)))
    if detection_indices is None:
        detection_indices = list(range(len(detections)))
    unmatched_detections = detection_indices
    matches = []
    if woC:
        levels = [list(track_indices)]
    else:
        levels = [[k for k in track_indices if tracks[k].time_since_update == 1 + level] for level in range(cascade_depth)]
    for level_tracks in levels:
        if not woC and len(unmatched_detections) == 0:      # no detections left
            break
        if not woC and len(level_tracks) == 0:              # nothing to match at this level
            continue
        matches_l, _, unmatched_detections = min_cost_matching(distance_metric, max_distance, tracks, detections, level_tracks, unmatched_detections, ctx=ctx)
        matches += matches_l
    unmatched_tracks = list(set(track_indices) - set(k for k, _ in matches))
    return matches, unmatched_tracks, unmatched_detections


def associate_round(stracks, detections, thresh, det_scores=None, fuse_motion=False, only_position=False, lambda_=0.98, ctx=None):
    """One whole association round on the device: predicted_cost's chain (prediction, predicted boxes, IoU cost with fuse_score, with
    `fuse_motion` the gated blend) followed by linear_assignment(cost, thresh).  The tracks get their predicted `mean` / `covariance`;
    -> (matches, u_track, u_detection) as linear_assignment returns them.  One device->host copy carries the states, the two match
    vectors and the status words; the [n,m] matrix never crosses.  Raises LinAlgError where predicted_cost does."""
    n, m = len(stracks), len(detections)
    if n == 0:
        return _empty_triple(0, m)
    ctx = ctx or geometry.default_context()
    mean, cov, cost, status = _predicted_cost_dev(ctx, stracks, detections, det_scores, fuse_motion, only_position, lambda_)
    sol = None if m == 0 else _assign_dev(ctx, cost.contiguous(), 1, n, m, thresh).to(torch.float64)
    host = _download_round(stracks, mean, cov, sol, status, "associate_round")      # states, match vectors, status words
    return _empty_triple(n, 0) if m == 0 else _solved(host.astype(np.int64), n, m, "associate_round")
