"""Proposal-side geometry with the reference's names and semantics (busca/tracking.py), computed by the
HIP kernels behind the C-ABI (busca_pairwise / busca_crop_gather / busca_appearance_cost).  Inputs and outputs are host numpy
arrays exactly like the reference; there is no CPU implementation here."""
import os

import numpy as np
import torch

from . import _lib, geometry
from .crop_pool import Slot

_F32_MIN = np.finfo("float32").min


def missing_candidate_bbox(seq_len=None, flavour="ltrb", pinned_numpy=True):
    """Sentinel box of a padded candidate (busca/tracking.py:7-20).  `pinned_numpy=True` reproduces the
    reference's pinned numpy 1.23.5, where np.float32 / 100.0 is float64 and the array therefore float64."""
    dt = np.float64 if pinned_numpy else np.float32
    m = dt(_F32_MIN)
    if flavour == "ltrb":
        bbox = np.array([m, m, m / dt(100.0), m / dt(100.0)], dtype=dt)
    elif flavour == "ltwh":
        bbox = np.array([m, m, -m / dt(100.0), -m / dt(100.0)], dtype=dt)
    else:
        raise ValueError("Unknown flavour: {}".format(flavour))
    if seq_len is not None:
        bbox = np.tile(bbox, (seq_len, 1))
    return bbox


def _tlbrs(items):
    if len(items) > 0 and isinstance(items[0], np.ndarray):
        return np.asarray(items, dtype=np.float64).reshape(-1, 4)
    return np.array([t.tlbr for t in items], dtype=np.float64).reshape(-1, 4)


def center_distance(atracks, btracks, weight_size=False, ctx=None):
    """Centre-to-centre distance matrix [len(a), len(b)] float64 (busca/tracking.py:23-60); accepts track
    objects (`.tlbr`) or ndarrays.  Empty input -> zeros (the reference's np.float alias is float64)."""
    a, b = _tlbrs(atracks), _tlbrs(btracks)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(atracks), len(btracks)), dtype=np.float64)
    ctx = ctx or geometry.default_context()
    mode = _lib.PAIR_CENTER_WEIGHTED if weight_size else _lib.PAIR_CENTER
    return geometry.pairwise_host(ctx, a, b, mode)


def iou_distance(atlbrs, btlbrs, det_scores=None, ctx=None):
    """1 - IoU cost matrix with the '+1' pixel convention of cython_bbox (adapters/ByteTrack/yolox/tracker/
    matching.py:53-91); with `det_scores` also applies fuse_score (:173-186)."""
    a, b = _tlbrs(atlbrs), _tlbrs(btlbrs)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), dtype=np.float64)
    ctx = ctx or geometry.default_context()
    return geometry.pairwise_host(ctx, a, b, _lib.PAIR_IOU_COST, scores_b=det_scores)

TRACKED = 1     # TrackState.Tracked (adapters/*/mot_online/basetrack.py:5-9)


def multi_predict(stracks, ctx=None):
    """STrack.multi_predict (adapters/ByteTrack/yolox/tracker/byte_tracker.py:50-61) on the GPU: constant-velocity Kalman
    prediction of every track's (mean [8], covariance [8,8]) in place; `mean[7]` of non-Tracked tracks is zeroed first."""
    if len(stracks) == 0:
        return
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    mean = torch.from_numpy(np.asarray([st.mean for st in stracks], dtype=np.float64)).to(dev)
    cov = torch.from_numpy(np.asarray([st.covariance for st in stracks], dtype=np.float64)).to(dev)
    nt = torch.from_numpy(np.asarray([st.state != TRACKED for st in stracks], dtype=np.uint8)).to(dev)
    ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, mean.data_ptr(), cov.data_ptr(), nt.data_ptr(), len(stracks),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    both = torch.cat([mean, cov.view(len(stracks), 64)], 1).cpu().numpy()       # one device->host copy for both
    mean, cov = np.ascontiguousarray(both[:, :8]), np.ascontiguousarray(both[:, 8:]).reshape(-1, 8, 8)
    for i, st in enumerate(stracks):
        st.mean = mean[i]
        st.covariance = cov[i]


CHI2INV95 = {2: 5.9915, 4: 9.4877}      # kalman_filter.py:10-19, the gates of only_position=True / False


def tlwh_to_xyah(tlwh):
    """STrack.tlwh_to_xyah (byte_tracker.py:165-172) of [n,4] boxes: (centre x, centre y, width / height, height)."""
    ret = np.array(tlwh, dtype=np.float64).reshape(-1, 4)
    ret[:, :2] += ret[:, 2:] / 2
    ret[:, 2] /= ret[:, 3]
    return ret


def _measurements(detections):
    """[m,4] float64 (x, y, a, h): an ndarray is taken as measurements already (what KalmanFilter.gating_distance takes),
    detection objects give tlwh_to_xyah(det.tlwh) as `det.to_xyah()` does."""
    if isinstance(detections, np.ndarray):
        return np.ascontiguousarray(detections, dtype=np.float64).reshape(-1, 4)
    return tlwh_to_xyah([d.tlwh for d in detections])


def _upload_states(stracks, dev):
    mean = torch.from_numpy(np.asarray([st.mean for st in stracks], dtype=np.float64).reshape(-1, 8)).to(dev)
    cov = torch.from_numpy(np.asarray([st.covariance for st in stracks], dtype=np.float64).reshape(-1, 8, 8)).to(dev)
    return mean, cov


def _raise_flagged(status, what):
    bad = np.nonzero(status)[0]
    if len(bad):
        raise np.linalg.LinAlgError("%s: the projected covariance of track %d is not positive definite (%d of %d tracks)"
                                    % (what, int(bad[0]), len(bad), len(status)))


def multi_update(stracks, detections, ctx=None):
    """The Kalman step of STrack.update / re_activate (byte_tracker.py:78,109) for every matched pair at once:
    `stracks[i].mean / .covariance` become KalmanFilter.update(mean, covariance, tlwh_to_xyah(detections[i].tlwh))
    (kalman_filter.py:193-225).  Ids, memories and states stay with the tracker.  Where the reference raises LinAlgError (a
    projected covariance that is not positive definite) this raises it too, naming the first such track - after every other
    track of the call has been updated; the flagged ones keep their state."""
    if len(stracks) != len(detections):
        raise ValueError("multi_update pairs track i with detection i: got %d tracks and %d detections" % (len(stracks), len(detections)))
    n = len(stracks)
    if n == 0:
        return
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    mean, cov = _upload_states(stracks, dev)
    meas = torch.from_numpy(_measurements(detections)).to(dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.busca_kalman_update(ctx.h, mean.data_ptr(), cov.data_ptr(), meas.data_ptr(), n, status.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    both = torch.cat([mean, cov.view(n, 64), status.to(torch.float64).view(n, 1)], 1).cpu().numpy()     # one device->host copy for all three
    mean, cov = np.ascontiguousarray(both[:, :8]), np.ascontiguousarray(both[:, 8:72]).reshape(-1, 8, 8)
    for i, st in enumerate(stracks):
        st.mean = mean[i]
        st.covariance = cov[i]
    _raise_flagged(both[:, 72], "multi_update")


def multi_initiate(detections, ctx=None):
    """KalmanFilter.initiate (kalman_filter.py:54-85) of every new detection, as STrack.activate calls it (byte_tracker.py:67):
    -> (mean [n,8], covariance [n,8,8]) float64."""
    meas = _measurements(detections)
    n = meas.shape[0]
    if n == 0:
        return np.zeros((0, 8)), np.zeros((0, 8, 8))
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    z = torch.from_numpy(meas).to(dev)
    both = torch.empty(n * 72, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_kalman_initiate(ctx.h, z.data_ptr(), n, both.data_ptr(), both.data_ptr() + 64 * n,
                                            torch.cuda.current_stream(dev).cuda_stream))
    host = both.cpu().numpy()
    return host[:8 * n].reshape(n, 8).copy(), host[8 * n:].reshape(n, 8, 8).copy()


_METRICS = {"maha": 0, "gaussian": 1}


def _gating_dev(ctx, mean, cov, meas, only_position, metric):
    """Device [n,m] gating distances and the [n] int32 status words of device states and measurements."""
    n, m = mean.shape[0], meas.shape[0]
    out = torch.empty(n, m, dtype=torch.float64, device=mean.device)
    status = torch.zeros(n, dtype=torch.int32, device=mean.device)
    ctx.check(ctx.lib.busca_kalman_gating(ctx.h, mean.data_ptr(), cov.data_ptr(), n, meas.data_ptr(), m, int(bool(only_position)), metric,
                                          out.data_ptr(), status.data_ptr(), torch.cuda.current_stream(mean.device).cuda_stream))
    return out, status


def _download_with_status(mat, status, what):
    """One device->host copy of a [n,m] matrix and its tracks' status words."""
    n, m = mat.shape
    host = torch.cat([mat.reshape(-1), status.to(torch.float64)]).cpu().numpy()
    _raise_flagged(host[n * m:], what)
    return host[:n * m].reshape(n, m).copy()


def gating_distance(stracks, detections, only_position=False, metric="maha", ctx=None):
    """KalmanFilter.gating_distance (kalman_filter.py:227-269) of every track against every detection: [n,m] float64, the
    squared Mahalanobis ('maha') or squared Euclidean ('gaussian') distance between the track's projected state and
    the detection's (x, y, a, h) - (x, y) only with `only_position`.  `detections`: objects with `.tlwh`, or an [m,4] array
    of measurements.  Raises LinAlgError where np.linalg.cholesky does in the reference."""
    if metric not in _METRICS:
        raise ValueError("invalid distance metric")
    meas = _measurements(detections)
    n, m = len(stracks), meas.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    mean, cov = _upload_states(stracks, dev)
    out, status = _gating_dev(ctx, mean, cov, torch.from_numpy(meas).to(dev), only_position, _METRICS[metric])
    return _download_with_status(out, status, "gating_distance")


def _gate_dev(cost, gate, only_position, lambda_, gated=float("inf")):
    """matching.py:141 / :154-155 on device tensors: `gated` (inf) above the chi-square gate, then (fuse_motion) the blend."""
    cost = torch.where(gate > CHI2INV95[2 if only_position else 4], gated, cost)
    if lambda_ is not None:
        cost = lambda_ * cost + (1 - lambda_) * gate
    return cost


def _gated(cost, stracks, detections, only_position, lambda_, ctx, what):
    n, m = len(stracks), len(detections)
    if n == 0 or m == 0:                                       # `if cost_matrix.size == 0: return cost_matrix`
        return cost.cpu().numpy() if torch.is_tensor(cost) else cost
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    if not torch.is_tensor(cost):
        cost = torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float64))
    cost = cost.to(device=dev, dtype=torch.float64).reshape(n, m)
    mean, cov = _upload_states(stracks, dev)
    gate, status = _gating_dev(ctx, mean, cov, torch.from_numpy(_measurements(detections)).to(dev), only_position, 0)
    return _download_with_status(_gate_dev(cost, gate, only_position, lambda_), status, what)


def gate_cost_matrix(cost, stracks, detections, only_position=False, ctx=None):
    """matching.gate_cost_matrix (adapters/ByteTrack/yolox/tracker/matching.py:132-142): entries whose squared Mahalanobis
    distance exceeds chi2inv95[4] = 9.4877 (chi2inv95[2] = 5.9915 with `only_position`) become inf.  `cost`: [n,m] host array
    or a device tensor (geometry.pairwise) - the gate is applied on the device either way.  Returns a new host array."""
    return _gated(cost, stracks, detections, only_position, None, ctx, "gate_cost_matrix")


def fuse_motion(cost, stracks, detections, only_position=False, lambda_=0.98, ctx=None):
    """matching.fuse_motion (matching.py:145-156): the gate of gate_cost_matrix, then lambda_ * cost + (1 - lambda_) * distance.
    Gating distances, gate and blend all stay on the device; one device->host copy of the result."""
    return _gated(cost, stracks, detections, only_position, float(lambda_), ctx, "fuse_motion")


def _predicted_cost_dev(ctx, stracks, detections, det_scores, fuse_motion, only_position, lambda_):
    """The device part of an association round: predicted states, then (m > 0) their IoU cost against the detections and, with
    `fuse_motion`, the gated blend.  -> (mean [n,8], cov [n,8,8], cost [n,m] or None, Kalman status [n] i32 or None), all device tensors."""
    n, m = len(stracks), len(detections)
    dev = torch.device("cuda", ctx.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    mean, cov = _upload_states(stracks, dev)
    nt = torch.from_numpy(np.asarray([st.state != TRACKED for st in stracks], dtype=np.uint8)).to(dev)
    ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, mean.data_ptr(), cov.data_ptr(), nt.data_ptr(), n, stream))
    cost = status = None
    if m > 0:
        boxes = torch.empty(n, 4, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, mean.data_ptr(), n, 1, boxes.data_ptr(), stream))
        cost = geometry.pairwise(ctx, boxes, _tlbrs(detections), _lib.PAIR_IOU_COST, scores_b=det_scores)
        if fuse_motion:
            gate, status = _gating_dev(ctx, mean, cov, torch.from_numpy(_measurements(detections)).to(dev), only_position, 0)
            cost = _gate_dev(cost, gate, only_position, float(lambda_))
    return mean, cov, cost, status


def _set_states(stracks, host):
    """The tracks' predicted states from the leading 72 n doubles of a downloaded round."""
    n = len(stracks)
    pm, pc = host[:8 * n].reshape(n, 8).copy(), host[8 * n:72 * n].reshape(n, 8, 8).copy()
    for i, st in enumerate(stracks):
        st.mean = pm[i]
        st.covariance = pc[i]


def predicted_cost(stracks, detections, det_scores=None, fuse_motion=False, only_position=False, lambda_=0.98, ctx=None):
    """One association round's cost matrix without leaving the device: STrack.multi_predict (busca_kalman_multi_predict) ->
    the predicted boxes (busca_kalman_boxes, tlbr) -> iou_distance, with fuse_score when `det_scores` is given (busca_pairwise
    IOU_COST) -> with `fuse_motion`, matching.fuse_motion on the predicted states (busca_kalman_gating + gate + blend).
    The tracks get their predicted `mean` / `covariance` as multi_predict gives them; the [n,m] cost matrix comes back in the
    same single device->host copy.  `detections`: objects with `.tlbr` and `.tlwh`."""
    n, m = len(stracks), len(detections)
    if n == 0:
        return np.zeros((0, m), dtype=np.float64)
    ctx = ctx or geometry.default_context()
    mean, cov, cost, status = _predicted_cost_dev(ctx, stracks, detections, det_scores, fuse_motion, only_position, lambda_)
    parts = [mean.view(-1), cov.view(-1)]
    if m > 0:
        parts.append(cost.view(-1))
        if fuse_motion:
            parts.append(status.to(torch.float64))
    host = torch.cat(parts).cpu().numpy()                        # one device->host copy: states, cost matrix, status words
    _set_states(stracks, host)
    if m == 0:
        return np.zeros((n, 0), dtype=np.float64)
    if fuse_motion:
        _raise_flagged(host[72 * n + n * m:], "predicted_cost")
    return host[72 * n:72 * n + n * m].reshape(n, m).copy()


# ---- linear assignment (include/busca_assign.h) ------------------------------------------------------------------------------
def _cost_to_dev(cost, dev):
    """A contiguous float64 device tensor of a host array or a tensor (a device float64 tensor is taken as it is)."""
    if not torch.is_tensor(cost):
        cost = torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float64))
    return cost.to(device=dev, dtype=torch.float64).contiguous()


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
                                              r2c.data_ptr(), c2r.data_ptr(), None, None, status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
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


def linear_assignment(cost_matrix, thresh, ctx=None):
    """matching.linear_assignment (adapters/ByteTrack/yolox/tracker/matching.py:39-50; lap.lapjv(cost, extend_cost=True, cost_limit=thresh))
    on the GPU: the partial matching of pairs with cost < thresh that minimises the sum of (cost - thresh).  `cost_matrix`: [n,m] host
    array or device tensor (geometry.pairwise) - a device matrix is never downloaded.  -> (matches [k,2] int sorted by row,
    unmatched_a, unmatched_b) as ndarrays; one device->host copy of n + m + 1 ints."""
    n, m = cost_matrix.shape
    if n == 0 or m == 0:
        return _empty_triple(n, m)
    ctx = ctx or geometry.default_context()
    out = _assign_dev(ctx, _cost_to_dev(cost_matrix, torch.device("cuda", ctx.device)), 1, n, m, thresh).cpu().numpy()[0]
    return _triple(out[:n], out[n:n + m], out[n + m], "linear_assignment")


def linear_assignment_batch(cost_matrices, thresh, ctx=None):
    """linear_assignment of every matrix of a list (host arrays or device tensors, shapes may differ) in ONE launch and one copy back:
    the matrices go into one [batch, max n, max m] slab (the padding is NaN and never read) with their sizes beside them."""
    shapes = [tuple(c.shape) for c in cost_matrices]
    if not shapes:
        return []
    n, m = max(s[0] for s in shapes), max(s[1] for s in shapes)
    if n == 0 or m == 0:
        return [_empty_triple(*s) for s in shapes]
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    if any(torch.is_tensor(c) for c in cost_matrices):
        slab = torch.full((len(shapes), n, m), float("nan"), dtype=torch.float64, device=dev)
        for k, c in enumerate(cost_matrices):
            slab[k, :shapes[k][0], :shapes[k][1]] = _cost_to_dev(c, dev)
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
    ctx = ctx or geometry.default_context()
    cost = _cost_to_dev(distance_metric(tracks, detections, track_indices, detection_indices), torch.device("cuda", ctx.device))
    n, m = cost.shape
    limit = max_distance + 1e-5
    cost = torch.where(cost > max_distance, limit, cost)
    out = _assign_dev(ctx, cost, 1, n, m, limit).cpu().numpy()[0]
    pairs, ua, ub = _triple(out[:n], out[n:n + m], out[n + m], "min_cost_matching")
    return ([(track_indices[r], detection_indices[c]) for r, c in pairs], [track_indices[r] for r in ua], [detection_indices[c] for c in ub])


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
    parts = [mean.view(-1), cov.view(-1)]
    if m > 0:
        parts.append(_assign_dev(ctx, cost.contiguous(), 1, n, m, thresh).view(-1).to(torch.float64))
        if fuse_motion:
            parts.append(status.to(torch.float64))
    host = torch.cat(parts).cpu().numpy()                        # one device->host copy: states, match vectors, status words
    _set_states(stracks, host)
    if m == 0:
        return _empty_triple(n, 0)
    if fuse_motion:
        _raise_flagged(host[72 * n + n + m + 1:], "associate_round")
    sol = host[72 * n:72 * n + n + m + 1].astype(np.int64)
    return _triple(sol[:n], sol[n:n + m], sol[n + m], "associate_round")


# ---- appearance cost (include/busca_appearance.h) ------------------------------------------------------------------------------
_REDUCE = {"min": _lib.APPEAR_MIN, "mean": _lib.APPEAR_MEAN, "max": _lib.APPEAR_MAX}
INFTY_COST = 1e+5                       # deep_sort/linear_assignment.py:12


def _feats_to_dev(x, dev):
    """A contiguous float32 device tensor of a host array or a tensor (a device float32 tensor is taken as it is)."""
    if not torch.is_tensor(x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        x = torch.from_numpy(x if x.flags.writeable else x.copy())
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _i32_to_dev(x, dev):
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32)).reshape(-1))
    return x.to(device=dev, dtype=torch.int32).contiguous()


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
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    g, d = _feats_to_dev(track_feats, dev), _feats_to_dev(det_feats, dev)
    if g.dim() == 2:
        g = g.unsqueeze(1)
    if g.dim() != 3 or d.dim() != 2:
        raise ValueError("appearance_cost takes [n,E] or [S,budget,E] track features and [m,E] detection features")
    S, budget, E = g.shape
    m = d.shape[0]
    if m > 0 and S > 0 and d.shape[1] != E:
        raise ValueError("track features are %d-dimensional, detection features %d-dimensional" % (E, d.shape[1]))
    for name, v, top in (("slot", slot, S), ("count", count, budget + 1)):       # host indices are checked here; device ones are the caller's
        if v is not None and not torch.is_tensor(v) and len(v) and int(np.max(v)) >= top:
            raise ValueError("%s holds %d, beyond the gallery's %d" % (name, int(np.max(v)), top - 1))
    if count is not None and len(count) != S:
        raise ValueError("count has %d entries for %d slots" % (len(count), S))
    slot, count = _i32_to_dev(slot, dev), _i32_to_dev(count, dev)
    n = S if slot is None else slot.numel()
    out = torch.empty(n, m, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_appearance_cost(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), n, budget, d.data_ptr(), m, E, _REDUCE[reduce],
                                            _lib.APPEAR_CLAMP0 if clamp else 0, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
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
    ctx = ctx or geometry.default_context()
    cost = _cost_to_dev(cost, torch.device("cuda", ctx.device)).reshape(n, m)
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

    def partial_fit(self, features, targets, active_targets):
        """Append feature k, L2-normalised (in float64, stored as float32; deep_sort/track.py:244 stores normalised features), to the samples of
        targets[k]; keep each target's last `budget`; drop every target that is not in `active_targets` and free its slot."""
        targets = list(np.asarray(targets).reshape(-1).tolist()) if not isinstance(targets, list) else targets
        dev = torch.device("cuda", self.ctx.device)
        if len(targets):
            f = _feats_to_dev(features, dev).reshape(len(targets), -1).to(torch.float64)
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
        dev = torch.device("cuda", self.ctx.device)
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
    dev = torch.device("cuda", ctx.device)
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
    ctx = ctx or geometry.default_context()
    cost = _cost_to_dev(cost, torch.device("cuda", ctx.device)).reshape(n, m)
    out, status = _gate_mc_dev(ctx, cost, tracks, detections, track_indices, detection_indices, gated_cost, mc_lambda)
    return _download_with_status(out, status, "gate_cost_matrix_mc")


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
    dev = torch.device("cuda", ctx.device)
    if det_features is None:
        feats = _feats_to_dev(np.asarray([detections[i].feature for i in detection_indices], dtype=np.float32), dev)
    else:
        feats = _feats_to_dev(det_features, dev)
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
        pairs, _, left = _triple(host[:len(rows)], host[len(rows):len(rows) + len(cols)], host[len(rows) + len(cols)], "appearance_round")
        matches += [(track_indices[rows[r]], detection_indices[cols[c]]) for r, c in pairs]
        cols = [cols[c] for c in left]
    unmatched_tracks = list(set(track_indices) - set(k for k, _ in matches))
    return matches, unmatched_tracks, [detection_indices[c] for c in cols]


# ---- GHOST association (include/busca_ghost.h) -----------------------------------------------------------------------------------
_GHOST_REDUCE = {"min": _lib.GHOST_MIN, "mean": _lib.GHOST_MEAN, "max": _lib.GHOST_MAX, "midrange": _lib.GHOST_MIDRANGE, "median": _lib.GHOST_MEDIAN,
                 1: _lib.GHOST_MIN, 2: _lib.GHOST_MEAN, 3: _lib.GHOST_MAX, 4: _lib.GHOST_MIDRANGE, 5: _lib.GHOST_MEDIAN}      # tracker_cfg['avg_inact']['num']
_GHOST_PROXY = {"last": _lib.GHOST_PROXY_LAST, "first": _lib.GHOST_PROXY_FIRST, "mean": _lib.GHOST_PROXY_MEAN, "meannorm": _lib.GHOST_PROXY_MEANNORM,
                "median": _lib.GHOST_PROXY_MEDIAN}
GHOST_LIMIT = 8192.0                    # the solver's limit in ghost_round: costs are <= 2 and n, m <= 2048, so one more match always beats any cost


def _ghost_gallery(track_feats, slot, count, dev, what):
    """The gallery operands of a GHOST call on the device -> (g [S,budget,E] f32, slot i32 or None, count i32 or None, n)."""
    g = _feats_to_dev(track_feats, dev)
    if g.dim() == 2:
        g = g.unsqueeze(1)
    if g.dim() != 3:
        raise ValueError("%s takes [n,E] or [S,budget,E] track features" % what)
    S, budget, _ = g.shape
    for name, v, top in (("slot", slot, S), ("count", count, budget + 1)):       # host indices are checked here; device ones are the caller's
        if v is not None and not torch.is_tensor(v) and len(v) and int(np.max(v)) >= top:
            raise ValueError("%s holds %d, beyond the gallery's %d" % (name, int(np.max(v)), top - 1))
    if count is not None and len(count) != S:
        raise ValueError("count has %d entries for %d slots" % (len(count), S))
    slot, count = _i32_to_dev(slot, dev), _i32_to_dev(count, dev)
    return g, slot, count, (S if slot is None else slot.numel())


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
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    g, slot, count, n = _ghost_gallery(track_feats, slot, count, dev, "ghost_distance")
    d = _feats_to_dev(det_feats, dev)
    if d.dim() != 2:
        raise ValueError("ghost_distance takes [m,E] detection features")
    S, budget, E = g.shape
    m = d.shape[0]
    if m > 0 and S > 0 and d.shape[1] != E:
        raise ValueError("track features are %d-dimensional, detection features %d-dimensional" % (E, d.shape[1]))
    if out is None:
        out = torch.empty(n, m, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (n, m) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 [%d,%d] device tensor" % (n, m))
    ctx.check(ctx.lib.busca_ghost_distance(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), n, budget, d.data_ptr(), m, E, _GHOST_REDUCE[reduce],
                                           out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def ghost_proxies(gallery, mode="mean", window=0, slot=None, count=None, newest=None, ctx=None):
    """busca_ghost_proxies: get_proxy (adapters/GHOST/src/tracking_utils.py:63-126) - one vector per track from its stored samples.
      gallery  [S,budget,E] float32, a ring of `budget` rows per slot; slot / count as appearance_cost
      newest   [S] ints or None: the ring row of every slot's newest sample (None: count - 1)
      mode     'last', 'first' (the oldest stored sample), 'mean', 'meannorm', 'median' (torch.median: the lower one)
      window   the newest `window` samples take part (tracker_cfg['avg_*']['num']); 0 or 'all', or more than a track has: all of them
    torch.mode and the stateful 'mv_avg' are not built (mv_avg is `mv_avg * a + last * (1 - a)` on the caller's own tensor).
    -> device float32 tensor [n,E]; a track without samples gets a row of NaN."""
    if mode in ("mode", "mv_avg"):
        raise NotImplementedError("ghost_proxies: the %r proxy is not built on the device (torch.mode has no kernel here; mv_avg is a stateful "
                                  "moving average - keep it a tensor op of the caller's)" % (mode,))
    if mode not in _GHOST_PROXY:
        raise ValueError("mode must be one of %s, not %r" % (sorted(_GHOST_PROXY), mode))
    window = 0 if window in (None, "all") else int(window)
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    g, slot, count, n = _ghost_gallery(gallery, slot, count, dev, "ghost_proxies")
    S, budget, E = g.shape
    if newest is not None and len(newest) != S:
        raise ValueError("newest has %d entries for %d slots" % (len(newest), S))
    newest = _i32_to_dev(newest, dev)
    out = torch.empty(n, E, dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.busca_ghost_proxies(ctx.h, g.data_ptr(), _lib.ptr(slot), _lib.ptr(count), _lib.ptr(newest), n, budget, E, _GHOST_PROXY[mode], window,
                                          out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def ghost_thresholds(cost, num_active, k_act, k_inact, out=None, ctx=None):
    """busca_ghost_thresholds: update_thresholds (adapters/GHOST/src/base_tracker.py:495-531) on a tracks x detections device matrix whose first
    `num_active` rows are the active tracks: (mean - k_act * std of those rows, mean - k_inact * std of the others), np.std's population std; the
    reference's k are (0, 2) with 'every' and (0.5, 1) with 'tbd'.  -> device float64 tensor [2], never synchronised: hand it to ghost_cost as it is.
    A group without rows keeps its entry of `out` (a new tensor starts at +inf, a threshold nothing exceeds)."""
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    cost = _cost_to_dev(cost, dev)
    n, m = cost.shape
    if out is None:
        out = torch.full((2,), float("inf"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_ghost_thresholds(ctx.h, cost.data_ptr(), n, m, int(num_active), float(k_act), float(k_inact), out.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream))
    return out


def ghost_cost(app, motion=None, alpha=0.0, track_labels=None, det_labels=None, num_active=None, thr=None, ctx=None):
    """busca_ghost_combine: the entrywise rest of GHOST's cost matrix on a tracks x detections matrix, in the reference's order - entries whose
    track and detection labels differ become NaN (nan_over_classes, tracker.py:272-275 / :299-302), then (1 - alpha) * app + alpha * motion
    (combine_motion_appearance with combi 'sum_<alpha>', base_tracker.py:713-731), then entries that are not <= thr[0] (the first `num_active` rows)
    / thr[1] (the others) become NaN (nan_first, tracker.py:392-396).  Every part is optional.  `thr`: two numbers or a device float64 [2] tensor
    (ghost_thresholds).  -> a new device float64 tensor [n,m]."""
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    app = _cost_to_dev(app, dev)
    n, m = app.shape
    if motion is not None:
        motion = _cost_to_dev(motion, dev)
        if tuple(motion.shape) != (n, m):
            raise ValueError("the motion cost is %s, the appearance cost %s: both are tracks x detections" % (tuple(motion.shape), (n, m)))
    if (track_labels is None) != (det_labels is None):
        raise ValueError("track_labels and det_labels go together")
    tl, dl = _i32_to_dev(track_labels, dev), _i32_to_dev(det_labels, dev)
    if tl is not None and (tl.numel() != n or dl.numel() != m):
        raise ValueError("%d track labels and %d detection labels for a %d x %d matrix" % (tl.numel(), dl.numel(), n, m))
    if thr is not None and not torch.is_tensor(thr):
        thr = torch.from_numpy(np.asarray(thr, dtype=np.float64).reshape(2))
    if thr is not None:
        thr = thr.to(device=dev, dtype=torch.float64).contiguous()
    out = torch.empty(n, m, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_ghost_combine(ctx.h, app.data_ptr(), _lib.ptr(motion), n, m, float(alpha), _lib.ptr(tl), _lib.ptr(dl),
                                          n if num_active is None else int(num_active), _lib.ptr(thr), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
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


# ---- GHOST's linear motion model (include/busca_ghost_motion.h) ----------------------------------------------------------------
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


def _small_to_dev(x, dev, dtype):
    """A small index / flag vector on the device; a host array goes through pinned staging, so the host does not wait for the stream."""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x.to(device=dev, dtype=dtype).contiguous().view(-1)
    return geometry.h2d_async(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dtype), dev)


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
        self.ctx = ctx or geometry.default_context()
        self.dev = torch.device("cuda", self.ctx.device)
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

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def add(self, slots, boxes, frame, det_index=None, new=None):
        """Detection det_index[i] (None: i) of `boxes` [m,4] tlbr (host array or device tensor) becomes the position of slot slots[i] and joins its
        history with frame number `frame`; new[i] true starts a new track in that slot (history emptied, velocity zero).  Host boxes are rounded to
        `box_dtype` first, as the reference's arrays are; a device tensor is taken as float64 values."""
        slot, k = _slots_checked(slots, self.capacity, "GhostMotion.add")
        if not torch.is_tensor(boxes):
            boxes = np.asarray(boxes, dtype=np.float32 if self.box32 else np.float64).astype(np.float64).reshape(-1, 4)
        boxes = _cost_to_dev(boxes, self.dev).view(-1, 4)
        m = boxes.shape[0]
        det = _small_to_dev(det_index if det_index is None or torch.is_tensor(det_index) else np.asarray(det_index, dtype=np.int32), self.dev, torch.int32)
        if det is None and k > m:
            raise ValueError("GhostMotion.add: %d slots for %d boxes" % (k, m))
        if det is not None and det.numel() != k:
            raise ValueError("GhostMotion.add: %d detection indices for %d slots" % (det.numel(), k))
        reset = None
        if new is not None:
            reset = _small_to_dev(new if torch.is_tensor(new) else np.asarray(new, dtype=np.bool_).astype(np.uint8), self.dev, torch.uint8)
            if reset.numel() != k:
                raise ValueError("GhostMotion.add: %d `new` flags for %d slots" % (reset.numel(), k))
        slot = _small_to_dev(slot, self.dev, torch.int32)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_append(c.h, self.hist.data_ptr(), self.frames.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(),
                                                self.pos.data_ptr(), self.vel.data_ptr(), self.capacity, self.history, slot.data_ptr(), _lib.ptr(det),
                                                _lib.ptr(reset), k, boxes.data_ptr(), m, int(frame), self._stream()))
        if k:
            self.all_warped = False

    def compensate(self, warp, slots=None):
        """Every stored box of `slots` (None: all) through the [2,3] warp (host float32), as motion_compensation does for every track."""
        warp = np.ascontiguousarray(np.asarray(warp, dtype=np.float32).reshape(6))
        slot, n = (None, 0) if slots is None else _slots_checked(slots, self.capacity, "GhostMotion.compensate")
        slot = _small_to_dev(slot, self.dev, torch.int32)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_warp(c.h, self.hist.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(), self.capacity, self.history,
                                              _lib.ptr(slot), n, warp.ctypes.data, self._stream()))
        if slots is None:
            self.all_warped = True

    def step(self, slots, num_active, last_n_frames):
        """One motion() step for the tracks in `slots`, ACTIVE TRACKS FIRST (`num_active` of them) -> device float64 [n,4], their positions in
        list order (a negative slot: a row of NaN).  It advances pos: once per frame, as the reference calls motion()."""
        slot, n = _slots_checked(slots, self.capacity, "GhostMotion.step")
        slot = _small_to_dev(slot, self.dev, torch.int32)
        out = torch.empty(n, 4, dtype=torch.float64, device=self.dev)
        c = self.ctx
        c.check(c.lib.busca_ghost_motion_step(c.h, self.hist.data_ptr(), self.frames.data_ptr(), self.count.data_ptr(), self.newest.data_ptr(),
                                              self.pos.data_ptr(), self.vel.data_ptr(), self.capacity, self.history, slot.data_ptr(), n, int(num_active),
                                              min(int(last_n_frames), 2 ** 31 - 1), int(self.diff32), out.data_ptr(), self._stream()))
        return out

    def cost(self, slots, num_active, det_boxes, last_n_frames):
        """step(), then get_motion_dist: 1 - IoU ("+1" pixel convention) of the stepped positions and `det_boxes` [m,4] -> device float64 [n,m],
        tracks x detections (the reference's matrix transposed): the `motion` operand of ghost_cost / ghost_round."""
        pos = self.step(slots, num_active, last_n_frames)
        if not torch.is_tensor(det_boxes):
            det_boxes = np.array(det_boxes, dtype=np.float64).reshape(-1, 4)
        return geometry.pairwise(self.ctx, pos, det_boxes, _lib.PAIR_IOU_COST)


_GHOST_WARP_MODES = {"Translation": _lib.ECC_TRANSLATION, "Affine": _lib.ECC_AFFINE, "Euclidean": _lib.ECC_EUCLIDEAN}     # warp_mode_dct, base_tracker.py:60-65


def ghost_ecc_check_config(motion_cfg):
    """motion_config['warp_mode'] -> the motion code of busca_ecc_align_planes.  'Homography' is refused; an unknown name raises KeyError, as
    `self.warp_mode_dct[...]` does."""
    mode = motion_cfg["warp_mode"]
    if mode == "Homography":
        raise ValueError("GHOST warp_mode 'Homography' is refused: the reference always passes np.eye(2, 3) (base_tracker.py:613) and OpenCV asserts a "
                         "3-row warp matrix for homographies, so this branch raises in the reference and there is nothing to reproduce")
    return _GHOST_WARP_MODES[mode]


def _ecc_frame(frame, dev):
    """A float32 frame [3,H,W] or [H,W] on the device, strides kept (a host frame through pinned staging) -> (tensor, channels, H, W)."""
    if not torch.is_tensor(frame):
        frame = torch.from_numpy(np.asarray(frame))
    if frame.dtype != torch.float32 or frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[0] != 3):
        raise ValueError("an ECC frame is float32 [3,H,W] or [H,W], not %s %s" % (frame.dtype, tuple(frame.shape)))
    if frame.device.type == "cpu":
        frame = geometry.h2d_async(frame, dev)
    elif frame.device != dev:
        frame = frame.to(dev)
    if any(s < 0 for s in frame.stride()) or frame.stride(-1) == 0:
        frame = frame.contiguous()
    return frame, (3 if frame.dim() == 3 else 1), int(frame.shape[-2]), int(frame.shape[-1])


def _ecc_prepare(ctx, frame, channels, H, W, ksize, out):
    """busca_ecc_prepare of a device frame into the [H,W] float32 plane `out`, on the current stream."""
    dev = out.device
    st = frame.stride()
    ctx.check(ctx.lib.busca_ecc_prepare(ctx.h, frame.data_ptr(), channels, H, W, st[0] if channels == 3 else 0, st[-2], st[-1], int(ksize),
                                        out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))


def _ecc_align_planes(ctx, templ, inp, motion, iters, eps, warp):
    """busca_ecc_align_planes on two [H,W] planes; `warp` (host float32 [2,3]) is updated in place -> (cc, iterations)."""
    import ctypes as C
    H, W = templ.shape
    cc, its = C.c_double(0.0), C.c_int32(0)
    ctx.check(ctx.lib.busca_ecc_align_planes(ctx.h, templ.data_ptr(), inp.data_ptr(), H, W, int(motion), int(iters), float(eps), warp.ctypes.data,
                                             C.byref(cc), C.byref(its), torch.cuda.current_stream(templ.device).cuda_stream))
    return cc.value, its.value


def _ecc_motion_code(motion):
    if isinstance(motion, str):
        if motion == "MOTION_HOMOGRAPHY" or motion == "Homography":
            raise ValueError("Invalid warp_mode: {}".format(motion))
        return _GHOST_WARP_MODES[motion[7:].capitalize() if motion.startswith("MOTION_") else motion]
    return int(motion)


def find_transform_ecc_f32(template, input, warp_matrix=None, motion="Euclidean", gauss_size=15, number_of_iterations=100, termination_eps=1e-5,
                           ctx=None):
    """cv2.cvtColor(RGB2GRAY) + cv2.findTransformECC(template, input, warp_matrix, motion, criteria, None, gauss_size) on float32 frames, on the
    GPU (busca_ecc_prepare x2 + busca_ecc_align_planes; OpenCV's arithmetic restated, parity unpinned: include/busca_ecc.h).  Frames: float32
    [3,H,W] RGB or [H,W] grey, host arrays or cuda tensors of any strides.  motion: 'Translation' | 'Euclidean' | 'Affine' (GHOST's names) or
    'MOTION_...' (OpenCV's).  Returns (cc, warp float32 [2,3]); raises BuscaError where OpenCV raises.  The stateless form, for callers with two
    frames in hand: a tracker prepares every frame once with GhostCameraMotion."""
    code = _ecc_motion_code(motion)
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    planes = []
    for f in (template, input):
        f, ch, H, W = _ecc_frame(f, dev)
        planes.append(torch.empty(H, W, dtype=torch.float32, device=dev))
        _ecc_prepare(ctx, f, ch, H, W, gauss_size, planes[-1])
    if planes[0].shape != planes[1].shape:
        raise ValueError("template %s and input %s differ in size" % (tuple(planes[0].shape), tuple(planes[1].shape)))
    warp = np.eye(2, 3, dtype=np.float32) if warp_matrix is None else np.ascontiguousarray(warp_matrix, dtype=np.float32).reshape(2, 3).copy()
    cc, its = _ecc_align_planes(ctx, planes[0], planes[1], code, number_of_iterations, termination_eps, warp)
    find_transform_ecc_f32.last_iterations = its
    return cc, warp


class GhostCameraMotion:
    """The estimate of GHOST's motion_compensation on the device (base_tracker.py:605-622, :633): every frame is prepared once - grey, 15-pixel
    Gaussian (busca_ecc_prepare) - and its plane serves as the template of this frame's alignment and as the input of the next one's, so no
    `last_image` is kept and no frame leaves the device.  Reads motion_cfg['warp_mode'], ['num_iter_mc'] and ['termination_eps_mc'].
      estimate(whole_image)  float32 [3,H,W] cuda tensor of any strides (or a host tensor / array, uploaded through pinned staging) -> None on
                             the first frame, then the float32 [2,3] warp of cv2.findTransformECC(current, previous, eye(2,3), ...)
      norm, cc, iterations   of the last estimate: np.linalg.norm(warp[:, -1]) (the reference's warp_matrix_nomr; None on a first frame), the
                             correlation coefficient, the iterations run
      prepared               busca_ecc_prepare calls so far
      reset()                a new sequence: the next frame is a first frame
    Where OpenCV raises (no convergence, singular Hessian) estimate raises BuscaError and the stored plane stays the one of the last good frame,
    as self.last_image does in the reference.  The two planes are allocated with the first frame and swapped from then on."""

    def __init__(self, motion_cfg, gauss_size=15, ctx=None):
        self.motion = ghost_ecc_check_config(motion_cfg)
        self.iters, self.eps = int(motion_cfg["num_iter_mc"]), float(motion_cfg["termination_eps_mc"])
        self.gauss_size = int(gauss_size)
        if self.gauss_size < 1 or self.gauss_size > _lib.ECC_KSIZE_MAX or self.gauss_size % 2 == 0:
            raise ValueError("gauss_size %d is not an odd size in 1 .. %d" % (self.gauss_size, _lib.ECC_KSIZE_MAX))
        self.ctx = ctx or geometry.default_context()
        self.dev = torch.device("cuda", self.ctx.device)
        self._planes, self._cur = None, 0               # two [H,W] planes; _planes[_cur] is the stored (previous) frame's
        self.prepared = 0
        self.reset()

    def reset(self):
        self._have = False
        self.norm = self.cc = self.iterations = None

    def estimate(self, whole_image):
        frame, ch, H, W = _ecc_frame(whole_image, self.dev)
        if self._planes is None:
            self._planes = [torch.empty(H, W, dtype=torch.float32, device=self.dev) for _ in range(2)]
        elif tuple(self._planes[0].shape) != (H, W):
            raise ValueError("GhostCameraMotion: a %d x %d frame in a sequence of %d x %d frames" % ((H, W) + tuple(self._planes[0].shape)))
        new = self._planes[1 - self._cur]
        _ecc_prepare(self.ctx, frame, ch, H, W, self.gauss_size, new)
        self.prepared += 1
        self.norm = None
        warp = None
        if self._have:
            warp = np.eye(2, 3, dtype=np.float32)
            self.cc, self.iterations = _ecc_align_planes(self.ctx, new, self._planes[self._cur], self.motion, self.iters, self.eps, warp)
            self.norm = np.linalg.norm(warp[:, -1])
        self._cur, self._have = 1 - self._cur, True
        return warp


def ghost_motion_compensation(camera, motion_state, whole_image, is_moving, enabled=True):
    """BaseTracker.motion_compensation (base_tracker.py:600-633) on the device: the warp of this frame against the previous one
    (camera: GhostCameraMotion) and, when the sequence has a moving camera (`is_moving`) and motion_config['motion_compensation'] (`enabled`),
    every stored position of every track through it (motion_state: GhostMotion).  Returns the warp, None on the first frame."""
    warp = camera.estimate(whole_image)
    if warp is not None and is_moving and enabled:
        motion_state.compensate(warp)
    return warp


def _ghost_get(state, name, default=None):
    return state.get(name, default) if isinstance(state, dict) else getattr(state, name, default)


def _ghost_proxy_rows(ctx, g, count, newest, slot, entry, what):
    """get_proxy's choice for one group of tracks (tracker_cfg['avg_act'] / ['avg_inact']) -> device [k,E] float32."""
    if not entry.get("do", False):
        return ghost_proxies(g, "last", slot=slot, count=count, newest=newest, ctx=ctx)          # track.feats: the newest sample
    proxy, num = entry.get("proxy", "last"), entry.get("num", "all")
    if proxy == "last":
        return ghost_proxies(g, "last", slot=slot, count=count, newest=newest, ctx=ctx)
    if num == "first":
        return ghost_proxies(g, "first", slot=slot, count=count, newest=newest, ctx=ctx)
    if proxy in ("mv_avg", "mode") or proxy not in _GHOST_PROXY:
        raise NotImplementedError("ghost_round: %s proxy %r is not built on the device" % (what, proxy))
    return ghost_proxies(g, proxy, 0 if num == "all" else int(num), slot=slot, count=count, newest=newest, ctx=ctx)


def ghost_round(state, det_feats, labels=None, motion=None, cfg=None, sep=None, thresholds=None, ctx=None, det_boxes=None):
    """GHOST's association round without leaving the device: get_hungarian_each_sample / get_hungarian_with_proxy + solve_hungarian
    (adapters/GHOST/src/tracker.py:306-480) from the tracks' sample galleries and the detections' features in HBM to the matches on the host.
      state       the tracks: a dict or object with `gallery` [S,budget,E] float32 (host array or device tensor), `count` [S] and `newest` [S] (or None,
                  as ghost_proxies), `slot` [n] or None - the gallery slot of track i, ACTIVE TRACKS FIRST - and `num_active`
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
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    g, slot, count, n = _ghost_gallery(_ghost_get(state, "gallery"), _ghost_get(state, "slot"), _ghost_get(state, "count"), dev, "ghost_round")
    newest = _i32_to_dev(_ghost_get(state, "newest"), dev)
    na = _ghost_get(state, "num_active")
    na = n if na is None else int(na)
    if not 0 <= na <= n:
        raise ValueError("num_active %d outside 0 .. %d" % (na, n))
    d = _feats_to_dev(det_feats, dev)
    m = d.shape[0]
    sep = bool(cfg.get("assign_separately", False)) if sep is None else bool(sep)
    empty = np.empty(0, dtype=np.int64)
    if n == 0 or m == 0:
        return torch.empty(m, n, dtype=torch.float64, device=dev), empty, empty
    if slot is None:
        slot = torch.arange(n, dtype=torch.int32, device=dev)
    act, inact = cfg.get("avg_act", {}), cfg.get("avg_inact", {})
    each = inact.get("proxy") == "each_sample"
    app = torch.empty(n, m, dtype=torch.float64, device=dev)
    def kind(entry):                                              # what a group of tracks runs: its rows depend on nothing else
        if each:
            return ("samples", inact.get("num", 2)) if entry.get("do", False) else ("last",)
        return ("proxy", entry.get("proxy", "last"), entry.get("num", "all")) if entry.get("do", False) else ("last",)
    groups = ((0, n, inact, "avg_inact"),) if kind(act) == kind(inact) else ((0, na, act, "avg_act"), (na, n, inact, "avg_inact"))      # one launch where both groups run the same
    for lo, hi, entry, what in groups:
        if hi == lo:
            continue
        if each and entry.get("do", False):                       # proxy_dist over the track's samples; both groups reduce with avg_inact['num']
            ghost_distance(g, d, inact.get("num", 2), slot=slot[lo:hi], count=count, out=app[lo:hi], ctx=ctx)
        else:                                                     # one vector per track (last_frame, or get_proxy), then the plain cosine distance
            entry = {"do": False} if each else entry
            ghost_distance(_ghost_proxy_rows(ctx, g, count, newest, slot[lo:hi], entry, what), d, "min", out=app[lo:hi], ctx=ctx)
    tl = dl = None
    if each and labels is not None and cfg.get("nan_over_classes", True):
        tl, dl = labels
    at, it = cfg.get("act_reid_thresh"), cfg.get("inact_reid_thresh")
    every, tbd = at == "every", at == "tbd"
    for name, v in (("act_reid_thresh", at), ("inact_reid_thresh", it)):
        if isinstance(v, str) and v not in ("every", "tbd"):
            raise ValueError("%s must be a number, 'every' or 'tbd', not %r" % (name, v))
    data_act, data_inact = every or tbd, every or it == "tbd"
    if it == "tbd" and not (every or tbd):
        raise ValueError("inact_reid_thresh 'tbd' needs act_reid_thresh 'tbd' or 'every': the reference leaves it a string otherwise (base_tracker.py:515-531)")
    mcfg = cfg.get("motion_config", {})
    blend = bool(mcfg.get("apply_motion_model", False))
    alpha = 0.0
    if blend:
        combi = str(mcfg.get("combi", ""))
        if "sum" not in combi:
            raise NotImplementedError("ghost_round: motion_config combi %r is not built; only 'sum_<alpha>'" % (combi,))
        alpha = float(combi.split("_")[-1])
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


def remove_duplicate_stracks(stracksa, stracksb, ctx=None, thresh=0.15):
    """remove_duplicate_stracks (byte_tracker.py:685-698): of two tracks whose IoU cost is below 0.15 the one alive for
    fewer frames goes (ties: the one of the first list).  IoU cost and the marking both run on the GPU."""
    if len(stracksa) == 0 or len(stracksb) == 0:
        return list(stracksa), list(stracksb)
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    cost = geometry.pairwise(ctx, _tlbrs(stracksa), _tlbrs(stracksb), _lib.PAIR_IOU_COST)
    age_a = torch.tensor([t.frame_id - t.start_frame for t in stracksa], dtype=torch.int32, device=dev)
    age_b = torch.tensor([t.frame_id - t.start_frame for t in stracksb], dtype=torch.int32, device=dev)
    keep_a = torch.empty(len(stracksa), dtype=torch.uint8, device=dev)
    keep_b = torch.empty(len(stracksb), dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.busca_duplicate_masks(ctx.h, cost.data_ptr(), len(stracksa), len(stracksb), age_a.data_ptr(), age_b.data_ptr(),
                                            float(thresh), keep_a.data_ptr(), keep_b.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    kab = torch.cat([keep_a, keep_b]).cpu().numpy()                              # one device->host copy for both masks
    ka, kb = kab[:len(stracksa)], kab[len(stracksa):]
    return [t for i, t in enumerate(stracksa) if ka[i]], [t for i, t in enumerate(stracksb) if kb[i]]


_PIXEL_MEAN = np.array([0.406, 0.456, 0.485])   # BGR
_PIXEL_STD = np.array([0.225, 0.224, 0.299])    # BGR; 0.299 is the reference's "ghost" normalisation


def normalize_crops(u8):
    """(x/255 - mean)/std in BGR order, float32 (busca/network.py:470-478)."""
    x = np.asarray(u8).astype(np.float32) / 255.0
    x -= _PIXEL_MEAN
    x /= _PIXEL_STD
    return x


class DeviceBackedCrops(np.ndarray):
    """Host uint8 crops that remember their device-resident twins (device-resident track memory).

    `get_image_crops(..., normalize=False)` returns this ndarray subclass: to the trackers it is an ordinary uint8
    array ([N,384,128,3] with REAL host bytes; `crops[i]` is what they append to `images_mem`), but `crops[i]` also
    carries `.slot`, its slot in the bounded device pool (busca_amd/crop_pool.py).  `associate_embeddings` gathers
    slots on the GPU and skips the per-frame host->device copy of B*(L+P) crops (147 KB each).  Anything that loses
    the slot (np.array(...) copies, pickling, arithmetic) is still a correct host crop and takes the host path."""

    def __new__(cls, host, slots):
        host = np.asarray(host)
        obj = host.view(cls)
        obj._slots = slots
        obj._host = host                    # the plain array: slot.host views must not reference this subclass (no cycles)
        obj.slot = None
        return obj

    def __array_finalize__(self, obj):
        self._slots = None                  # generic views/copies do not know which pool slots they cover
        self._host = None
        self.slot = None

    def __getitem__(self, key):
        if self._slots is not None and self.ndim == 4 and isinstance(key, (int, np.integer)):
            # the crop is a view of the PLAIN host array: it keeps the frame's host bytes alive (as the reference's
            # np.stack'ed crops do) but not this container, so the other crops' pool slots are free to go
            k = int(key)
            out = self._host[k].view(DeviceBackedCrops)
            out.slot = self._slots[k]
            if out.slot.host is None:
                out.slot.host = self._host[k]             # a spill of this crop needs no device->host copy
            return out
        return super().__getitem__(key)

    def __reduce__(self):                   # pickling / copy.deepcopy: a plain host array (the slot stays with this process)
        return np.asarray(self).__reduce__()

    @property
    def dev(self):
        """cuda u8 view of this crop's slot ([384,128,3]); None for non-crop views and after a spill."""
        return self.slot.tensor() if self.slot is not None else None


class FrameHostCopy:
    """The host bytes of one get_image_crops call, ON DEMAND (round 5): the crops live in pool slots; nothing is copied to the host until somebody
    reads a pixel.  The first host read of ANY crop of the call fetches the WHOLE batch in one go - one index-gather launch over the call's slots
    (busca_gather_crops) and one device->host copy - so a tracker that looks at every crop pays one transfer per call, and one that never looks
    (the five adapters only store the crops and hand them back to associate_embeddings) pays nothing: no pinned buffer, no copy, no side stream
    (rounds 3-4 enqueued a 17 MB pinned copy per call whether or not anyone read it: 0.12 ms of host time per call).
    A slot that was released and reused before the read shows another crop's bytes in its row - a row nobody can ask for any more."""
    __slots__ = ("ctx", "ptrs", "event", "_np", "expired")

    def __init__(self, ctx=None, ptrs=None, event=None):
        self.ctx, self.ptrs, self.event, self._np, self.expired = ctx, ptrs, event, None, False

    def rows(self):
        """uint8 [n,384,128,3] host view of the batch (fetched on the first call)."""
        if self._np is None:
            dev = torch.device("cuda", self.ctx.device)
            if self.event is not None:
                torch.cuda.current_stream(dev).wait_event(self.event)      # the crop kernel may have run on another stream
            self._np = geometry.gather_crops(self.ctx, self.ptrs).cpu().numpy()
            self.event = None
        return self._np


DeviceCrop = Slot                       # one object per crop: the pool slot IS what the tracker stores (busca_amd/crop_pool.py)


class DeviceCrops:
    """Sequence of DeviceCrop ([N,384,128,3] uint8 to duck-typing callers); `crops[i]` is what a tracker stores."""
    dtype, ndim = np.dtype(np.uint8), 4

    def __init__(self, slots):
        self._items = list(slots)

    @property
    def shape(self):
        return (len(self._items), 384, 128, 3)

    def __len__(self):
        return len(self._items)

    def __iter__(self):
        return iter(self._items)

    def __getitem__(self, key):
        if isinstance(key, (int, np.integer)):
            return self._items[int(key)]
        return np.asarray(self)[key]

    def __array__(self, dtype=None, copy=None):
        a = np.stack([np.asarray(c) for c in self._items]) if self._items else np.zeros((0, 384, 128, 3), np.uint8)
        return a if dtype is None else a.astype(dtype)


def box_extents(bboxes):
    """[n,4] x1y1x2y2 -> int32 (floor(x1), floor(y1), ceil(x2), ceil(y2)) on the caller's float64 values, as
    busca/tracking.py:84-87 does with math.floor / math.ceil (a float32 copy of the box can land on the other side of
    an integer).  Clamped to +-2^30 so absurd boxes cannot overflow the kernel's int arithmetic."""
    b = np.nan_to_num(np.asarray(bboxes, dtype=np.float64).reshape(-1, 4), nan=0.0, posinf=2.0 ** 30, neginf=-2.0 ** 30)
    r = np.empty(b.shape, np.float64)
    r[:, :2] = np.floor(b[:, :2])
    r[:, 2:] = np.ceil(b[:, 2:])
    return np.clip(r, -2.0 ** 30, 2.0 ** 30).astype(np.int32)


def get_image_crops(im, bboxes, normalize=True, ctx=None, device_only=False, host_copy=None, output_size=None):
    """All crops of one frame in one launch: u8 BGR [N,384,128,3] (float32 normalised if `normalize`).
    With normalize=False every crop is written into a slot of the device crop pool and the returned crops remember
    their slot.  `host_copy` says what happens to the HOST bytes of those crops (147 KB each - the bulk of this call when it
    is waited for; busca/network.py:492-507 returns host arrays):
      "lazy"  (default) nothing is copied until somebody reads a pixel: the returned `DeviceCrops` fetch the whole batch with one
              gather + one device->host copy on the first host read of any of its crops;
      "eager" wait for it: a real uint8 ndarray (`DeviceBackedCrops`) - for callers that need ndarray instances;
      "never" (`device_only=True`) no copy at all; a host read copies that one crop back synchronously."""
    rects = box_extents(bboxes)
    sized = output_size is not None and tuple(int(v) for v in output_size) != (128, 384)
    if len(rects) == 0:
        return np.zeros([0, int(output_size[0]), int(output_size[1]), 3]) if sized else np.zeros([0, 128, 384, 3])     # the reference's (transposed) empty shape, network.py:503
    ctx = ctx or geometry.default_context()
    if sized:
        # `output_size` = (width, height) as cv2.resize takes it (tracking.py:71): plain host arrays [N, height, width, 3], no pool slots -
        # only the 384 x 128 crops are ReID inputs
        u8 = geometry.crop_gather_sized(ctx, im, rects, int(output_size[0]), int(output_size[1])).cpu().numpy()
        return normalize_crops(u8) if normalize else u8
    if normalize:
        u8, _ = geometry.crop_gather(ctx, im, rects, want_u8=True)
        return normalize_crops(u8.cpu().numpy())
    if host_copy is None:
        host_copy = "never" if device_only else "lazy"
    if host_copy not in ("lazy", "eager", "never"):
        raise ValueError("host_copy must be 'lazy', 'eager' or 'never', not %r" % (host_copy,))
    pool = geometry.crop_pool(ctx)
    frame = FrameHostCopy() if host_copy == "lazy" else None
    slots = pool.alloc(len(rects), frame)
    ptrs = np.fromiter((s.ptr for s in slots), dtype=np.uint64, count=len(slots))
    if host_copy == "never":
        geometry.crop_gather(ctx, im, rects, want_u8=False, dst_ptrs=ptrs)
        return DeviceCrops(slots)
    if host_copy == "eager":
        packed, _ = geometry.crop_gather(ctx, im, rects, want_u8=True, dst_ptrs=ptrs)    # the same launch also writes the batch as one contiguous buffer (the slots need not be adjacent)
        return DeviceBackedCrops(packed.cpu().numpy(), slots)
    # lazy: pool slots only; the host bytes are fetched by the first host read (FrameHostCopy)
    geometry.crop_gather(ctx, im, rects, want_u8=False, dst_ptrs=ptrs)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(torch.device("cuda", ctx.device)))
    frame.ctx, frame.ptrs, frame.event = ctx, ptrs, ev
    return DeviceCrops(slots)


def get_bbox_crop(im, bbox_real_scale, output_size=(128, 384), normalize=True, ghost_normalize=True, ctx=None):
    """Single crop (busca/tracking.py:62-78); `output_size` = (width, height) as cv2.resize takes it."""
    crop = np.asarray(get_image_crops(im, [bbox_real_scale], normalize=False, ctx=ctx, output_size=output_size)[0])
    if normalize:
        crop = crop.astype(np.float32) / 255.0
        crop -= _PIXEL_MEAN
        crop /= (_PIXEL_STD if ghost_normalize else np.array([0.225, 0.224, 0.229]))
    return crop


def get_detection_coverage(frame_shape, active_stracks, inactive_stracks=(), ctx=None):
    """Share of the frame covered by the tracks' boxes and the per-object area statistics of the reliability gate
    (adapters/ByteTrack/yolox/tracker/byte_tracker.py:574-623) - same dict as the reference; the pixel count comes
    from busca_coverage instead of drawing filled rectangles on an H x W x 3 canvas.  `frame_shape` = frame.shape.
    The reference's area normalisation divides the box WIDTH by the frame height and the box HEIGHT by the frame
    width (:589); that is reproduced as is."""
    H, W = int(frame_shape[0]), int(frame_shape[1])
    rects, areas = [], []
    for track in list(active_stracks) + list(inactive_stracks):
        bb = np.array(track.tlbr) * track.scale
        x1, y1, x2, y2 = int(bb[0]), int(bb[1]), int(bb[2]), int(bb[3])          # int() truncates toward zero
        xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        if xb >= 0 and yb >= 0 and xa <= W - 1 and ya <= H - 1:                  # clipped rectangle is not empty
            rects.append([max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)])
        areas.append(max(min(((bb[2] - bb[0]) / H) * ((bb[3] - bb[1]) / W), 1.0), 0.0))
    n_obj = len(areas)
    covered = 0
    if rects:
        ctx = ctx or geometry.default_context()
        dev = torch.device("cuda", ctx.device)
        r = torch.tensor(rects, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.check(ctx.lib.busca_coverage(ctx.h, r.data_ptr(), len(rects), H, W, cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        covered = int(cnt.item())
    pct = covered / (H * W)
    if n_obj > 0:
        avg_cov = pct / n_obj
        avg_area = np.sqrt(np.array(areas)).mean() ** 2
    else:
        avg_cov, avg_area = 0.0, 0.0
    return {"area_covered": pct, "area_covered_per_obj": avg_cov, "max_bbox_area": max(areas) if areas else 0.0,
            "average_bbox_area": avg_area, "bbox_areas": areas}


def is_reliable(frame_shape, active_stracks, p, ctx=None):
    """byte_tracker.py:459-465: the frame is 'reliable' when the covered area exceeds p[0] * per-object area + p[1]."""
    cov = get_detection_coverage(frame_shape, active_stracks, (), ctx=ctx)
    return bool(cov["area_covered"] > cov["area_covered_per_obj"] * p[0] + p[1])


def find_transform_ecc(prev_frame, cur_frame, warp_matrix=None, motion="MOTION_EUCLIDEAN", number_of_iterations=100,
                       termination_eps=1e-5, ctx=None):
    """cv2.cvtColor(BGR2GRAY) + cv2.findTransformECC(templateImage=prev, inputImage=cur, ...) on the GPU (busca_ecc_align;
    third-party OpenCV arithmetic restated, see oracle/ecc.py).  Frames: u8 BGR [H,W,3] (numpy or cuda tensors).
    Returns (cc, warp float32 [2,3]); raises BuscaError where OpenCV raises (no convergence / NaN)."""
    import ctypes as C
    ctx = ctx or geometry.default_context()
    dev = torch.device("cuda", ctx.device)
    if motion not in ("MOTION_EUCLIDEAN", "MOTION_AFFINE"):
        raise ValueError("Invalid warp_mode: {}".format(motion))
    fr = []
    for f in (prev_frame, cur_frame):
        if not torch.is_tensor(f):
            f = torch.from_numpy(np.ascontiguousarray(f))
        f = f.to(dev).contiguous()
        assert f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3
        fr.append(f)
    assert fr[0].shape == fr[1].shape
    H, W = fr[0].shape[:2]
    warp = np.eye(2, 3, dtype=np.float32) if warp_matrix is None else np.ascontiguousarray(warp_matrix, dtype=np.float32).reshape(2, 3).copy()
    cc, iters = C.c_double(0.0), C.c_int32(0)
    ctx.check(ctx.lib.busca_ecc_align(ctx.h, fr[0].data_ptr(), fr[1].data_ptr(), H, W, fr[0].stride(0), fr[1].stride(0),
                                      0 if motion == "MOTION_EUCLIDEAN" else 1, int(number_of_iterations), float(termination_eps),
                                      warp.ctypes.data, C.byref(cc), C.byref(iters), torch.cuda.current_stream(dev).cuda_stream))
    find_transform_ecc.last_iterations = iters.value
    return cc.value, warp


def warp_pos(pos, warp_matrix):
    """BYTETracker.warp_pos (byte_tracker.py:653-657): float32 [2,3] @ [x, y, 1]."""
    p = np.array([pos[0], pos[1], 1.0], dtype=np.float32)
    return (np.asarray(warp_matrix, dtype=np.float32).reshape(2, 3) @ p).astype(np.float32)


def camera_motion_compensation(track_pool, last_image, current_frame, frame_id=2, number_of_iterations=100, termination_eps=0.00001,
                               warp_mode="MOTION_EUCLIDEAN", ctx=None):
    """BYTETracker.camera_motion_compensation (byte_tracker.py:626-650): estimate the previous->current frame warp and move every
    track of `track_pool` by it (`STrack.apply_camera_motion`, :123-137: position (mean[:2] or _tlwh[:2]) * scale -> warp ->
    / scale).  Returns the correlation coefficient (1.0 on the first frame, as the reference does)."""
    cc = 1.0
    if frame_id > 1 and last_image is not None:
        cc, warp = find_transform_ecc(last_image, current_frame, None, warp_mode, number_of_iterations, termination_eps, ctx=ctx)
        for t in track_pool:
            if hasattr(t, "apply_camera_motion"):
                t.apply_camera_motion(warp)
                continue
            holder = t.mean if getattr(t, "mean", None) is not None else t._tlwh
            new_pos = warp_pos(np.asarray(holder[:2], dtype=np.float64) * t.scale, warp) / t.scale
            holder[:2] = new_pos
    return cc


def recover_with_busca(probs_matrix, reliable, n_dets, busca_thresh):
    """Caller-side decision rule shared by the adapters (byte_tracker.py:504-527, StrongSORT tracker.py:347-371,
    GHOST tracker.py:776-800): lost track i is recovered at its own Kalman prediction iff its memory is reliable
    and probs[i, n_dets + i] > busca_thresh.  Returns (matches [[i, prob], ...], unmatched track indices)."""
    matches, unmatched = [], []
    if probs_matrix is None:
        return matches, unmatched
    for i in range(probs_matrix.shape[0]):
        pr = probs_matrix[i, n_dets + i]
        if reliable[i] and pr > busca_thresh:
            matches.append([i, pr])
        else:
            unmatched.append(i)
    return matches, unmatched
