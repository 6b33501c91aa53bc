"""ByteTrack's Kalman filter for all tracks of a call at once: prediction, measurement update, initiation, gating distances, and the gated /
blended cost matrix of an association round.  Fronts the busca_kalman_* entry points of include/busca_hip.h; restates
adapters/ByteTrack/yolox/tracker/kalman_filter.py, matching.py:132-156 and byte_tracker.py:50-61,67,78,109,165-172.
Tracks are objects with `.mean` [8], `.covariance` [8,8] and `.state`; every call makes one device->host copy.  kalman_store.KalmanStore is the same
filter on state that stays on the device."""
import numpy as np
import torch

from . import _lib, geometry
from ._xfer import dev_of, stream_of, to_dev
from .track_boxes import _tlbrs

TRACKED = 1     # TrackState.Tracked (adapters/*/mot_online/basetrack.py:5-9)
CHI2INV95 = {2: 5.9915, 4: 9.4877}      # kalman_filter.py:10-19, the gates of only_position=True / False
_METRICS = {"maha": 0, "gaussian": 1}


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


def _set_states(stracks, host):
    """The tracks' states from the leading 72 n doubles of a download: n means, then n covariances."""
    n = len(stracks)
    pm, pc = host[:8 * n].reshape(n, 8).copy(), host[8 * n:72 * n].reshape(n, 8, 8).copy()
    for i, st in enumerate(stracks):
        st.mean = pm[i]
        st.covariance = pc[i]


def _raise_flagged(status, what):
    bad = np.nonzero(status)[0]
    if len(bad):
        raise np.linalg.LinAlgError("%s: the projected covariance of track %d is not positive definite (%d of %d tracks)"
                                    % (what, int(bad[0]), len(bad), len(status)))


def _download_with_status(mat, status, what):
    """One device->host copy of a [n,m] matrix and its tracks' status words."""
    n, m = mat.shape
    host = torch.cat([mat.reshape(-1), status.to(torch.float64)]).cpu().numpy()
    _raise_flagged(host[n * m:], what)
    return host[:n * m].reshape(n, m).copy()


def _download_round(stracks, mean, cov, payload, status, what):
    """The single device->host copy of an association round: the predicted states, which the tracks get, then `payload` (a device float64 tensor,
    or None) and the Kalman status words (or None), which raise LinAlgError as `what`.  -> the payload as a flat host array, or None."""
    parts = [mean.view(-1), cov.view(-1)]
    if payload is not None:
        parts.append(payload.view(-1))
        if status is not None:
            parts.append(status.to(torch.float64))
    host = torch.cat(parts).cpu().numpy()
    _set_states(stracks, host)
    if payload is None:
        return None
    lo, hi = 72 * len(stracks), 72 * len(stracks) + payload.numel()
    if status is not None:
        _raise_flagged(host[hi:], what)
    return host[lo:hi]


def _predict_dev(ctx, stracks, dev):
    """busca_kalman_multi_predict of the uploaded states -> device (mean [n,8], cov [n,8,8])."""
    mean, cov = _upload_states(stracks, dev)
    nt = torch.from_numpy(np.asarray([st.state != TRACKED for st in stracks], dtype=np.uint8)).to(dev)
    ctx.check(ctx.lib.busca_kalman_multi_predict(ctx.h, mean.data_ptr(), cov.data_ptr(), nt.data_ptr(), len(stracks), stream_of(dev)))
    return mean, cov


def multi_predict(stracks, ctx=None):
    """STrack.multi_predict (adapters/ByteTrack/yolox/tracker/byte_tracker.py:50-61) on the GPU: constant-velocity Kalman
    prediction of every track's (mean [8], covariance [8,8]) in place; `mean[7]` of non-Tracked tracks is zeroed first."""
    if len(stracks) == 0:
        return
    ctx, dev = geometry.ctx_dev(ctx)
    mean, cov = _predict_dev(ctx, stracks, dev)
    _set_states(stracks, torch.cat([mean.view(-1), cov.view(-1)]).cpu().numpy())      # one device->host copy for both


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
    ctx, dev = geometry.ctx_dev(ctx)
    mean, cov = _upload_states(stracks, dev)
    meas = torch.from_numpy(_measurements(detections)).to(dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.busca_kalman_update(ctx.h, mean.data_ptr(), cov.data_ptr(), meas.data_ptr(), n, status.data_ptr(), stream_of(dev)))
    host = torch.cat([mean.view(-1), cov.view(-1), status.to(torch.float64)]).cpu().numpy()     # one device->host copy for all three
    _set_states(stracks, host)
    _raise_flagged(host[72 * n:], "multi_update")


def multi_initiate(detections, ctx=None):
    """KalmanFilter.initiate (kalman_filter.py:54-85) of every new detection, as STrack.activate calls it (byte_tracker.py:67):
    -> (mean [n,8], covariance [n,8,8]) float64."""
    meas = _measurements(detections)
    n = meas.shape[0]
    if n == 0:
        return np.zeros((0, 8)), np.zeros((0, 8, 8))
    ctx, dev = geometry.ctx_dev(ctx)
    z = torch.from_numpy(meas).to(dev)
    both = torch.empty(n * 72, dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.busca_kalman_initiate(ctx.h, z.data_ptr(), n, both.data_ptr(), both.data_ptr() + 64 * n, stream_of(dev)))
    host = both.cpu().numpy()
    return host[:8 * n].reshape(n, 8).copy(), host[8 * n:].reshape(n, 8, 8).copy()


def _gating_dev(ctx, mean, cov, meas, only_position, metric):
    """Device [n,m] gating distances and the [n] int32 status words of device states and measurements."""
    n, m = mean.shape[0], meas.shape[0]
    out = torch.empty(n, m, dtype=torch.float64, device=mean.device)
    status = torch.zeros(n, dtype=torch.int32, device=mean.device)
    ctx.check(ctx.lib.busca_kalman_gating(ctx.h, mean.data_ptr(), cov.data_ptr(), n, meas.data_ptr(), m, int(bool(only_position)), metric,
                                          out.data_ptr(), status.data_ptr(), stream_of(mean.device)))
    return out, status


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
    ctx, dev = geometry.ctx_dev(ctx)
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
    ctx, dev = geometry.ctx_dev(ctx)
    cost = to_dev(cost, dev, torch.float64).reshape(n, m)
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
    dev = dev_of(ctx)
    mean, cov = _predict_dev(ctx, stracks, dev)
    cost = status = None
    if m > 0:
        boxes = torch.empty(n, 4, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, mean.data_ptr(), n, 1, boxes.data_ptr(), stream_of(dev)))
        cost = geometry.pairwise(ctx, boxes, _tlbrs(detections), _lib.PAIR_IOU_COST, scores_b=det_scores)
        if fuse_motion:
            gate, status = _gating_dev(ctx, mean, cov, torch.from_numpy(_measurements(detections)).to(dev), only_position, 0)
            cost = _gate_dev(cost, gate, only_position, float(lambda_))
    return mean, cov, cost, status


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
    host = _download_round(stracks, mean, cov, cost, status, "predicted_cost")       # states, cost matrix, status words
    return np.zeros((n, 0), dtype=np.float64) if m == 0 else host.reshape(n, m).copy()
