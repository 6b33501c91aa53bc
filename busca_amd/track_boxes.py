"""Box-level helpers of the trackers: sentinel boxes, the pairwise distance matrices, duplicate removal, frame coverage and the BUSCA recovery
rule.  Fronts busca_pairwise, busca_duplicate_masks and busca_coverage of include/busca_hip.h; restates busca/tracking.py:7-60 and
adapters/ByteTrack/yolox/tracker/matching.py:53-91,173-186 and byte_tracker.py:459-465,504-527,574-623,653-657,685-698."""
import numpy as np
import torch

from . import _lib, geometry
from ._xfer import dev_of, stream_of

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


def remove_duplicate_stracks(stracksa, stracksb, ctx=None, thresh=0.15):
    """remove_duplicate_stracks (byte_tracker.py:685-698): of two tracks whose IoU cost is below 0.15 the one alive for
    fewer frames goes (ties: the one of the first list).  IoU cost and the marking both run on the GPU."""
    if len(stracksa) == 0 or len(stracksb) == 0:
        return list(stracksa), list(stracksb)
    ctx = ctx or geometry.default_context()
    dev = dev_of(ctx)
    cost = geometry.pairwise(ctx, _tlbrs(stracksa), _tlbrs(stracksb), _lib.PAIR_IOU_COST)
    age_a = torch.tensor([t.frame_id - t.start_frame for t in stracksa], dtype=torch.int32, device=dev)
    age_b = torch.tensor([t.frame_id - t.start_frame for t in stracksb], dtype=torch.int32, device=dev)
    keep_a = torch.empty(len(stracksa), dtype=torch.uint8, device=dev)
    keep_b = torch.empty(len(stracksb), dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.busca_duplicate_masks(ctx.h, cost.data_ptr(), len(stracksa), len(stracksb), age_a.data_ptr(), age_b.data_ptr(),
                                            float(thresh), keep_a.data_ptr(), keep_b.data_ptr(), stream_of(dev)))
    kab = torch.cat([keep_a, keep_b]).cpu().numpy()                              # one device->host copy for both masks
    ka, kb = kab[:len(stracksa)], kab[len(stracksa):]
    return [t for i, t in enumerate(stracksa) if ka[i]], [t for i, t in enumerate(stracksb) if kb[i]]


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
        dev = dev_of(ctx)
        r = torch.tensor(rects, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.check(ctx.lib.busca_coverage(ctx.h, r.data_ptr(), len(rects), H, W, cnt.data_ptr(), stream_of(dev)))
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


def warp_pos(pos, warp_matrix):
    """BYTETracker.warp_pos (byte_tracker.py:653-657): float32 [2,3] @ [x, y, 1]."""
    p = np.array([pos[0], pos[1], 1.0], dtype=np.float32)
    return (np.asarray(warp_matrix, dtype=np.float32).reshape(2, 3) @ p).astype(np.float32)


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
