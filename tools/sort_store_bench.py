#!/usr/bin/env python3
"""Time a StrongSORT frame with its Kalman state on the device (SortStore) against the object route it replaces (needs a GPU; bench.py is not involved).

    python tools/sort_store_bench.py [out.json] [reps=200]

50 tracks x 60 detections and 150 x 150.  Four fifths of the tracks are confirmed, the rest unconfirmed.  Every second detection sits on a track
(jittered by 2 % of the box height), the others are clutter; every fourth detection on a track carries a feature of its own, so the appearance
stage leaves it to the IoU stage.  One frame, as Tracker.predict / _match / update order it (adapters/StrongSORT/deep_sort/tracker.py):
  predict      of every track
  appearance   confirmed tracks x all detections: gallery distance, gate, MC blend (lambda 0.98), clamp at 0.3, assignment (opt.woC: one problem)
  iou          unconfirmed tracks and the confirmed ones the first stage left x the detections it left: iou_cost, clamp at 0.7, assignment
  update       of every matched pair with its detection's confidence (NSA Kalman), one call
  initiate     of the detections still unmatched, one call (into spare tracks / slots that never join, so every frame has the same shape)
The two routes (both run in this process, alternating inside one loop, 20 warm-up frames, host clock around a frame that ends in a stream
synchronisation; p50 in microseconds):
  store_us    SortStore.predict, .appearance_round, .iou_round, .update, .initiate: slot tables and detections go up, match vectors come down
  object_us   the per-track host filter StrongSORT runs - the numpy / Python restatement of tests/test_sort_store.py (predict, NSA update, iou_cost,
              initiate) on objects - with tracking.appearance_round (states up per call) and tracking.min_cost_matching
Both routes start from the same states and must return the same matches in the first frame (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one frame of each route enqueues (torch.profiler)
  state_gap   the largest |difference| of a mean entry between the two routes after the last frame, relative to max(1, |value|)

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kalman_store_bench import alternate, launches  # noqa: E402  (tools/ is this script's directory: one copy of the timing helpers)

CASES = [(50, 60), (150, 150)]
E = 128


def scene(k, n, m):
    """n track measurements on a grid with a unit feature each; m detections (xyah, tlwh, feature, confidence), every second one on a track."""
    from busca_amd import synth
    cols = int(np.ceil(np.sqrt(n)))
    h = synth.uniform(900 + k, "h", (n,), 60, 110).astype(np.float64)
    z = np.stack([150.0 + 130.0 * (np.arange(n) % cols), 150.0 + 260.0 * (np.arange(n) // cols), synth.uniform(900 + k, "a", (n,), 0.3, 0.5), h], 1)
    tf = synth.uniform(920 + k, "tf", (n, E), -1, 1).astype(np.float32)
    owner = (np.arange(m) * 7) % n
    jit = synth.uniform(910 + k, "jit", (m, 4), -1, 1).astype(np.float64)
    d = z[owner].copy()
    d[:, 0] += 0.02 * d[:, 3] * jit[:, 0]
    d[:, 1] += 0.02 * d[:, 3] * jit[:, 1]
    d[:, 3] *= 1.0 + 0.02 * jit[:, 3]
    clutter = np.arange(m) % 2 == 1
    d[clutter, 0] += 5000.0                                                    # off every track
    df = synth.uniform(930 + k, "df", (m, E), -1, 1).astype(np.float32)
    own = ~clutter & (np.arange(m) % 8 != 4)                                   # on a track and looking like it
    df[own] = tf[owner[own]] + 0.15 * df[own]
    tlwh = d.copy()
    tlwh[:, 2] *= tlwh[:, 3]
    tlwh[:, :2] -= tlwh[:, 2:] / 2
    conf = 0.5 + 0.499 * np.abs(jit[:, 2])
    return z, tf, d, tlwh, df, conf


def main():
    import torch
    from busca_amd import _lib, geometry, tracking
    from tests.test_kalman_filter import r_boxes, r_initiate
    from tests.test_sort_store import r_iou_cost, r_predict, r_update_nsa
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sort_store_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "sort_store_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(CASES):
        z, tf, xyah, tlwh, df, conf = scene(k, n, m)
        nc = 4 * n // 5
        ids = [100 + i for i in range(n)]
        metric = tracking.NearestNeighborDistanceMetric("cosine", 0.3, None, ctx=ctx)
        metric.partial_fit(tf[:nc], ids[:nc], ids[:nc])
        mean0, cov0 = r_initiate(z)
        tracks = [types.SimpleNamespace(mean=mean0[i].copy(), covariance=cov0[i].copy(), track_id=ids[i], time_since_update=1) for i in range(n)]
        spare = [types.SimpleNamespace(mean=None, covariance=None) for _ in range(m)]
        dets = [types.SimpleNamespace(to_xyah=(lambda v=xyah[j]: v), feature=df[j], tlwh=tlwh[j], confidence=float(conf[j])) for j in range(m)]
        store = tracking.SortStore(n + m)
        slots = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))          # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        store.load(slots, tracks)
        spare_slots = n + np.arange(m)
        tsu = [1] * n
        first = {}

        def store_frame():
            store.predict(slots)
            ma, ut, ud = store.appearance_round(metric, slots[:nc], ids[:nc], tsu[:nc], df, xyah, mc_lambda=0.98)
            cand = list(range(nc, n)) + sorted(ut)
            mb, _, ud_b = store.iou_round(slots[cand], tlwh, 0.7, detection_indices=ud)
            pairs = list(ma) + [(cand[r], j) for r, j in mb]
            store.update(slots[[i for i, _ in pairs]], xyah, [j for _, j in pairs], confidence=conf)
            store.initiate(spare_slots[:len(ud_b)], xyah, ud_b)
            if "store" not in first:
                first["store"] = (sorted((int(i), int(j)) for i, j in pairs), sorted(int(j) for j in ud_b))

        def iou_metric(trs, _dets, ti, di):
            return r_iou_cost(r_boxes(np.stack([trs[i].mean for i in ti]), False), tlwh[list(di)], [trs[i].time_since_update > 1 for i in ti])

        def object_frame():
            for t in tracks:
                t.mean, t.covariance = r_predict(t.mean, t.covariance)
            ma, ut, ud = tracking.appearance_round(metric, tracks, dets, list(range(nc)), None, mc_lambda=0.98, ctx=ctx, det_features=df)
            cand = list(range(nc, n)) + sorted(ut)
            mb, _, ud_b = tracking.min_cost_matching(iou_metric, 0.7, tracks, dets, cand, ud, ctx=ctx)
            pairs = list(ma) + list(mb)
            for i, j in pairs:
                tracks[i].mean, tracks[i].covariance = r_update_nsa(tracks[i].mean, tracks[i].covariance, xyah[j], dets[j].confidence)
            if len(ud_b):
                nm, ncov = r_initiate(xyah[list(ud_b)])
                for q in range(len(ud_b)):
                    spare[q].mean, spare[q].covariance = nm[q], ncov[q]
            if "object" not in first:
                first["object"] = (sorted((int(i), int(j)) for i, j in pairs), sorted(int(j) for j in ud_b))

        store_frame(); sync(); object_frame(); sync()
        assert first["store"] == first["object"], "the two routes disagree at %d x %d" % (n, m)
        ts, to, spread = alternate(store_frame, object_frame, reps, sync)
        back = [types.SimpleNamespace(mean=None, covariance=None) for _ in range(n)]
        store.store(slots, back)
        gap = max(float((np.abs(b.mean - t.mean) / np.maximum(1.0, np.abs(t.mean))).max()) for b, t in zip(back, tracks))
        n_iou = sum(1 for i, _ in first["store"][0] if i >= nc)
        rows.append(dict(case="StrongSORT frame %dx%d" % (n, m), pairs_per_frame=len(first["store"][0]), pairs_of_unconfirmed_tracks=n_iou,
                         initiations_per_frame=len(first["store"][1]), store_us=ts, object_us=to, store_p10_p90=spread[0], object_p10_p90=spread[1],
                         store_launches=launches(store_frame), object_launches=launches(object_frame), state_gap=gap))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/sort_store_bench.py", reps=reps, unit="us, p50 per frame", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
