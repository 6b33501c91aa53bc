#!/usr/bin/env python3
"""Time a StrongSORT frame as one chain on resident state (SortStore.frame) against the composition it replaces (needs a GPU; bench.py is not
involved).

    python tools/sort_frame_bench.py [out.json] [reps=200]

The scenes and the clock are those of tools/sort_store_bench.py and tools/assign_stages_bench.py: 50 tracks x 60 detections and 150 x 150, four
fifths of the tracks confirmed, every second detection on a track, every fourth of those with a feature of its own.  Per shape two cases: the
matching cascade at depth 30 with the confirmed tracks' ages spread (seven in ten at 1, the others over 2 .. 30), and opt.woC.  Every frame carries
a camera matrix.  New tracks go into spare slots that never join, so every frame has the same shape.  The two routes run on two stores loaded
alike, alternating inside one loop (20 warm-up frames, host clock around a frame that ends in a stream synchronisation; p50 in microseconds):
  frame_us     SortStore.frame: two uploads, busca_sframe_advance, busca_appearance_cost, busca_sframe_cost, busca_assign_stages,
               busca_sframe_apply, ONE copy home
  composed_us  the route of the parent commit: SortStore.camera_update, .predict, .match with a metric over the same feature rows, .update with
               the confidences, .initiate, and busca_store_ema_fit for the rows - the host between the assignment and the filter
Both routes must return the same matches and initiations in the first frame and leave the same states and feature rows, bit for bit, after the
last (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one frame of each route enqueues (torch.profiler)
  *_copies    device->host copies of one frame (Tensor.cpu calls, counted)

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from assign_stages_bench import DEPTH, ages, copies  # noqa: E402  (tools/ is this script's directory: one copy of the helpers)
from kalman_store_bench import alternate, launches  # noqa: E402
from sort_store_bench import CASES, E, scene  # noqa: E402

MATCH_THRESH, MAX_IOU, ALPHA, MC_LAMBDA = 0.3, 0.7, 0.9, 0.98
WARP = np.array([[0.999998, -0.002, 1.5], [0.002, 0.999998, -1.0], [0.0, 0.0, 1.0]])


class RowMetric:
    """What SortStore.match needs of a metric, over the feature rows of a store: the track ids are the slots."""

    def __init__(self, store, ctx):
        self.store, self.ctx, self.matching_threshold = store, ctx, MATCH_THRESH

    def distance(self, features, targets, device=False):
        from busca_amd import tracking
        out = tracking.appearance_cost(self.store.feat.view(self.store.capacity + 1, 1, -1), features, "min", slot=np.asarray(targets, dtype=np.int32),
                                       ctx=self.ctx)
        return out if device else out.cpu().numpy()


def main():
    import torch
    from busca_amd import _lib, _store_lib, geometry, tracking
    from busca_amd._xfer import small_to_dev
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sort_frame_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "sort_frame_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    slib = _store_lib.load()
    rows = []
    for k, (n, m) in enumerate(CASES):
        z, tf, xyah, tlwh, df, conf = scene(k, n, m)
        nc = 4 * n // 5
        xyah = tlwh.copy()                                                     # the measurements as frame() derives them: Detection.to_xyah of the boxes
        xyah[:, :2] += xyah[:, 2:] / 2
        xyah[:, 2] /= xyah[:, 3]
        tf = tf / np.linalg.norm(tf, axis=1, keepdims=True)
        slots = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))          # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        ids = [int(s) for s in slots]
        spare_slots = n + np.arange(m)
        confirmed = [i < nc for i in range(n)]
        d_df = torch.from_numpy(df).to(dev)                                    # the detection features are on the device already (the extractor's output)
        for depth in (DEPTH, None):
            tsu = (ages(nc) if depth is not None else [1] * nc) + [1] * (n - nc)
            stores = [tracking.SortStore(n + m, feature_dim=E) for _ in range(2)]      # [0] the chain's, [1] the composed route's: alike
            for st in stores:
                st.initiate(slots, z)
                st.load_features(slots, tf)
            metric = RowMetric(stores[1], ctx)
            first = {}

            def frame():
                got = stores[0].frame(slots, tsu, confirmed, tlwh, conf, d_df, MAX_IOU, MATCH_THRESH, ALPHA, free_slots=spare_slots, cascade_depth=depth,
                                      mc_lambda=MC_LAMBDA, camera_matrix=WARP)
                first.setdefault("frame", got)

            def composed():
                st = stores[1]
                st.camera_update(slots, WARP)
                st.predict(slots)
                pairs, _, ud = st.match(metric, slots, ids, tsu, confirmed, d_df, xyah, tlwh, MAX_IOU, cascade_depth=depth, mc_lambda=MC_LAMBDA)
                st.update(slots[[i for i, _ in pairs]], xyah, [j for _, j in pairs], confidence=conf)
                st.initiate(spare_slots[:len(ud)], xyah, ud)
                g = len(pairs) + len(ud)
                table = small_to_dev(np.concatenate([[ids[i] for i, _ in pairs], spare_slots[:len(ud)], [0] * len(pairs), [-1] * len(ud), np.arange(g + 1),
                                                     [j for _, j in pairs], ud]).astype(np.int32), dev, torch.int32)
                _store_lib.check(slib.busca_store_ema_fit(st.feat.data_ptr(), st.capacity + 1, 1, E, d_df.data_ptr(), m, table.data_ptr(),
                                                          table[g:].data_ptr(), table[2 * g:].data_ptr(), table[3 * g + 1:].data_ptr(), g, g, ALPHA,
                                                          dev.index, torch.cuda.current_stream(dev).cuda_stream))
                first.setdefault("composed", (pairs, ud))

            frame(); sync(); composed(); sync()
            got, (pairs, ud) = first["frame"], first["composed"]
            assert got.matches == [(int(i), int(j)) for i, j in pairs] and got.new_tracks == [(int(j), int(s)) for j, s in zip(ud, spare_slots)] \
                and not got.overflow, "the two routes disagree at %d x %d" % (n, m)
            tf_us, tc_us, spread = alternate(frame, composed, reps, sync)
            for name in ("mean", "cov", "feat"):
                assert torch.equal(getattr(stores[0], name), getattr(stores[1], name)), "%s differs after %d frames" % (name, reps + 21)
            rows.append(dict(case="StrongSORT frame %dx%d, %s" % (n, m, "cascade of depth %d" % depth if depth is not None else "woC"),
                             pairs_per_frame=len(got.matches), initiations_per_frame=len(got.new_tracks), frame_us=tf_us, composed_us=tc_us,
                             frame_p10_p90=spread[0], composed_p10_p90=spread[1], speedup=tc_us / tf_us, frame_launches=launches(frame),
                             composed_launches=launches(composed), frame_copies=copies(frame), composed_copies=copies(composed)))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/sort_frame_bench.py", reps=reps, unit="us, p50 per frame", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
