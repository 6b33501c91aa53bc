#!/usr/bin/env python3
"""Time StrongSORT's Tracker._match as one staged assignment (SortStore.match) against the composition it replaces (needs a GPU; bench.py is not
involved).

    python tools/assign_stages_bench.py [out.json] [reps=200]

50 tracks x 60 detections and 150 x 150, the scene of tools/sort_store_bench.py: four fifths of the tracks confirmed, every second detection on a
track, every fourth of those with a feature of its own (the appearance stage leaves it to the IoU stage).  The confirmed tracks' ages
(time_since_update) are spread as a tracker's are: seven in ten at 1, the others - the lost ones - over 2 .. 30.  Only _match is timed; it does not
change the state, so every frame is the same frame.  Per shape two cases: the matching cascade at depth 30 (max_age) and opt.woC.  The two routes
(both in this process, alternating inside one loop, 20 warm-up frames, host clock around a call that ends with its results on the host; p50 in
microseconds):
  match_us    SortStore.match: gallery distance, gate into plane 0, iou_cost into plane 1, one table upload, busca_assign_stages, ONE copy
  rounds_us   SortStore.appearance_round(cascade_depth) + SortStore.iou_round wired as Tracker._match wires them (tracker.py:226-252): one index upload,
              two index_selects, one solve and one copy per populated level, then the IoU stage's upload, two launches and copy
Both routes must return the same matches (asserted before anything is timed).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one call of each route enqueues (torch.profiler)
  *_copies    device->host copies of one call (Tensor.cpu calls, counted)
  levels      cascade levels that hold tracks

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kalman_store_bench import alternate, launches  # noqa: E402  (tools/ is this script's directory: one copy of the timing helpers)
from sort_store_bench import CASES, scene  # noqa: E402

DEPTH = 30


def ages(nc):
    """time_since_update of nc confirmed tracks: seven in ten seen in the last frame, the others lost for 1 .. 29 frames."""
    return [1 if i % 10 < 7 else 2 + (i * 13) % 29 for i in range(nc)]


def copies(fn):
    import torch
    orig, n = torch.Tensor.cpu, [0]

    def cpu(self, *a, **k):
        n[0] += int(self.is_cuda)
        return orig(self, *a, **k)
    torch.Tensor.cpu = cpu
    try:
        fn()
    finally:
        torch.Tensor.cpu = orig
    return n[0]


def main():
    import torch
    from busca_amd import _lib, geometry, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "assign_stages_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "assign_stages_bench needs a GPU"
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
        store = tracking.SortStore(n)
        slots = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))          # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        store.initiate(slots, z)
        store.predict(slots)
        confirmed = [i < nc for i in range(n)]
        for depth in (DEPTH, None):
            tsu = (ages(nc) if depth is not None else [1] * nc) + [1] * (n - nc)
            got = {}

            def match_call():
                got["match"] = store.match(metric, slots, ids, tsu, confirmed, df, xyah, tlwh, 0.7, cascade_depth=depth, mc_lambda=0.98)

            def rounds_call():
                ma, ua, ud = store.appearance_round(metric, slots[:nc], ids[:nc], tsu[:nc], df, xyah, cascade_depth=depth, mc_lambda=0.98)
                cand = list(range(nc, n)) + [r for r in ua if tsu[r] == 1]
                left = [r for r in ua if tsu[r] != 1]
                mb, ub, ud = store.iou_round(slots[cand], tlwh, 0.7, stale=[tsu[r] > 1 for r in cand], detection_indices=ud)
                got["rounds"] = (list(ma) + [(cand[r], j) for r, j in mb], left + [cand[r] for r in ub], ud)

            match_call(); sync()
            staged = ctx.get_option("last_assign_staged")                       # of busca_assign_stages: the last solver launch so far
            rounds_call(); sync()
            a, b = got["match"], got["rounds"]
            assert sorted(a[0]) == sorted((int(i), int(j)) for i, j in b[0]) and set(a[1]) == set(b[1]) and set(a[2]) == set(b[2]), \
                "the two routes disagree at %d x %d" % (n, m)
            tm, tr, spread = alternate(match_call, rounds_call, reps, sync)
            levels = len(set(t for t in tsu[:nc] if t <= depth)) if depth is not None else 1
            rows.append(dict(case="_match %dx%d, %s" % (n, m, "cascade of depth %d" % depth if depth is not None else "woC"), levels=levels,
                             pairs_per_frame=len(a[0]), match_us=tm, rounds_us=tr, match_p10_p90=spread[0], rounds_p10_p90=spread[1],
                             match_launches=launches(match_call), rounds_launches=launches(rounds_call), match_copies=copies(match_call),
                             rounds_copies=copies(rounds_call), plane_staged_in_lds=staged))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/assign_stages_bench.py", reps=reps, unit="us, p50 per call", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
