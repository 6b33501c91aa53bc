#!/usr/bin/env python3
"""Time one time step of S lock-step GHOST sequences on one store as one chain (GhostStore.frame_batch) against the loop of S GhostStore.frame calls
it replaces (needs a GPU; bench.py is not involved).

    python tools/ghost_frame_batch_bench.py [out.json] [reps=200]

The scenes, the configurations and the clock are those of tools/ghost_frame_bench.py: 50 tracks x 60 detections and 150 x 150 per sequence, E = 512,
budget 32, history 32, four fifths of the tracks active, every track with three samples when the clock starts; the default configuration,
assign_separately and mv_avg proxies.  S = 1, 2 and 16 sequences of the same scene live in disjoint slot ranges of one store, each with its own
frame numbers; the detection features are on the device already (the extractor's output).  New tracks go into spare slots that never join, so
every step has the same shape.  The two routes run on two stores loaded alike, alternating inside one loop (20 warm-up steps, host clock around a
step that ends in a stream synchronisation; p50 in microseconds):
  batch_us    GhostStore.frame_batch: two uploads, one torch.cat of the feature tables, busca_mgframe_advance, the proxy launches on the whole slot
              list, busca_mgframe_distance, busca_mgframe_cost, one busca_linear_assignment over the batch (two in the separate mode),
              busca_mgframe_keep, busca_mgframe_apply, ONE copy home
  loop_us     the route of the parent commit: S x GhostStore.frame - per sequence two uploads, 11 - 14 launches and a copy home the host waits for
Both routes must return the same matches and new tracks in every compared step and leave the same state bits after the last (asserted).
  *_p10_p90        the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches       device kernels + copies one step of each route enqueues (torch.profiler)
  *_copies_home    blocking device->host copies of one step (Tensor.cpu calls, counted)
The parts of a step - uploads, kernels, the copy home, the host's own work - are not timed separately.

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ghost_frame_bench import BUDGET, CONFIGS, E, HISTORY  # noqa: E402
from tools.kalman_store_bench import CASES, alternate, launches, scene  # noqa: E402

SEQUENCES = (1, 2, 16)
STATE = ("_gallery", "_count", "_newest", "_mv_avg", "_mv_seen", "hist", "frames", "count", "newest", "pos", "vel")


def main():
    import torch
    from busca_amd import synth, tracking
    args = [a for a in sys.argv[1:]]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "ghost_frame_batch_bench.json")
    reps = int(args[1]) if len(args) > 1 else 200
    assert torch.cuda.is_available(), "ghost_frame_batch_bench needs a GPU"
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.current_stream(dev).synchronize()      # noqa: E731
    rows = []
    for k, (n, m) in enumerate(CASES):
        z, dets, scores = scene(k, n, m)
        boxes = np.stack([d.tlbr for d in dets])
        track_boxes = np.stack([z[:, 0] - z[:, 2] * z[:, 3] / 2, z[:, 1] - z[:, 3] / 2, z[:, 0] + z[:, 2] * z[:, 3] / 2, z[:, 1] + z[:, 3] / 2], 1)
        base = synth.uniform(900 + k, "base", (n, E), -1, 1).astype(np.float32)
        owner = (np.arange(m) * 7) % n
        noise = synth.uniform(910 + k, "noise", (m, E), -1, 1).astype(np.float32)
        feats = np.where((np.arange(m) % 2 == 1)[:, None], noise, base[owner] + 0.05 * noise).astype(np.float32)
        d_feats = torch.from_numpy(feats).to(dev)                  # the detection features are on the device already
        na = 4 * n // 5
        cap = n + m
        perm = np.random.RandomState(40 + k).permutation(cap)
        for name, cfg in CONFIGS.items():
            for S in SEQUENCES:
                seqs = [([int(s * cap + x) for x in perm[:na]], [int(s * cap + x) for x in perm[na:n]], [int(s * cap + x) for x in perm[n:]]) for s in range(S)]
                stores = [tracking.GhostStore(S * cap, BUDGET, E, HISTORY) for _ in range(2)]      # [0] the batch's, [1] the loop's: alike
                for st in stores:
                    for active, inactive, _ in seqs:
                        for q in range(3):
                            jit = synth.uniform(920 + q, "load", (n, E), -1, 1).astype(np.float32)
                            st.gallery.add(active + inactive, base + 0.05 * jit, new=[q == 0] * n)
                            st.motion.add(active + inactive, track_boxes + 0.5 * (q - 2), q, new=[q == 0] * n)
                clock = {"a": 3, "b": 3}
                seen = {}

                def batch():
                    t = clock["a"]
                    got = stores[0].frame_batch([tracking.GhostFrameProblem(a, i, d_feats, boxes, t + 100 * s, det_conf=scores, free_slots=f)
                                                 for s, (a, i, f) in enumerate(seqs)], cfg)
                    clock["a"] += 1
                    seen["a"] = [(g.matches, g.new) for g in got]

                def loop():
                    t = clock["b"]
                    got = [stores[1].frame(a, i, d_feats, boxes, t + 100 * s, cfg, det_conf=scores, free_slots=f) for s, (a, i, f) in enumerate(seqs)]
                    clock["b"] += 1
                    seen["b"] = [(g.matches, g.new) for g in got]
                batch(), loop()
                assert seen["a"] == seen["b"] and len(seen["a"][0][0]) >= n // 4, (name, n, m, S)
                tb, tl, spread = alternate(batch, loop, reps, sync)
                assert seen["a"] == seen["b"], (name, n, m, S)
                for x, y in ((stores[0].gallery, stores[1].gallery), (stores[0].motion, stores[1].motion)):
                    for key in STATE:
                        assert not hasattr(x, key) or torch.equal(getattr(x, key), getattr(y, key)), (name, S, key)

                def copies_home(fn):
                    count, orig = [0], torch.Tensor.cpu
                    torch.Tensor.cpu = lambda self, *a, **kw: (count.__setitem__(0, count[0] + int(self.is_cuda)), orig(self, *a, **kw))[1]
                    try:
                        fn()
                    finally:
                        torch.Tensor.cpu = orig
                    return count[0]
                rows.append(dict(config=name, tracks=n, detections=m, sequences=S, E=E, budget=BUDGET, history=HISTORY, matches_per_frame=len(seen["a"][0][0]),
                                 new_per_frame=len(seen["a"][0][1]), batch_us=tb, loop_us=tl, batch_p10_p90=spread[0], loop_p10_p90=spread[1],
                                 speedup=tl / tb, batch_copies_home=copies_home(batch), loop_copies_home=copies_home(loop),
                                 batch_launches=launches(batch), loop_launches=launches(loop)))
                print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(tool="tools/ghost_frame_batch_bench.py", device=torch.cuda.get_device_name(0), reps=reps, warmup=20,
                       unit="us, p50 per time step of S sequences", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
