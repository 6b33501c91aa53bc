#!/usr/bin/env python3
"""Time one time step of S lock-step StrongSORT sequences on one store as one chain (SortStore.frame_batch) against the loop of S SortStore.frame
calls it replaces (needs a GPU; bench.py is not involved).

    python tools/sort_frame_batch_bench.py [out.json] [reps=200]

The scenes and the clock are those of tools/sort_frame_bench.py: 50 tracks x 60 detections and 150 x 150 per sequence, four fifths of the tracks
confirmed, every second detection on a track; per shape the matching cascade at depth 30 with the confirmed tracks' ages spread, and opt.woC.  S =
1, 2, 4, 8 and 16 sequences of the same scene live in disjoint slot ranges of one store, each with a camera matrix of its own; the detection
features are on the device already (the extractor's output).  New tracks go into spare slots that never join, so every step has the same shape.
The two routes run on two stores loaded alike, alternating inside one loop (20 warm-up steps, host clock around a step that ends in a stream
synchronisation; p50 in microseconds):
  batch_us    SortStore.frame_batch: two uploads, one torch.cat of the feature tables, busca_msframe_advance, busca_msframe_cost (the appearance
              entries inside), busca_assign_stages over the batch, busca_msframe_apply, ONE copy home
  loop_us     the route of the parent commit: S x SortStore.frame - per sequence two uploads, five launches and a copy home the host waits for
Both routes must return the same frames in the first step and leave the same states and feature rows, bit for bit, after the last (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one step of each route enqueues (torch.profiler): fixed per step on the new route, S times a frame's on the old
  *_copies    device->host copies of one step (Tensor.cpu calls, counted)
The parts of a step - uploads, kernels, the copy home, the host's own work - are not timed separately.

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from assign_stages_bench import DEPTH, ages, copies  # noqa: E402  (tools/ is this script's directory: one copy of the helpers)
from kalman_store_bench import alternate, launches  # noqa: E402
from sort_frame_bench import ALPHA, MATCH_THRESH, MAX_IOU, MC_LAMBDA  # noqa: E402
from sort_store_bench import CASES, E, scene  # noqa: E402

SEQUENCES = (1, 2, 4, 8, 16)
FIELDS = ("matches", "unmatched_tracks", "unmatched_detections", "new_tracks", "overflow")


def warp(s):
    """The camera matrix of sequence s: a small rotation and shift, different for every sequence."""
    t = 0.002 + 0.0001 * s
    return np.array([[np.cos(t), -np.sin(t), 1.5 + 0.25 * s], [np.sin(t), np.cos(t), -1.0 - 0.125 * s], [0.0, 0.0, 1.0]])


def main():
    import torch
    from busca_amd import _lib, geometry, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sort_frame_batch_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "sort_frame_batch_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(CASES):
        z, tf, _, tlwh, df, conf = scene(k, n, m)
        nc = 4 * n // 5
        tf = tf / np.linalg.norm(tf, axis=1, keepdims=True)
        perm = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))            # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        confirmed = [i < nc for i in range(n)]
        d_df = torch.from_numpy(df).to(dev)                                     # the detection features are on the device already
        for depth in (DEPTH, None):
            tsu = (ages(nc) if depth is not None else [1] * nc) + [1] * (n - nc)
            for S in SEQUENCES:
                home = [s * (n + m) for s in range(S)]                            # sequence s: its tracks and spare slots in [home, home + n + m)
                stores = [tracking.SortStore(S * (n + m), feature_dim=E) for _ in range(2)]      # [0] the batch's, [1] the loop's: alike
                for st in stores:
                    st.initiate(np.concatenate([h + perm for h in home]), np.concatenate([z] * S))
                    st.load_features(np.concatenate([h + perm for h in home]), np.concatenate([tf] * S))
                problems = [tracking.SortFrameProblem(h + perm, tsu, confirmed, tlwh, conf, d_df, h + n + np.arange(m), warp(s)) for s, h in enumerate(home)]

                def batch():
                    return stores[0].frame_batch(problems, MAX_IOU, MATCH_THRESH, ALPHA, cascade_depth=depth, mc_lambda=MC_LAMBDA)

                def loop():
                    return [stores[1].frame(p.slots, p.time_since_update, p.confirmed, p.det_tlwh, p.det_confidence, p.det_features, MAX_IOU, MATCH_THRESH,
                                            ALPHA, free_slots=p.free_slots, cascade_depth=depth, mc_lambda=MC_LAMBDA, camera_matrix=p.camera_matrix)
                            for p in problems]

                got, want = batch(), loop()
                sync()
                assert [[getattr(f, x) for x in FIELDS] for f in got] == [[getattr(f, x) for x in FIELDS] for f in want], "the routes disagree at S = %d" % S
                assert not any(f.overflow for f in got) and all(f.matches and f.new_tracks for f in got)
                tb, tl, spread = alternate(batch, loop, reps, sync)
                for name in ("mean", "cov", "feat"):
                    assert torch.equal(getattr(stores[0], name), getattr(stores[1], name)), "%s differs after %d steps" % (name, reps + 21)
                rows.append(dict(case="StrongSORT frame %dx%d, %s" % (n, m, "cascade of depth %d" % depth if depth is not None else "woC"), sequences=S,
                                 pairs_per_frame=len(got[0].matches), initiations_per_frame=len(got[0].new_tracks), batch_us=tb, loop_us=tl,
                                 batch_p10_p90=spread[0], loop_p10_p90=spread[1], speedup=tl / tb, batch_launches=launches(batch),
                                 loop_launches=launches(loop), batch_copies=copies(batch), loop_copies=copies(loop)))
                print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/sort_frame_batch_bench.py", reps=reps, unit="us, p50 per time step of S sequences", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
