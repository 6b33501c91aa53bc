#!/usr/bin/env python3
"""Time one time step of S lock-step ByteTrack sequences on one store as one chain (KalmanStore.frame_batch) against the loop of S
KalmanStore.frame calls it replaces (needs a GPU; bench.py is not involved).

    python tools/byte_frame_batch_bench.py [out.json] [reps=200]

The scenes and the clock are those of tools/byte_frame_bench.py: 50 tracks x 60 detections and 150 x 150 per sequence, four fifths of the tracks the
pool (every tenth of them Lost), the rest unconfirmed; two thirds of the detections high-score, every second detection on a track.  S = 1, 2, 4, 8
and 16 sequences of the same scene live in disjoint slot ranges of one store.  The two routes run on two stores loaded alike, alternating inside
one loop (20 warm-up steps, host clock around a step that ends in a stream synchronisation; p50 in microseconds):
  batch_us    KalmanStore.frame_batch: two uploads, predict, busca_mframe_cost, busca_assign_stages over the batch, busca_mframe_apply, ONE copy home
  loop_us     the route of the parent commit: S x KalmanStore.frame - per sequence two uploads, four launches and a copy home the host waits for
Both routes must return the same frames in the first step and leave the same states, bit for bit, after the last (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one step of each route enqueues (torch.profiler): fixed per step on the new route, S times a frame's on the old

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kalman_store_bench as ksb  # noqa: E402
from byte_frame_bench import DET_THRESH, MATCH_THRESH, TRACK_THRESH  # noqa: E402

SEQUENCES = (1, 2, 4, 8, 16)
FIELDS = ("first", "second", "unconfirmed", "unmatched_pool", "unmatched_unconfirmed", "new_tracks", "overflow")


def main():
    import torch
    from busca_amd import _lib, geometry, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "byte_frame_batch_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "byte_frame_batch_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(ksb.CASES):
        z, dets, scores = ksb.scene(k, n, m)
        n_pool = 4 * n // 5
        not_tracked = np.arange(n_pool) % 10 == 9
        mean0, cov0 = tracking.multi_initiate(z, ctx=ctx)
        perm = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))            # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        for S in SEQUENCES:
            home = [s * (n + m) for s in range(S)]                                # sequence s: its tracks and spare slots in [home, home + n + m)
            stores = [tracking.KalmanStore(S * (n + m)) for _ in range(2)]       # [0] the batch's, [1] the loop's: alike, so both routes see the same states
            for st in stores:
                st.load(np.concatenate([h + perm for h in home]), [ksb.Track(mean0[i], cov0[i], 1) for i in range(n)] * S)
            problems = [tracking.FrameProblem(h + perm[:n_pool], not_tracked, h + perm[n_pool:], dets, scores, h + n + np.arange(m)) for h in home]

            def batch():
                return stores[0].frame_batch(problems, TRACK_THRESH, MATCH_THRESH, DET_THRESH)

            def loop():
                return [stores[1].frame(p.pool_slots, p.lost, p.unconfirmed_slots, p.detections, p.det_scores, TRACK_THRESH, MATCH_THRESH, DET_THRESH,
                                        free_slots=p.free_slots) for p in problems]

            got, want = batch(), loop()
            sync()
            assert [[getattr(f, x) for x in FIELDS] for f in got] == [[getattr(f, x) for x in FIELDS] for f in want], "the routes disagree at S = %d" % S
            assert not any(f.overflow for f in got) and all(f.first and f.new_tracks for f in got)
            tb, tl, spread = ksb.alternate(batch, loop, reps, sync)
            assert torch.equal(stores[0].mean, stores[1].mean) and torch.equal(stores[0].cov, stores[1].cov), "states differ after %d steps" % (reps + 21)
            rows.append(dict(case="ByteTrack frame %dx%d" % (n, m), sequences=S, first=len(got[0].first), second=len(got[0].second),
                             unconfirmed=len(got[0].unconfirmed), initiations_per_frame=len(got[0].new_tracks), batch_us=tb, loop_us=tl,
                             batch_p10_p90=spread[0], loop_p10_p90=spread[1], speedup=tl / tb, batch_launches=ksb.launches(batch),
                             loop_launches=ksb.launches(loop)))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/byte_frame_batch_bench.py", reps=reps, unit="us, p50 per time step of S sequences", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
