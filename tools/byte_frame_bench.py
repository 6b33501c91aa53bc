#!/usr/bin/env python3
"""Time a ByteTrack frame as one chain on resident state (KalmanStore.frame) against the composition it replaces (needs a GPU; bench.py is not
involved).

    python tools/byte_frame_bench.py [out.json] [reps=200]

The scenes, the frame and the clock are those of tools/kalman_store_bench.py: 50 tracks x 60 detections and 150 x 150, four fifths of the tracks the
pool (every tenth of them Lost), the rest unconfirmed; two thirds of the detections high-score, every second detection on a track.  The two routes
run on two stores loaded alike, alternating inside one loop (20 warm-up frames, host clock around a frame that ends in a stream synchronisation; p50
in microseconds):
  frame_us    KalmanStore.frame: two uploads, predict, busca_frame_cost, busca_assign_stages, busca_frame_apply, ONE copy home
  rounds_us   the route of the parent commit as kalman_store_bench.py composes a frame: KalmanStore.round x 3 with the lists compacted on the host
              between them, .update, .initiate - an upload, a cost launch, a solver launch and a copy home per round, and the host between the
              assignment and the filter
Both routes must return the same matches and initiations in the first frame and leave the same states, bit for bit, after the last (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one frame of each route enqueues (torch.profiler): the figure that is fixed per frame on the new route

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kalman_store_bench as ksb  # noqa: E402

TRACK_THRESH, MATCH_THRESH, DET_THRESH = 0.6, 0.8, 0.7      # the scene's high scores are 0.85 .. 0.9, its low ones 0.25 .. 0.3


def main():
    import torch
    from busca_amd import _lib, geometry, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "byte_frame_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "byte_frame_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(ksb.CASES):
        z, dets, scores = ksb.scene(k, n, m)
        n_pool, mh = 4 * n // 5, 2 * m // 3
        assert (scores[:mh] > DET_THRESH).all() and (scores[mh:] < TRACK_THRESH).all() and (scores[mh:] > 0.1).all()
        not_tracked = np.arange(n_pool) % 10 == 9
        mean0, cov0 = tracking.multi_initiate(z, ctx=ctx)
        slots = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))          # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        spare_slots = n + np.arange(m)
        stores = [tracking.KalmanStore(n + m) for _ in range(2)]              # [0] the chain's, [1] the rounds': alike, so both routes see the same states
        for st in stores:
            st.load(slots, [ksb.Track(mean0[i], cov0[i], 1) for i in range(n)])
        seq = types.SimpleNamespace(slots=slots, spare_slots=spare_slots, dets=dets, high=dets[:mh], low=dets[mh:], scores=scores, n_pool=n_pool, mh=mh,
                                    not_tracked=not_tracked)

        def frame():
            return stores[0].frame(slots[:n_pool], not_tracked, slots[n_pool:], dets, scores, TRACK_THRESH, MATCH_THRESH, DET_THRESH, free_slots=spare_slots)

        def rounds():
            return ksb.sequence_frame(stores[1], seq)

        got = frame()
        pairs, new = rounds()
        sync()
        a = (sorted([(int(slots[r]), j) for r, j in got.first + got.second] + [(int(slots[n_pool + r]), j) for r, j in got.unconfirmed]),
             [(j, s) for j, s in got.new_tracks])
        b = (sorted((int(s), int(j)) for s, j in pairs), [(int(j), int(s)) for j, s in zip(new, spare_slots)])
        assert a == b and not got.overflow, "the two routes disagree at %d x %d" % (n, m)
        tf, tr, spread = ksb.alternate(frame, rounds, reps, sync)
        assert torch.equal(stores[0].mean, stores[1].mean) and torch.equal(stores[0].cov, stores[1].cov), "states differ after %d frames" % (reps + 21)
        rows.append(dict(case="ByteTrack frame %dx%d" % (n, m), first=len(got.first), second=len(got.second), unconfirmed=len(got.unconfirmed),
                         initiations_per_frame=len(got.new_tracks), frame_us=tf, rounds_us=tr, frame_p10_p90=spread[0], rounds_p10_p90=spread[1],
                         speedup=tr / tf, frame_launches=ksb.launches(frame), rounds_launches=ksb.launches(rounds)))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/byte_frame_bench.py", reps=reps, unit="us, p50 per frame", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
