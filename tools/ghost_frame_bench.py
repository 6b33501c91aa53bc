#!/usr/bin/env python3
"""Time a GHOST frame as one chain on resident state (GhostStore.frame) against the composed route it replaces (needs a GPU; bench.py is not involved).

    python tools/ghost_frame_bench.py [out.json] [reps=200]

50 tracks x 60 detections and 150 x 150 (the scenes of tools/kalman_store_bench.py: every second detection sits on a track, the others are clutter),
E = 512, budget 32, history 32.  Four fifths of the tracks are active, the rest inactive within patience; every track holds three samples when the
clock starts.  A detection on a track carries that track's feature with a little noise, clutter a feature of its own.  One frame of either route:
the motion step, the appearance distances (active: the newest sample, inactive: the mean over the samples), the blend with the IoU motion cost, the
solve, the reference's threshold filter, Track.add_detection of every assigned track, Track.__init__ of every unassigned confident detection (into
spare slots that never join the tracks, so every frame has the same shape).
  frame_us     GhostStore.frame: two uploads, the chain, one copy home
  composed_us  GhostGallery.state + ghost_round (which runs GhostMotion.cost) with the host filter behind its copy home (separate mode: a second
               linear_assignment on the compacted inactive block), then GhostGallery.add and GhostMotion.add for the matches and for the new tracks
Both routes run in this process on two stores loaded alike, alternating inside one loop (the clock of tools/kalman_store_bench.py: 20 warm-up
frames, host clock around a frame that ends in a stream synchronisation; p50 and p10-p90 in microseconds).  Both must return the same matches and
new tracks in every frame and leave the same state, bit for bit, after the last (asserted).
  *_launches   device kernels + copies one frame of each route enqueues (torch.profiler)
  *_copies_home   blocking device->host copies of one frame (Tensor.cpu calls)
Configurations: the default, assign_separately, and mv_avg proxies.

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.kalman_store_bench import CASES, alternate, launches, scene  # noqa: E402

E, BUDGET, HISTORY = 512, 32, 32
DEFAULT = dict(avg_act={"do": False, "num": 2, "proxy": "each_sample"}, avg_inact={"do": True, "num": 2, "proxy": "each_sample"}, act_reid_thresh=0.55,
               inact_reid_thresh=0.5, nan_first=False, assign_separately=False, new_track_conf=0.6,
               motion_config={"apply_motion_model": True, "combi": "sum_0.4", "last_n_frames": 3})
CONFIGS = {"default": DEFAULT, "separate": dict(DEFAULT, assign_separately=True),
           "mv_avg": dict(DEFAULT, avg_act={"do": True, "num": 0.9, "proxy": "mv_avg"}, avg_inact={"do": True, "num": 0.8, "proxy": "mv_avg"})}


def composed_frame(st, active, inactive, feats, boxes, frame, cfg, conf, free):
    """The frame by the older calls, with the host between the assignment and the state update -> (matches [(row, detection)], new [(detection, slot)])."""
    import torch
    from busca_amd import tracking
    na, n, m = len(active), len(active) + len(inactive), len(boxes)
    sep = cfg["assign_separately"]
    state = st.gallery.state(active, inactive, motion=st.motion)
    dist, row, col = tracking.ghost_round(state, feats, cfg=cfg, det_boxes=boxes)
    thr = (cfg["act_reid_thresh"], cfg["inact_reid_thresh"])
    if not sep:
        d = dist.cpu().numpy()
        pairs = [(int(r), int(c)) for r, c in zip(row, col) if d[r, c] < thr[0 if c < na else 1]]
    else:
        d_act, d_inact = dist[0].cpu().numpy(), dist[1]
        pairs = [(int(r), int(c)) for r, c in zip(row, col) if d_act[r, c] < thr[0]]
        left = sorted(set(range(m)) - {r for r, _ in pairs})
        if d_inact is not None and left:
            idx = torch.as_tensor(left, device=d_inact.device)
            compact = d_inact[idx]                                             # [detections left, inactive tracks]
            mt, _, _ = tracking.linear_assignment(compact.T.contiguous(), tracking.GHOST_LIMIT)
            c_host = compact.cpu().numpy()
            pairs += [(left[int(r)], na + int(t)) for t, r in sorted((int(t), int(r)) for t, r in mt) if c_host[r, t] < thr[1]]
    slots = list(active) + list(inactive)
    if pairs:
        s, j = [slots[c] for _, c in pairs], [r for r, _ in pairs]
        st.gallery.add(s, feats, det_index=j)
        st.motion.add(s, boxes, frame, det_index=j)
    taken = {r for r, _ in pairs}
    starts = [j for j in range(m) if j not in taken and conf[j] > cfg["new_track_conf"]][:len(free)]
    if starts:
        st.gallery.add(free[:len(starts)], feats, det_index=starts, new=[1] * len(starts))
        st.motion.add(free[:len(starts)], boxes, frame, det_index=starts, new=[1] * len(starts))
    return sorted((c, r) for r, c in pairs), list(zip(starts, free[:len(starts)]))


def main():
    import torch
    from busca_amd import synth, tracking
    args = [a for a in sys.argv[1:]]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "ghost_frame_bench.json")
    reps = int(args[1]) if len(args) > 1 else 200
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
        d_feats = torch.from_numpy(feats).to(dev)
        na = 4 * n // 5
        cap = n + m
        perm = np.random.RandomState(40 + k).permutation(cap)
        active, inactive, free = [int(s) for s in perm[:na]], [int(s) for s in perm[na:n]], [int(s) for s in perm[n:]]
        for name, cfg in CONFIGS.items():
            stores = [tracking.GhostStore(cap, BUDGET, E, HISTORY) for _ in range(2)]
            for st in stores:
                for q in range(3):
                    jit = synth.uniform(920 + q, "load", (n, E), -1, 1).astype(np.float32)
                    st.gallery.add(active + inactive, base + 0.05 * jit, new=[q == 0] * n)
                    st.motion.add(active + inactive, track_boxes + 0.5 * (q - 2), q, new=[q == 0] * n)
            clock = {"a": 3, "b": 3}
            seen = {}

            def frame_route():
                got = stores[0].frame(active, inactive, d_feats, boxes, clock["a"], cfg, det_conf=scores, free_slots=free)
                clock["a"] += 1
                seen["a"] = (got.matches, got.new)

            def composed_route():
                seen["b"] = composed_frame(stores[1], active, inactive, d_feats, boxes, clock["b"], cfg, scores, free)
                clock["b"] += 1
            frame_route(), composed_route()
            assert seen["a"] == seen["b"] and len(seen["a"][0]) >= n // 4, (name, n, m, len(seen["a"][0]))
            tf, tc, spread = alternate(frame_route, composed_route, reps, sync)
            assert seen["a"] == seen["b"], (name, n, m)
            for x, y in ((stores[0].gallery, stores[1].gallery), (stores[0].motion, stores[1].motion)):
                for key in ("_gallery", "_count", "_newest", "_mv_avg", "_mv_seen", "hist", "frames", "count", "newest", "pos", "vel"):
                    assert not hasattr(x, key) or torch.equal(getattr(x, key), getattr(y, key)), (name, key)

            def copies_home(fn):
                count, orig = [0], torch.Tensor.cpu
                torch.Tensor.cpu = lambda self, *a, **kw: (count.__setitem__(0, count[0] + int(self.is_cuda)), orig(self, *a, **kw))[1]
                try:
                    fn()
                finally:
                    torch.Tensor.cpu = orig
                return count[0]
            rows.append(dict(config=name, tracks=n, detections=m, E=E, budget=BUDGET, history=HISTORY, matches=len(seen["a"][0]), new=len(seen["a"][1]),
                             frame_us=tf, composed_us=tc, frame_p10_p90=spread[0], composed_p10_p90=spread[1],
                             frame_copies_home=copies_home(frame_route), composed_copies_home=copies_home(composed_route),
                             frame_launches=launches(frame_route), composed_launches=launches(composed_route)))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=reps, warmup=20, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
