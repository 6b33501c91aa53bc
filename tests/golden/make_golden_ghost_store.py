#!/usr/bin/env python3
"""Generate tests/golden/ghost_store.npz, the fixture of tests/test_ghost_store.py.  Run from the repo root where the reference is present:

    python tests/golden/make_golden_ghost_store.py

Real Track objects of the reference (adapters/GHOST/src/tracking_utils.py, loaded as make_golden_ghost.py loads it) are driven on the CPU through a
scripted sequence - Track(...) when the script starts a track, add_detection(...) when it matches one - and get_proxy is called on them after every
frame.  The fixture holds arrays only: the script, the detection features and what get_proxy returned.

E = 32, budget 4 (the ring the device keeps; the reference keeps everything), 8 slots, 12 frames, 6 tracks:
  track 0 (slot 5)   matched in every frame: 12 samples, a ring of 4 wraps twice; its feature of frame 2 repeats that of frame 1 (a median tie)
  track 1 (slot 0)   matched in frames 0-3, inactive in 4-7, matched again from 8
  track 2 (slot 3)   matched in frames 0-5, released at frame 6
  track 3 (slot 7)   born at frame 5
  track 4 (slot 1)   matched in frames 0-1, inactive from 2 on
  track 5 (slot 3)   born at frame 8 in the slot track 2 left
A frame: releases, then adds, then the queries over the live tracks, those matched in this frame (active) first.

  params [5]                     E, budget, capacity, frames, tracks;  tie [2]: slot and frame of the repeated feature
  det_<f> [m,E] f32              the detections' features of frame f (seeded normals; one row more than there are matches)
  adds_<f> [k,3]                 slot, detection row, new flag of every add;  release_<f>, active_<f>, inactive_<f>: slot lists
  px_<f>_<mode>_<num> [n,E] f32  get_proxy over active + inactive: last, and mean / median / meannorm with num 3 and 'all'.  'all' is recorded only
                                 where no queried track has more than `budget` samples (elsewhere the reference averages samples the ring has
                                 dropped); meannorm with num 3 only where every queried track has fewer than 3 (its num <= len branch raises in the
                                 reference: F.normalize over dim 1 of a vector)
  err_<f>_<mode>_<num>           mean / meannorm: the largest difference between the reference's float32 output and a float64 numpy restatement
  mv_px_<f> [n,E] f32            get_proxy with proxy 'mv_avg': num 0.9 for the active tracks, then num 0.5 for the inactive ones, on one mv_avg dict
  mv_tab_<f> [capacity,E] f32, mv_seen_<f> [capacity] u8     that dict after the two calls, by the slot of the live track that owns the entry

Every recorded array is also reproduced bit for bit by the plain-numpy restatement of tests/test_ghost_store.py (asserted here)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from busca_amd import synth  # noqa: E402
from make_golden_ghost import load_reference  # noqa: E402
from tests.test_ghost_store import A_ACT, A_INACT, BUDGET, CAPACITY, E, FRAMES, MODES, TRACKS, NpStore  # noqa: E402

SEED = 610
SLOT = {0: 5, 1: 0, 2: 3, 3: 7, 4: 1, 5: 3}
MATCHED = {0: range(0, 12), 1: [0, 1, 2, 3, 8, 9, 10, 11], 2: range(0, 6), 3: range(5, 12), 4: [0, 1], 5: range(8, 12)}      # the frames with a detection
RELEASED = {2: 6}                                                                                                               # track: frame
TIE = (0, 2)                                                                                                                    # track, frame: repeats its previous feature


def main():
    tu = load_reference()[0]
    out = dict(params=np.array([E, BUDGET, CAPACITY, FRAMES, TRACKS], dtype=np.int64), tie=np.array([SLOT[TIE[0]], TIE[1]], dtype=np.int64))
    tracks, mv_avg, samples = {}, {}, {}
    rest = NpStore(CAPACITY, BUDGET, E)
    prev_feat = {}
    all_frames = wrapped_frames = 0
    for f in range(FRAMES):
        matched = [t for t in range(TRACKS) if f in MATCHED[t]]
        m = len(matched) + 1
        det = synth.normal(SEED + f, "det", (m, E))
        order = np.argsort(synth.uniform(SEED + f, "order", (m,)), kind="stable")[:len(matched)]      # which detection row each matched track takes
        if f == TIE[1]:
            det[order[matched.index(TIE[0])]] = prev_feat[TIE[0]]
        released = [t for t, fr in RELEASED.items() if fr == f]
        for t in released:
            del tracks[t]
        adds = []
        for t, row in zip(matched, order):
            feat = torch.from_numpy(det[row].copy())
            box = np.array([10.0 * t, 20.0, 10.0 * t + 30.0, 90.0])
            new = t not in tracks
            if new:
                tracks[t] = tu.Track(track_id=100 + t, bbox=box, feats=feat, im_index=int(row), gt_id=t, vis=1.0, conf=0.9, frame=f, label=0)
                samples[t] = 0
            else:
                tracks[t].add_detection(bbox=box, feats=feat, im_index=int(row), gt_id=t, vis=1.0, conf=0.9, frame=f, label=0)
            samples[t] += 1
            prev_feat[t] = det[row].copy()
            adds.append([SLOT[t], int(row), int(new)])
        adds = np.array(adds, dtype=np.int64).reshape(-1, 3)
        active = [t for t in sorted(tracks) if t in matched]
        inactive = [t for t in sorted(tracks) if t not in matched]
        queried = active + inactive
        assert len(set(SLOT[t] for t in queried)) == len(queried)
        slots = [SLOT[t] for t in queried]
        out.update({"det_%d" % f: det, "adds_%d" % f: adds, "release_%d" % f: np.array([SLOT[t] for t in released], dtype=np.int64),
                    "active_%d" % f: np.array([SLOT[t] for t in active], dtype=np.int64), "inactive_%d" % f: np.array([SLOT[t] for t in inactive], dtype=np.int64)})
        rest.release([SLOT[t] for t in released])
        rest.add(adds[:, 0], det, adds[:, 1], adds[:, 2])
        longest = max(samples[t] for t in queried)
        shortest_all = longest < 3
        all_frames += longest <= BUDGET
        wrapped_frames += longest > BUDGET
        curr = {100 + t: tracks[t] for t in queried}
        for mode, num in MODES:
            if (num == "all" and longest > BUDGET) or (mode == "meannorm" and num == 3 and not shortest_all):
                continue
            ref = tu.get_proxy(curr_it=curr, mode="act", tracker_cfg={"avg_act": {"num": num, "proxy": mode}}, mv_avg=None).numpy()
            assert ref.shape == (len(queried), E) and ref.dtype == np.float32
            key = "%d_%s_%s" % (f, mode, num)
            out["px_" + key] = ref
            mine = rest.proxy(slots, mode, num)
            assert np.array_equal(mine, ref), "the numpy restatement differs from the reference at " + key
            if mode in ("mean", "meannorm"):
                r64 = []
                for t in queried:
                    w = np.stack([p.numpy() for p in tracks[t].past_feats])
                    w = w if num == "all" or len(w) < num else w[-num:]
                    mu = w.astype(np.float64).mean(0)
                    if mode == "meannorm":
                        mu = mu.astype(np.float32).astype(np.float64)
                        mu = mu / max(np.sqrt((mu * mu).sum()), 1e-12)
                    r64.append(mu)
                out["err_" + key] = np.float64(np.abs(np.asarray(r64) - ref).max())
                assert out["err_" + key] < 1e-6
        parts = []
        for group, a in ((active, A_ACT), (inactive, A_INACT)):
            if group:
                parts.append(tu.get_proxy(curr_it={100 + t: tracks[t] for t in group}, mode="act", tracker_cfg={"avg_act": {"num": a, "proxy": "mv_avg"}},
                                          mv_avg=mv_avg).numpy())
        px = np.concatenate(parts)
        tab, seen = np.zeros((CAPACITY, E), dtype=np.float32), np.zeros(CAPACITY, dtype=np.uint8)
        for t in queried:
            tab[SLOT[t]], seen[SLOT[t]] = mv_avg[100 + t].numpy(), 1
        mine = np.concatenate([rest.mv([SLOT[t] for t in active], A_ACT), rest.mv([SLOT[t] for t in inactive], A_INACT)])
        assert np.array_equal(mine, px) and np.array_equal(rest.mv_avg[slots], tab[slots]) and np.array_equal(rest.mv_seen, seen), f
        out.update({"mv_px_%d" % f: px, "mv_tab_%d" % f: tab, "mv_seen_%d" % f: seen})
        print("frame %2d: %d adds (%d new), %d released, %d active + %d inactive, longest track %2d, recorded %s"
              % (f, len(adds), int(adds[:, 2].sum()), len(released), len(active), len(inactive), longest,
                 " ".join(sorted(k[len("px_%d_" % f):] for k in out if k.startswith("px_%d_" % f)))))
    assert all_frames >= 3 and wrapped_frames >= 3, (all_frames, wrapped_frames)
    assert max(samples.values()) == FRAMES and len(samples) == TRACKS
    path = os.path.join(OUT, "ghost_store.npz")
    np.savez_compressed(path, **out)
    print("wrote ghost_store.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
