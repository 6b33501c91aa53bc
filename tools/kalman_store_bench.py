#!/usr/bin/env python3
"""Time a ByteTrack frame with its Kalman state on the device (KalmanStore) against the object route it replaces (needs a GPU; bench.py is not involved).

    python tools/kalman_store_bench.py [out.json] [reps=200]

50 tracks x 60 detections and 150 x 150.  Four fifths of the tracks are the pool (every tenth of them Lost), the rest unconfirmed; two thirds of
the detections are high-score.  Every second detection sits on a track (jittered by 2 % of the box height), the others are clutter.  One frame:
  round 1   pool x high detections, prediction, IoU cost with fuse_score, thresh 0.8
  round 2   the pool tracks round 1 left x low detections, IoU cost, thresh 0.5 (no second prediction)
  round 3   unconfirmed tracks x the high detections round 1 left, IoU cost with fuse_score, thresh 0.7
  update    of every matched pair of the three rounds, one call
  initiate  of the detections still unmatched, one call (into spare tracks / slots that never join the pool, so every frame has the same shape)
The two routes (both run in this process, alternating inside one loop, 20 warm-up frames, host clock around a frame that ends in a stream
synchronisation; p50 in microseconds):
  store_us    KalmanStore.round x 3 (predict=False in rounds 2 and 3), .update, .initiate: slot tables and detections go up, match vectors come down
  object_us   the code paths this repository had before: associate_round (round 1: states up, states and matches down), iou_distance +
              linear_assignment (rounds 2 and 3, on the objects' boxes), multi_update (states up and down), multi_initiate (states down)
Both routes see the same states and must return the same matches in the first frame (asserted).
  *_p10_p90   the 10th and 90th percentile of the same samples: the spread to read a difference of two p50 against
  *_launches  device kernels + copies one frame of each route enqueues (torch.profiler)
  cost_us / chain_us   the cost matrix of a fuse_motion round alone, on states and detections already on the device: busca_track_round_cost (one
              launch) against busca_kalman_boxes + busca_pairwise (with its zero-fill) + busca_kalman_gating + torch.where + the blend

    python tools/kalman_store_bench.py --sequences 1 2 4 8 16 [out.json] [reps=200]

S sequences in lock-step over ONE store of S x (n + m) slots, each with the frame above on a scene of its own; written to
profiles/kalman_store_batch_bench.json.  The two routes run on two stores loaded alike, alternating inside one loop as above:
  loop_us     the frame above once per sequence: 3 S KalmanStore.round, S update, S initiate
  batch_us    KalmanStore.round_batch x 3 over the S sequences, ONE update and ONE initiate on the concatenated lists (detections_batch)
Both must return the same matches and initiations in the first frame and leave the same states, bit for bit, after the last (asserted).
  *_launches  as above; per_sequence_us = batch_us / S

Nothing here is a pass / fail criterion: the figures are reported as they come out, whichever route wins."""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(50, 60), (150, 150)]


def p50(v):
    return float(np.median(v) * 1e6)


def alternate(a, b, reps, sync):
    for _ in range(20):
        a(); sync(); b(); sync()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); a(); sync(); t1 = time.perf_counter(); b(); sync(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    return p50(ta), p50(tb), [[float(np.percentile(t, q) * 1e6) for q in (10, 90)] for t in (ta, tb)]


def launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if e.device_type.name != "CPU"))
    except Exception as err:                                                  # no device tracer in this build: say so in the JSON, the timings stand
        return "not counted: %s" % (err,)


class Track:
    """What the object route keeps per track: STrack's state and its tlbr property (byte_tracker.py:142-163)."""

    def __init__(self, mean, cov, state):
        self.mean, self.covariance, self.state = mean, cov, state

    @property
    def tlbr(self):
        ret = self.mean[:4].copy()
        ret[2] *= ret[3]
        ret[:2] -= ret[2:] / 2
        ret[2:] += ret[:2]
        return ret


def scene(k, n, m):
    """n track measurements on a grid, m detections (every second one on a track), scores: high for the first two thirds."""
    from busca_amd import synth
    cols = int(np.ceil(np.sqrt(n)))
    h = synth.uniform(800 + k, "h", (n,), 60, 110).astype(np.float64)
    z = np.stack([150.0 + 130.0 * (np.arange(n) % cols), 150.0 + 260.0 * (np.arange(n) // cols), synth.uniform(800 + k, "a", (n,), 0.3, 0.5), h], 1)
    owner = (np.arange(m) * 7) % n
    jit = synth.uniform(810 + k, "jit", (m, 4), -1, 1).astype(np.float64)
    d = z[owner].copy()
    d[:, 0] += 0.02 * d[:, 3] * jit[:, 0]
    d[:, 1] += 0.02 * d[:, 3] * jit[:, 1]
    d[:, 3] *= 1.0 + 0.02 * jit[:, 3]
    clutter = np.arange(m) % 2 == 1
    d[clutter, 0] += 5000.0                                                    # off every track
    scores = np.where(np.arange(m) < 2 * m // 3, 0.9, 0.3) - 0.05 * np.abs(jit[:, 2])
    dets = []
    for j in range(m):
        w = d[j, 2] * d[j, 3]
        tlwh = np.array([d[j, 0] - w / 2, d[j, 1] - d[j, 3] / 2, w, d[j, 3]])
        dets.append(types.SimpleNamespace(tlwh=tlwh, tlbr=np.array([tlwh[0], tlwh[1], tlwh[0] + tlwh[2], tlwh[1] + tlwh[3]]), score=float(scores[j])))
    return z, dets, scores


def sequence_frame(store, q):
    """The frame of one sequence through KalmanStore.round -> (the (slot, detection) pairs it updated, the detections it initiated).  `q`: the
    sequence's slots, spare_slots, dets / high / low, scores, n_pool, mh and not_tracked."""
    mt, ut, ud = store.round(q.slots[:q.n_pool], q.high, 0.8, det_scores=q.scores[:q.mh], not_tracked=q.not_tracked)
    pairs = [(q.slots[i], j) for i, j in mt]
    left = np.asarray([i for i in ut if not q.not_tracked[i]], dtype=np.int64)
    m2, _, _ = store.round(q.slots[left], q.low, 0.5, predict=False)
    pairs += [(q.slots[left[i]], q.mh + j) for i, j in m2]
    rest = [q.high[j] for j in ud]
    m3, _, ud3 = store.round(q.slots[q.n_pool:], rest, 0.7, det_scores=q.scores[:q.mh][list(ud)], predict=False)
    pairs += [(q.slots[q.n_pool + i], ud[j]) for i, j in m3]
    det_all = store.detections(q.dets, boxes=False)
    store.update([p[0] for p in pairs], det_all, [p[1] for p in pairs])
    new = [ud[j] for j in ud3]
    store.initiate(q.spare_slots[:len(new)], det_all, new)
    return pairs, new


def batch_frame(store, seqs):
    """The same frame of every sequence of a list at once: three round_batch, one update, one initiate -> [(pairs, initiations)] per sequence."""
    from busca_amd.tracking import RoundProblem
    r1 = store.round_batch([RoundProblem(q.slots[:q.n_pool], q.high, q.scores[:q.mh], q.not_tracked) for q in seqs], 0.8)
    pairs = [[(q.slots[i], j) for i, j in mt] for q, (mt, _, _) in zip(seqs, r1)]
    left = [np.asarray([i for i in ut if not q.not_tracked[i]], dtype=np.int64) for q, (_, ut, _) in zip(seqs, r1)]
    r2 = store.round_batch([RoundProblem(q.slots[lf], q.low) for q, lf in zip(seqs, left)], 0.5, predict=False)
    r3 = store.round_batch([RoundProblem(q.slots[q.n_pool:], [q.high[j] for j in ud], q.scores[:q.mh][list(ud)]) for q, (_, _, ud) in zip(seqs, r1)], 0.7,
                           predict=False)
    new = []
    for k, (q, lf) in enumerate(zip(seqs, left)):
        ud = r1[k][2]
        pairs[k] += [(q.slots[lf[i]], q.mh + j) for i, j in r2[k][0]]
        pairs[k] += [(q.slots[q.n_pool + i], ud[j]) for i, j in r3[k][0]]
        new.append([ud[j] for j in r3[k][2]])
    det_all, begin = store.detections_batch([q.dets for q in seqs], boxes=False)
    store.update([p[0] for ps in pairs for p in ps], det_all, [p[1] + begin[k] for k, ps in enumerate(pairs) for p in ps])
    store.initiate(np.concatenate([q.spare_slots[:len(nw)] for q, nw in zip(seqs, new)]), det_all, [j + begin[k] for k, nw in enumerate(new) for j in nw])
    return list(zip(pairs, new))


def main_sequences(counts, out_path, reps):
    """--sequences: S sequences in lock-step over one store, a loop of sequence_frame against batch_frame."""
    import torch
    from busca_amd import _lib, geometry, tracking
    assert torch.cuda.is_available(), "kalman_store_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(CASES):
        for S in counts:
            stores = [tracking.KalmanStore(S * (n + m)) for _ in range(2)]      # [0] the loop's, [1] the batch's: alike, so both routes see the same states
            seqs = []
            for s in range(S):
                z, dets, scores = scene(k + 2 * s, n, m)                        # (seeds 800 + k + 2 s: a scene of its own per sequence)
                n_pool, mh = 4 * n // 5, 2 * m // 3
                not_tracked = np.arange(n_pool) % 10 == 9
                mean0, cov0 = tracking.multi_initiate(z, ctx=ctx)
                slots = s * (n + m) + np.argsort(np.argsort((np.arange(n) * 7919) % 10007))
                for st in stores:
                    st.load(slots, [Track(mean0[i], cov0[i], 1) for i in range(n)])
                seqs.append(types.SimpleNamespace(slots=slots, spare_slots=s * (n + m) + n + np.arange(m), dets=dets, high=dets[:mh], low=dets[mh:], scores=scores,
                                                  n_pool=n_pool, mh=mh, not_tracked=not_tracked))

            def loop():
                return [sequence_frame(stores[0], q) for q in seqs]

            def batch():
                return batch_frame(stores[1], seqs)

            def plain(result):
                return [(sorted((int(a), int(b)) for a, b in pairs), sorted(int(j) for j in new)) for pairs, new in result]
            a, b = plain(loop()), plain(batch())
            assert a == b, "the two routes disagree at %d x %d, %d sequences" % (n, m, S)
            tl, tb, spread = alternate(loop, batch, reps, sync)
            assert torch.equal(stores[0].mean, stores[1].mean) and torch.equal(stores[0].cov, stores[1].cov), "states differ after %d frames" % (reps + 21)
            rows.append(dict(case="ByteTrack frame %dx%d" % (n, m), sequences=S, pairs_per_frame=sum(len(p) for p, _ in a), initiations_per_frame=sum(len(w) for _, w in a),
                             loop_us=tl, batch_us=tb, loop_p10_p90=spread[0], batch_p10_p90=spread[1], per_sequence_us=tb / S,
                             loop_launches=launches(loop), batch_launches=launches(batch)))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/kalman_store_bench.py --sequences", reps=reps, unit="us, p50 per frame of all sequences", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    import torch
    from busca_amd import _lib, geometry, kalman, tracking
    if "--sequences" in sys.argv:
        at = sys.argv.index("--sequences")
        counts = []
        while at + 1 + len(counts) < len(sys.argv) and sys.argv[at + 1 + len(counts)].isdigit():
            counts.append(int(sys.argv[at + 1 + len(counts)]))
        rest = sys.argv[1:at] + sys.argv[at + 1 + len(counts):]
        return main_sequences(counts or [1, 2, 4, 8, 16], rest[0] if rest else os.path.join(ROOT, "profiles", "kalman_store_batch_bench.json"),
                              int(rest[1]) if len(rest) > 1 else 200)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kalman_store_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "kalman_store_bench needs a GPU"
    ctx = geometry.default_context(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.current_stream(dev).synchronize
    rows = []
    for k, (n, m) in enumerate(CASES):
        z, dets, scores = scene(k, n, m)
        n_pool, mh = 4 * n // 5, 2 * m // 3
        high, low = dets[:mh], dets[mh:]
        not_tracked = np.arange(n_pool) % 10 == 9
        mean0, cov0 = tracking.multi_initiate(z, ctx=ctx)
        tracks = [Track(mean0[i].copy(), cov0[i].copy(), 1 if i >= n_pool or not not_tracked[i] else 2) for i in range(n)]
        spare = [Track(None, None, 1) for _ in range(m)]
        store = tracking.KalmanStore(n + m)
        slots = np.argsort(np.argsort((np.arange(n) * 7919) % 10007))          # a fixed permutation of 0 .. n-1: the tracks are not in slot order
        store.load(slots, tracks)
        spare_slots = n + np.arange(m)
        first = {}

        seq = types.SimpleNamespace(slots=slots, spare_slots=spare_slots, dets=dets, high=high, low=low, scores=scores, n_pool=n_pool, mh=mh, not_tracked=not_tracked)

        def store_frame():
            pairs, new = sequence_frame(store, seq)
            if "store" not in first:
                first["store"] = (sorted((int(np.nonzero(slots == s)[0][0]), int(j)) for s, j in pairs), sorted(int(j) for j in new))

        def object_frame():
            pool = tracks[:n_pool]
            mt, ut, ud = tracking.associate_round(pool, high, 0.8, det_scores=scores[:mh], ctx=ctx)
            pairs = [(i, j) for i, j in mt]
            left = [i for i in ut if pool[i].state == 1]
            m2, _, _ = tracking.linear_assignment(tracking.iou_distance([pool[i] for i in left], low, ctx=ctx), 0.5, ctx=ctx)
            pairs += [(left[i], mh + j) for i, j in m2]
            rest = [high[j] for j in ud]
            m3, _, ud3 = tracking.linear_assignment(tracking.iou_distance(tracks[n_pool:], rest, det_scores=scores[:mh][list(ud)], ctx=ctx), 0.7, ctx=ctx)
            pairs += [(n_pool + i, ud[j]) for i, j in m3]
            tracking.multi_update([tracks[i] for i, _ in pairs], [dets[j] for _, j in pairs], ctx=ctx)
            new = [ud[j] for j in ud3]
            nm, nc = tracking.multi_initiate([dets[j] for j in new], ctx=ctx)
            for q in range(len(new)):
                spare[q].mean, spare[q].covariance = nm[q], nc[q]
            if "object" not in first:
                first["object"] = (sorted((int(i), int(j)) for i, j in pairs), sorted(int(j) for j in new))

        store_frame(); sync(); object_frame(); sync()
        assert first["store"] == first["object"], "the two routes disagree at %d x %d" % (n, m)
        back = [types.SimpleNamespace(mean=None, covariance=None) for _ in range(n)]
        store.store(slots, back)
        assert all(np.array_equal(b.mean, t.mean) and np.array_equal(b.covariance, t.covariance) for b, t in zip(back, tracks)), "states differ after one frame"
        ts, to, frame_spread = alternate(store_frame, object_frame, reps, sync)

        # ---- the cost matrix of a fuse_motion round alone, everything on the device already
        det_dev = store.detections(high, scores[:mh])
        pool_slots = torch.from_numpy(slots[:n_pool].astype(np.int32)).to(dev)
        mean = store.mean[pool_slots.long()].contiguous()
        cov = store.cov[pool_slots.long()].contiguous()

        def cost_one():
            return store.cost(pool_slots, det_dev, fuse_motion=True)

        def cost_chain():
            boxes = torch.empty(n_pool, 4, dtype=torch.float64, device=dev)
            ctx.check(ctx.lib.busca_kalman_boxes(ctx.h, mean.data_ptr(), n_pool, 1, boxes.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            cost = geometry.pairwise(ctx, boxes, det_dev.tlbr, _lib.PAIR_IOU_COST)
            gate, status = kalman._gating_dev(ctx, mean, cov, det_dev.xyah, False, 0)
            return kalman._gate_dev(cost, gate, False, 0.98), status
        tc, tch, cost_spread = alternate(cost_one, cost_chain, reps, sync)
        rows.append(dict(case="ByteTrack frame %dx%d" % (n, m), pairs_per_frame=len(first["store"][0]), initiations_per_frame=len(first["store"][1]),
                         store_us=ts, object_us=to, store_p10_p90=frame_spread[0], object_p10_p90=frame_spread[1], store_launches=launches(store_frame), object_launches=launches(object_frame),
                         cost_us=tc, chain_us=tch, cost_p10_p90=cost_spread[0], chain_p10_p90=cost_spread[1], cost_launches=launches(cost_one), chain_launches=launches(cost_chain)))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/kalman_store_bench.py", reps=reps, unit="us, p50 per frame (cost_us / chain_us: per call)", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
