#!/usr/bin/env python3
"""Time the per-frame appearance bookkeeping with its state on the device against the host route it replaces (needs a GPU; bench.py is not involved).

    python tools/ghost_store_bench.py [out.json] [reps=200]

Synthetic ReID features (busca_amd.synth.normal, E = 512) already in HBM, as the extractor leaves them; 50 tracks x 60 detections and 150 x 150,
budget 32, every ring full, two thirds of the tracks active, every track matched to one detection per frame.  Every figure is the p50 in microseconds
of `reps` frames after 20 warm-up frames, host clock around a frame that ends in ghost_round's (or distance's) device->host copy, so it is
synchronised; the two routes of a row alternate inside one loop.  device_p10_us / device_p90_us (and host_*) are the 10th and 90th percentile of the
same frames: the spread a difference between two builds has to exceed.

GHOST, per proxy ('mv_avg' with num 0.9 / 0.5, 'mean' with num 3), one frame = the round of this frame, then the matched features join the galleries:
  device_us   GhostGallery.state -> ghost_round -> GhostGallery.add(slots, <the device features>, det_index): nothing but the slot tables goes up,
              nothing but the matches comes down
  host_us     what a user has today: the features downloaded, Track.past_feats as host lists (and the mv_avg dict in numpy), a [n,budget,E] gallery
              rebuilt from the lists and uploaded every frame, then ghost_round on it.  'mv_avg' has no device route without the table, so the host
              route computes the proxies in numpy and hands ghost_round one vector per track
  add_launches / release_launches   device kernels + copies one GhostGallery.add / release enqueues (torch.profiler, host slot tables: the pinned
                 upload of the tables is one of them)
  round_launches the same count for one ghost_round of the row's proxy, state() included: the proxy's launches and the rest of the round
StrongSORT EMA (opt.EMA_alpha 0.9), one frame = partial_fit of the matched features, then metric.distance against all detections:
  device_us   partial_fit(<device features>, ema_alpha=0.9)
  host_us     download of the features, the four lines of deep_sort/track.py:244-248 in numpy per track, partial_fit of the smoothed rows
              (budget 1: the newest row replaces the old one; partial_fit renormalises, which leaves a unit vector as it is up to rounding)
  fit_launches   device kernels + copies of one partial_fit(ema_alpha=) (the gather ddet[sel], the table upload and the count upload are among them)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, BUDGET = 512, 32
CASES = [(50, 60), (150, 150)]
PROXIES = [("mv_avg", 0.9, 0.5), ("mean", 3, 3)]


def p50(v):
    return float(np.median(v) * 1e6)


def spread(name, v):
    return {name + "_p10_us": float(np.percentile(v, 10) * 1e6), name + "_p90_us": float(np.percentile(v, 90) * 1e6)}


def alternate(a, b, reps):
    for _ in range(20):
        a(); b()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); a(); t1 = time.perf_counter(); b(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    return p50(ta), p50(tb), dict(spread("device", ta), **spread("host", tb))


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


def main():
    import torch
    from busca_amd import _lib, synth, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ghost_store_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "ghost_store_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    rows = []
    for k, (n, m) in enumerate(CASES):
        na = 2 * n // 3
        seedf = synth.normal(700 + k, "fill", (BUDGET, n, E))
        det = synth.normal(710 + k, "det", (m, E)) + np.float32(0.25)
        ddet = torch.from_numpy(det).to(dev)
        slots = np.arange(n)
        match = (np.arange(n) * 7) % m                                        # the detection row every track takes
        active, inactive = slots[:na], slots[na:]
        for proxy, a_act, a_inact in PROXIES:
            cfg = dict(avg_act={"do": True, "proxy": proxy, "num": a_act}, avg_inact={"do": True, "proxy": proxy, "num": a_inact})
            store = tracking.GhostGallery(n, BUDGET, E, ctx=ctx)
            past = [[] for _ in range(n)]
            for t in range(BUDGET):
                store.add(slots, seedf[t])
                for i in range(n):
                    past[i].append(seedf[t, i])
            mv = {}

            def device():
                _, row, col = tracking.ghost_round(store.state(active, inactive), ddet, cfg=cfg, ctx=ctx)
                store.add(slots, ddet, det_index=match)
                return row, col

            def host():
                d = ddet.cpu().numpy()
                if proxy == "mv_avg":
                    px = np.empty((n, E), dtype=np.float32)
                    for i in range(n):
                        a = a_act if i < na else a_inact
                        px[i] = mv[i] * np.float32(a) + past[i][-1] * np.float32(1 - a) if i in mv else past[i][-1]
                        mv[i] = px[i]
                    state = dict(gallery=px[:, None], count=None, newest=None, slot=None, num_active=na)
                    _, row, col = tracking.ghost_round(state, ddet, cfg={}, ctx=ctx)
                else:
                    gal = np.stack([np.stack(p[-BUDGET:]) for p in past])
                    state = dict(gallery=gal, count=None, newest=None, slot=None, num_active=na)      # rows oldest first: newest = count - 1
                    _, row, col = tracking.ghost_round(state, ddet, cfg=cfg, ctx=ctx)
                for i in range(n):
                    past[i].append(d[match[i]])
                    del past[i][:-BUDGET]
                return row, col

            got, want = device(), host()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(got[0]) == min(n, m), "the two routes disagree at %d x %d %s" % (n, m, proxy)
            td, th, sp = alternate(device, host, reps)
            rows.append(dict(case="GHOST %dx%d budget %d %s" % (n, m, BUDGET, proxy), device_us=td, host_us=th, **sp,
                             add_launches=launches(lambda: store.add(slots, ddet, det_index=match)),
                             round_launches=launches(lambda: tracking.ghost_round(store.state(active, inactive), ddet, cfg=cfg, ctx=ctx)),
                             release_launches=launches(lambda: store.release(inactive))))
            print(json.dumps(rows[-1]), flush=True)

        # ---- StrongSORT EMA ----------------------------------------------------------------------------------------------------------
        alpha, ids = 0.9, list(range(n))
        dmetric = tracking.NearestNeighborDistanceMetric("cosine", 0.4, budget=BUDGET, ctx=ctx)
        hmetric = tracking.NearestNeighborDistanceMetric("cosine", 0.4, budget=1, ctx=ctx)
        sel = torch.from_numpy(match).to(dev)
        smooth = {}

        def device_ema():
            dmetric.partial_fit(ddet[sel], ids, ids, ema_alpha=alpha)
            return dmetric.distance(ddet, ids)

        def host_ema():
            d = ddet.cpu().numpy()
            for i in ids:
                f = d[match[i]] / np.linalg.norm(d[match[i]])
                if i in smooth:
                    f = np.float32(alpha) * smooth[i] + np.float32(1 - alpha) * f
                    f /= np.linalg.norm(f)
                smooth[i] = f
            hmetric.partial_fit(np.stack([smooth[i] for i in ids]), ids, ids)
            return hmetric.distance(ddet, ids)

        got, want = device_ema(), host_ema()
        assert np.abs(got - want).max() < 1e-6, "the two EMA routes disagree at %d x %d" % (n, m)
        td, th, sp = alternate(device_ema, host_ema, reps)
        rows.append(dict(case="StrongSORT EMA %dx%d" % (n, m), device_us=td, host_us=th, **sp,
                         fit_launches=launches(lambda: dmetric.partial_fit(ddet[sel], ids, ids, ema_alpha=alpha))))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/ghost_store_bench.py", E=E, budget=BUDGET, reps=reps, unit="us, p50 per frame", device=torch.cuda.get_device_name(0),
               host_threads=torch.get_num_threads(), build=_lib.build_info(ctx.lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
