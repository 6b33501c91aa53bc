#!/usr/bin/env python3
"""Time the device appearance association against the host route it replaces (needs a GPU; bench.py is not involved).

    python tools/appearance_bench.py [out.json] [reps=200]

Synthetic ReID features (busca_amd.synth.appearance_features, E = 512, max_distance 0.45) at 50 tracks x 60 detections with one vector per track,
150 x 150 with one vector per track, and 150 x 150 with a full gallery of 100 samples per track (StrongSORT's nn_budget).  Both routes start from
features that are already in HBM - where busca_reid_forward* leaves them - and end with the matches on the host.  Every figure is the p50 in
microseconds of `reps` calls after 20 warm-up calls, host clock around a call that ends in a device->host copy (so it is synchronised); the two
routes of a row alternate inside one loop.

  device_us   tracking.appearance_cost on the device tensors, then tracking.min_cost_matching on the device matrix: two launches plus the torch clamp,
              one copy of n + m + 1 ints
  host_us     the route without the kernel: one device->host copy of the gallery and of the detections' features, the cosine cost in float64 numpy
              (BLAS matrix product, then the minimum over a track's samples), then tracking.min_cost_matching on the host matrix (upload, device solve)
  host_cost_us  the numpy cost alone, inside the same loop
  kernel_us   the cost kernel alone, mean of HIP events around `reps` launches (busca_timing_*)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_DISTANCE, E = 0.45, 512
SHAPES = [(50, 60, 1), (150, 150, 1), (150, 150, 100)]      # tracks, detections, samples per track


def host_cost(gallery, dets):
    """[n,budget,E], [m,E] float32 -> [n,m] float64 nearest-neighbour cosine distance."""
    n, budget, e = gallery.shape
    g, d = gallery.reshape(n * budget, e).astype(np.float64), dets.astype(np.float64)
    c = 1.0 - (g @ d.T) / (np.sqrt((g * g).sum(1))[:, None] * np.sqrt((d * d).sum(1))[None, :])
    return c.reshape(n, budget, -1).min(1)


def main():
    import torch
    from busca_amd import _lib, synth, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "appearance_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "appearance_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    lib, h = ctx.lib, ctx.h
    rows = []
    for k, (n, m, budget) in enumerate(SHAPES):
        trk, det = synth.appearance_features(400 + k, n, m, E, budget, twins=True)
        dg, dd = torch.from_numpy(trk).to(dev), torch.from_numpy(det).to(dev)
        tracks, dets = list(range(n)), list(range(m))
        t_host = []

        def device():
            return tracking.min_cost_matching(lambda *_: tracking.appearance_cost(dg, dd, "min", ctx=ctx), MAX_DISTANCE, tracks, dets, ctx=ctx)

        def host():
            g, d = dg.cpu().numpy(), dd.cpu().numpy()
            t0 = time.perf_counter()
            c = host_cost(g, d)
            t_host.append(time.perf_counter() - t0)
            return tracking.min_cost_matching(lambda *_: c, MAX_DISTANCE, tracks, dets, ctx=ctx)

        got, want = device(), host()
        assert got[0] == want[0] and len(got[0]) >= 5, "the two routes disagree at %d x %d x %d" % (n, m, budget)
        err = float(np.abs(tracking.appearance_cost(dg, dd, "min", ctx=ctx).cpu().numpy() - host_cost(trk, det)).max())
        for _ in range(20):
            device(); host()
        t_host.clear()
        ta, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); device(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        out = torch.empty(n, m, dtype=torch.float64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream

        def launch():
            ctx.check(lib.busca_appearance_cost(h, dg.data_ptr(), None, None, n, budget, dd.data_ptr(), m, E, _lib.APPEAR_MIN, 0, out.data_ptr(), s))
        for _ in range(20):
            launch()
        torch.cuda.synchronize(dev)
        lib.busca_timing_read(h, None, None, 1); lib.busca_timing_enable(h, 1)
        for _ in range(reps):
            launch()
        torch.cuda.synchronize(dev)
        avg, cnt = C.c_double(0), C.c_int64(0)
        lib.busca_timing_read(h, C.byref(avg), C.byref(cnt), 1); lib.busca_timing_enable(h, 0)
        assert cnt.value == reps
        rows.append(dict(case="%dx%d budget %d" % (n, m, budget), matched=len(got[0]), max_abs_diff=err, device_us=float(np.median(ta) * 1e6),
                         host_us=float(np.median(tb) * 1e6), host_cost_us=float(np.median(t_host) * 1e6), kernel_us=avg.value * 1e3))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/appearance_bench.py", E=E, max_distance=MAX_DISTANCE, reps=reps, unit="us, p50 (kernel_us: mean of HIP events)",
               device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), build=_lib.build_info(lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
