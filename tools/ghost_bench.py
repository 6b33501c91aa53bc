#!/usr/bin/env python3
"""Time GHOST's association round on the device against the host route it replaces (needs a GPU; bench.py is not involved).

    python tools/ghost_bench.py [out.json] [reps=200]

Synthetic ReID features (busca_amd.synth.appearance_features, E = 512, twins) at 50 tracks x 60 detections with one sample per track, and at
150 x 150 with a gallery of 100 samples per track reduced by MEDIAN and by MIDRANGE - the two reductions of proxy_dist that busca_appearance_cost
does not have.  The round is the each_sample route with fixed thresholds 0.9 / 0.8 and nan_first, two thirds of the tracks active, one solve.
Both routes start from features that are already in HBM and end with the matches on the host.  Every figure is the p50 in microseconds of `reps`
calls after 20 warm-up calls, host clock around a call that ends in a device->host copy (so it is synchronised); the two routes of a row alternate
inside one loop.

  device_us     tracking.ghost_round: busca_ghost_distance (one launch: both groups of tracks run the same reduction), busca_ghost_combine, busca_linear_assignment,
                one copy of n + m + 1 ints
  host_us       the route without the kernels: one device->host copy of the gallery and of the detections' features, the cosine distances in float64
                numpy (BLAS matrix product), np.median / (max + min) / 2 over a track's samples, the thresholds, then tracking.linear_assignment on
                the host matrix (upload, device solve)
  host_cost_us  the numpy cost alone, inside the same loop
  kernel_us               busca_ghost_distance with the row's reduction alone, all tracks in one launch, mean of HIP events (busca_timing_*)
  kernel_ghost_min_us     the same kernel with MIN: the distance phase without a selection (kernel_us - this = what MEDIAN's selection costs)
  kernel_appear_min_us    busca_appearance_cost MIN at the same shape
"""
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, THR = 512, (0.9, 0.8)
CASES = [(50, 60, 1, "mean"), (150, 150, 100, "median"), (150, 150, 100, "midrange")]      # tracks, detections, samples per track, reduction
NUM = {"mean": 2, "midrange": 4, "median": 5}


def host_cost(gallery, dets, reduce, na):
    """[n,budget,E], [m,E] float32 -> [n,m] float64 thresholded proxy distances."""
    n, budget, e = gallery.shape
    g, d = gallery.reshape(n * budget, e).astype(np.float64), dets.astype(np.float64)
    c = (1.0 - (g @ d.T) / (np.sqrt((g * g).sum(1))[:, None] * np.sqrt((d * d).sum(1))[None, :])).reshape(n, budget, -1)
    c = np.median(c, 1) if reduce == "median" else (c.max(1) + c.min(1)) / 2 if reduce == "midrange" else c.mean(1)
    c[:na] = np.where(c[:na] <= THR[0], c[:na], np.nan)
    c[na:] = np.where(c[na:] <= THR[1], c[na:], np.nan)
    return c


def kernel_time(ctx, launch, reps):
    import torch
    lib, h = ctx.lib, ctx.h
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    lib.busca_timing_read(h, None, None, 1); lib.busca_timing_enable(h, 1)
    for _ in range(reps):
        launch()
    torch.cuda.synchronize()
    avg, cnt = C.c_double(0), C.c_int64(0)
    lib.busca_timing_read(h, C.byref(avg), C.byref(cnt), 1); lib.busca_timing_enable(h, 0)
    assert cnt.value == reps
    return avg.value * 1e3


def main():
    import torch
    from busca_amd import _lib, ghost, synth, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ghost_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "ghost_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    lib, h = ctx.lib, ctx.h
    rows = []
    for k, (n, m, budget, reduce) in enumerate(CASES):
        trk, det = synth.appearance_features(500 + k, n, m, E, budget, twins=True)
        dg, dd = torch.from_numpy(trk).to(dev), torch.from_numpy(det).to(dev)
        na = 2 * n // 3
        state = types.SimpleNamespace(gallery=dg, count=None, newest=None, slot=torch.arange(n, dtype=torch.int32, device=dev), num_active=na)
        entry = {"do": True, "num": NUM[reduce], "proxy": "each_sample"}
        cfg = dict(avg_act=entry, avg_inact=entry, act_reid_thresh=THR[0], inact_reid_thresh=THR[1], nan_first=True, distance="cosine", use_bism=False)
        t_host = []

        def device():
            _, row, col = tracking.ghost_round(state, dd, cfg=cfg, ctx=ctx)
            return row, col

        def host():
            g, d = dg.cpu().numpy(), dd.cpu().numpy()
            t0 = time.perf_counter()
            c = host_cost(g, d, reduce, na)
            t_host.append(time.perf_counter() - t0)
            pairs, _, _ = tracking.linear_assignment(c, tracking.GHOST_LIMIT, ctx=ctx)
            order = np.argsort(pairs[:, 1], kind="stable")
            return pairs[order, 1], pairs[order, 0]

        got, want = device(), host()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(got[0]) >= 5, "the two routes disagree at %d x %d x %d" % (n, m, budget)
        for _ in range(20):
            device(); host()
        t_host.clear()
        ta, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); device(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        out = torch.empty(n, m, dtype=torch.float64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        code = ghost._GHOST_REDUCE[reduce]
        kt = kernel_time(ctx, lambda: ctx.check(lib.busca_ghost_distance(h, dg.data_ptr(), None, None, n, budget, dd.data_ptr(), m, E, code, out.data_ptr(), s)), reps)
        kmin = kernel_time(ctx, lambda: ctx.check(lib.busca_ghost_distance(h, dg.data_ptr(), None, None, n, budget, dd.data_ptr(), m, E, _lib.GHOST_MIN, out.data_ptr(), s)), reps)
        kapp = kernel_time(ctx, lambda: ctx.check(lib.busca_appearance_cost(h, dg.data_ptr(), None, None, n, budget, dd.data_ptr(), m, E, _lib.APPEAR_MIN, 0, out.data_ptr(), s)), reps)
        rows.append(dict(case="%dx%d budget %d %s" % (n, m, budget, reduce), matched=int(len(got[0])), device_us=float(np.median(ta) * 1e6),
                         host_us=float(np.median(tb) * 1e6), host_cost_us=float(np.median(t_host) * 1e6), kernel_us=kt, kernel_ghost_min_us=kmin,
                         kernel_appear_min_us=kapp))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/ghost_bench.py", E=E, thresholds=THR, reps=reps, unit="us, p50 (kernel_*: mean of HIP events)",
               device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), build=_lib.build_info(lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
