#!/usr/bin/env python3
"""Time the device linear assignment against the host route it replaces (needs a GPU; bench.py is not involved).

    python tools/assign_bench.py [out.json] [reps=300]

Tracker-like cost matrices (busca_amd.synth.tracker_costs, limit 0.8) at 50 x 60, 100 x 150 and 250 x 300, and a batch of 16 at 100 x 150.
Every figure is the p50 in microseconds of `reps` calls after 20 warm-up calls, host clock around a call that ends in a device->host copy
(so it is synchronised); the two routes of a row alternate inside one loop.

  device_us        tracking.linear_assignment on a device-resident cost matrix: the launch plus the copy of n + m + 1 ints
  host_us          the route without the solver: one device->host copy of the [n,m] matrix, then scipy.optimize.linear_sum_assignment on the
                   clamped rectangular restatement (entries >= limit at the limit, clamped pairs dropped) - the cheaper of the two restatements
  round_device_us  tracking.associate_round (prediction, boxes, IoU cost, assignment; one copy back)
  round_host_us    tracking.predicted_cost (the same chain, the matrix copied back) plus the host solve
  kernel_us        the solver kernel alone, mean of HIP events around `reps` launches (busca_timing_*)
  batch rows       linear_assignment_batch of 16 device matrices against 16 times the host route; kernel_us is the one launch of 16 workgroups
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

LIMIT = 0.8
SIZES = [(50, 60), (100, 150), (250, 300)]
BATCH = (16, 100, 150)


def host_solve(c, t):
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(np.where(c < t, c, t))
    keep = c[rows, cols] < t
    x = np.full(c.shape[0], -1, dtype=np.int64)
    x[rows[keep]] = cols[keep]
    y = np.full(c.shape[1], -1, dtype=np.int64)
    y[cols[keep]] = rows[keep]
    return np.stack([rows[keep], cols[keep]], 1), np.where(x < 0)[0], np.where(y < 0)[0]


def p50_pair(fa, fb, reps, warm=20):
    """p50 in us of two routes, alternated call by call."""
    for _ in range(warm):
        fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); t1 = time.perf_counter(); fb(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    return float(np.median(ta) * 1e6), float(np.median(tb) * 1e6)


def scene(seed, n, m):
    """Tracks (initiated Kalman states of the scene's boxes) and detection objects of synth.tracker_boxes."""
    from busca_amd import synth, tracking
    trk, det = synth.tracker_boxes(seed, n, m)

    def tlwh(b):
        return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
    mean, cov = tracking.multi_initiate(tracking.tlwh_to_xyah(tlwh(trk)))
    dets = [types.SimpleNamespace(tlwh=w, tlbr=b) for w, b in zip(tlwh(det), det)]
    return mean, cov, dets


def main():
    import torch
    from busca_amd import _lib, synth, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "assign_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    assert torch.cuda.is_available(), "assign_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    lib, h = ctx.lib, ctx.h

    def kernel_us(cost, batch, n, m, dims=None):
        out = torch.empty(batch, n + m, dtype=torch.int32, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream

        def launch():
            ctx.check(lib.busca_linear_assignment(h, cost.data_ptr(), batch, n, m, None if dims is None else dims.data_ptr(), LIMIT, out.data_ptr(), None,
                                                  None, None, st.data_ptr(), s))
        for _ in range(20):
            launch()
        torch.cuda.synchronize(dev)
        lib.busca_timing_read(h, None, None, 1); lib.busca_timing_enable(h, 1)
        for _ in range(reps):
            launch()
        torch.cuda.synchronize(dev)
        avg, cnt = C.c_double(0), C.c_int64(0)
        lib.busca_timing_read(h, C.byref(avg), C.byref(cnt), 1); lib.busca_timing_enable(h, 0)
        assert cnt.value == reps and int(st.cpu().max()) == 0
        return avg.value * 1e3

    rows = []
    for k, (n, m) in enumerate(SIZES):
        c = synth.tracker_costs(100 + k, n, m)
        dc = torch.from_numpy(c).to(dev)
        got, want = tracking.linear_assignment(dc, LIMIT, ctx=ctx), host_solve(c, LIMIT)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the two routes disagree at %d x %d" % (n, m)
        d_us, h_us = p50_pair(lambda: tracking.linear_assignment(dc, LIMIT, ctx=ctx), lambda: host_solve(dc.cpu().numpy(), LIMIT), reps)
        mean, cov, dets = scene(100 + k, n, m)

        def tracks():
            return [types.SimpleNamespace(mean=mean[i], covariance=cov[i], state=1) for i in range(n)]
        rd_us, rh_us = p50_pair(lambda: tracking.associate_round(tracks(), dets, LIMIT, ctx=ctx),
                                lambda: host_solve(tracking.predicted_cost(tracks(), dets, ctx=ctx), LIMIT), reps)
        rows.append(dict(case="%dx%d" % (n, m), batch=1, matched=int(len(want[0])), staged=None, device_us=d_us, host_us=h_us, round_device_us=rd_us,
                         round_host_us=rh_us, kernel_us=kernel_us(dc, 1, n, m)))
        rows[-1]["staged"] = ctx.get_option("last_assign_staged")
        print(json.dumps(rows[-1]), flush=True)
    b, n, m = BATCH
    mats = [torch.from_numpy(synth.tracker_costs(200 + k, n, m)).to(dev) for k in range(b)]
    got = tracking.linear_assignment_batch(mats, LIMIT, ctx=ctx)
    for k in range(b):
        assert all(np.array_equal(x, y) for x, y in zip(got[k], host_solve(mats[k].cpu().numpy(), LIMIT)))
    d_us, h_us = p50_pair(lambda: tracking.linear_assignment_batch(mats, LIMIT, ctx=ctx), lambda: [host_solve(a.cpu().numpy(), LIMIT) for a in mats], reps)
    slab = torch.stack(mats)
    rows.append(dict(case="16 x %dx%d" % (n, m), batch=b, matched=int(sum(len(g[0]) for g in got)), staged=None, device_us=d_us, host_us=h_us,
                     round_device_us=None, round_host_us=None, kernel_us=kernel_us(slab, b, n, m)))
    rows[-1]["staged"] = ctx.get_option("last_assign_staged")
    print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/assign_bench.py", limit=LIMIT, reps=reps, unit="us, p50 (kernel_us: mean of HIP events)", device=torch.cuda.get_device_name(0),
               build=_lib.build_info(lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
