#!/usr/bin/env python3
"""Time GHOST's motion model on the device against the host route it replaces (needs a GPU; bench.py is not involved).

    python tools/ghost_motion_bench.py [out.json] [reps=200]

n tracks x m detections at 50 x 60 and 150 x 150, every track with a full history of H = 32 positions, two thirds of the tracks active,
last_n_frames = all.  One frame of a moving-camera sequence is: warp every stored position, step the motion model, build the [n,m] IoU motion
cost.  Every figure is the p50 in microseconds of `reps` frames after 20 warm-up frames, host clock, both routes ending with the cost matrix in HBM
and the stream synchronised; the two routes of a row alternate inside one loop.

  device_us   GhostMotion.compensate + GhostMotion.cost on resident state: busca_ghost_motion_warp, one upload of the n slot indices,
              busca_ghost_motion_step, busca_pairwise(IOU_COST) - three launches
  host_us     the reference's route restated in numpy on Python lists of the same length: every track's rows through the warp (one [H,3] x [3,2]
              product per corner and track instead of the reference's two torch.mm per row, which is kinder to the host), motion()'s per-track loop
              (np.asarray of the list, differences, np.repeat of the frame gaps, mean), pos += v, the IoU matrix of get_motion_dist in numpy, and
              the upload of [n,m] float64
  host_motion_us, host_warp_us, host_iou_us, host_upload_us   the parts of host_us, inside the same loop
  kernel_warp_us, kernel_step_us, kernel_iou_us               each kernel alone, mean of HIP events (busca_timing_*)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 32
CASES = [(50, 60), (150, 150)]
LAST_N = 100000000


def boxes_of(seed, n):
    from busca_amd import synth
    cx = synth.uniform(seed, "cx", (n,), 0, 1920).astype(np.float64)
    cy = synth.uniform(seed, "cy", (n,), 0, 1080).astype(np.float64)
    h = synth.uniform(seed, "h", (n,), 40, 300).astype(np.float64)
    w = h * synth.uniform(seed, "ar", (n,), 0.3, 0.5).astype(np.float64)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def host_warp(tracks, W):
    A = W.astype(np.float64)
    for t in tracks:
        P = np.asarray(t["last_pos"], dtype=np.float64)
        one = np.ones((len(P), 1))
        q = np.concatenate([np.concatenate([P[:, :2], one], 1) @ A.T, np.concatenate([P[:, 2:], one], 1) @ A.T], 1).astype(np.float32)
        t["last_pos"] = list(q)


def host_motion(tracks, na):
    for i, t in enumerate(tracks):
        if len(t["last_pos"]) > 1:
            if i < na:
                last_pos = np.asarray(t["last_pos"][-LAST_N:])
                frames = np.asarray(t["frames"][-LAST_N:])
                vs = (last_pos[1:, ] - last_pos[:-1, ]) / np.repeat(np.expand_dims((frames[1:] - frames[:-1]), 1), [4], axis=1)
                t["v"] = vs.mean(axis=0)
            t["pos"] = t["pos"] + t["v"]


def host_iou_cost(pos, dets):
    """1 - IoU with the "+1" pixel convention, tracks x detections."""
    a, b = pos[:, None, :], dets[None, :, :]
    iw = np.clip(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + 1, 0, None)
    ih = np.clip(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + 1, 0, None)
    area = lambda x: (x[..., 2] - x[..., 0] + 1) * (x[..., 3] - x[..., 1] + 1)
    return 1 - iw * ih / (area(a) + area(b) - iw * ih)


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
    from busca_amd import _lib, synth, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ghost_motion_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "ghost_motion_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    lib, h = ctx.lib, ctx.h
    rows = []
    for k, (n, m) in enumerate(CASES):
        base, drift = boxes_of(700 + k, n), synth.uniform(700 + k, "drift", (n, 4), -3, 3).astype(np.float64)
        dets = np.concatenate([base + (H + 1) * drift, boxes_of(800 + k, m)])[:m]
        d_dev = torch.from_numpy(dets).to(dev)
        na, slots = 2 * n // 3, np.arange(n)
        gm = tracking.GhostMotion(n, H, ctx=ctx)
        tracks = [dict(last_pos=[], frames=[], pos=None, v=np.zeros(4)) for _ in range(n)]
        for t in range(H):
            b = base + t * drift
            gm.add(slots, b, 1 + 2 * t, new=np.full(n, t == 0))
            for i, tr in enumerate(tracks):
                tr["last_pos"].append(b[i].copy()); tr["frames"].append(1 + 2 * t); tr["pos"] = b[i].copy()
        warps = [np.array([[1, 0, s * 0.5], [0, 1, -s * 0.25]], dtype=np.float32) for s in (1, -1)]
        parts = {"warp": [], "motion": [], "iou": [], "upload": []}

        def device(W):
            gm.compensate(W)
            c = gm.cost(slots, na, d_dev, LAST_N)
            torch.cuda.synchronize()
            return c

        def host(W):
            t0 = time.perf_counter()
            host_warp(tracks, W)
            t1 = time.perf_counter()
            host_motion(tracks, na)
            t2 = time.perf_counter()
            c = host_iou_cost(np.array([t["pos"] for t in tracks]), dets)
            t3 = time.perf_counter()
            c = torch.from_numpy(c).to(dev)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            for key, v in zip(("warp", "motion", "iou", "upload"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[key].append(v)
            return c

        got, want = device(warps[0]).cpu().numpy(), host(warps[0]).cpu().numpy()
        assert np.abs(got - want).max() < 1e-6 and got.min() < 0.5, "the two routes disagree at %d x %d: %g" % (n, m, np.abs(got - want).max())
        for r in range(20):
            device(warps[(r + 1) % 2]); host(warps[(r + 1) % 2])
        for v in parts.values():
            v.clear()
        ta, tb = [], []
        for r in range(reps):
            W = warps[(r + 1) % 2]
            t0 = time.perf_counter(); device(W); t1 = time.perf_counter(); host(W); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        s = torch.cuda.current_stream(dev).cuda_stream
        slot_dev = torch.arange(n, dtype=torch.int32, device=dev)
        out, cost = torch.empty(n, 4, dtype=torch.float64, device=dev), torch.empty(n, m, dtype=torch.float64, device=dev)
        st = [t.data_ptr() for t in (gm.hist, gm.frames, gm.count, gm.newest, gm.pos, gm.vel)]
        W = np.ascontiguousarray(warps[0].reshape(6))
        kw = kernel_time(ctx, lambda: ctx.check(lib.busca_ghost_motion_warp(h, st[0], st[2], st[3], n, H, None, 0, W.ctypes.data, s)), reps)
        ks = kernel_time(ctx, lambda: ctx.check(lib.busca_ghost_motion_step(h, *st, n, H, slot_dev.data_ptr(), n, na, LAST_N, 1, out.data_ptr(), s)), reps)
        ki = kernel_time(ctx, lambda: ctx.check(lib.busca_pairwise(h, out.data_ptr(), n, d_dev.data_ptr(), m, _lib.PAIR_IOU_COST, None, cost.data_ptr(), s)), reps)
        p50 = lambda v: float(np.median(v) * 1e6)
        rows.append(dict(case="%dx%d H %d" % (n, m, H), device_us=p50(ta), host_us=p50(tb), host_warp_us=p50(parts["warp"]), host_motion_us=p50(parts["motion"]),
                         host_iou_us=p50(parts["iou"]), host_upload_us=p50(parts["upload"]), kernel_warp_us=kw, kernel_step_us=ks, kernel_iou_us=ki))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/ghost_motion_bench.py", H=H, last_n_frames=LAST_N, reps=reps, unit="us, p50 (kernel_*: mean of HIP events)",
               device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), build=_lib.build_info(lib), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
