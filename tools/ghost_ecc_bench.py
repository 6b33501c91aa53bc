#!/usr/bin/env python3
"""Time GHOST's camera-motion estimate on the device (needs a GPU; bench.py is not involved).

    python tools/ghost_ecc_bench.py [out.json] [reps=100]

A synthetic moving sequence at 1080 x 1920 and 540 x 960: one smooth random float32 RGB scene (feature cells of 16 pixels) under a camera
that drifts by (1.3, -0.7) pixels and 0.5 mrad a frame, 12 frames resident in HBM, walked back and forth.  Settings: warp_mode Euclidean,
num_iter_mc 100, termination_eps_mc 1e-5, gaussFiltSize 15.  Host clock unless stated, microseconds.

  estimate_us        p50 of GhostCameraMotion.estimate per frame: one busca_ecc_prepare + busca_ecc_align_planes (the gradient pass and
                     `iterations` passes, each followed by a stream synchronisation and the host solve); the warp is on the host when it returns
  iterations         p50 / min / max of the iterations the loop ran
  prepare_us         busca_ecc_prepare alone (grey + rows, columns: two launches), mean of HIP events over `reps` calls
  iteration_us       one iteration of busca_ecc_align_planes, host clock: a 20-iteration call with the termination test off, minus a
                     1-iteration call, over 19 - kernel, reduction, 8-byte-per-sum download, synchronisation and the host solve
  download_us        p50 of the two `whole_image.cpu().numpy()` calls the reference makes per frame (float32 [3,H,W] each) - the part of the
                     host route that can be timed here
The CPU ECC itself (cv2.cvtColor x 2 + cv2.findTransformECC with a 15 x 15 Gaussian) is NOT timed: cv2 is not installed where this runs, and
the numpy restatement under tests/ is a checker, not OpenCV - its time says nothing about cv2's.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1080, 1920), (540, 960)]
CFG = {"warp_mode": "Euclidean", "num_iter_mc": 100, "termination_eps_mc": 1e-5}
FRAMES, CELL = 12, 16


def sequence(H, W, dev):
    """FRAMES frames [3,H,W] float32 in [0, 1] of one scene, frame i moved by i x (1.3, -0.7) pixels and i x 0.5 mrad."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(H)
    low = torch.rand(1, 3, H // CELL + 8, W // CELL + 8, generator=g).to(dev)
    big = F.interpolate(low, size=(H + 8 * CELL, W + 8 * CELL), mode="bicubic", align_corners=False).clamp_(0, 1)
    bh, bw = big.shape[2:]
    out = []
    for i in range(FRAMES):
        th, tx, ty = 0.0005 * i, 1.3 * i, -0.7 * i
        c, s = float(np.cos(th)), float(np.sin(th))
        # output pixel (x, y), centred, samples the scene at R (x, y) + t; in affine_grid's normalised coordinates of the big image
        theta = torch.tensor([[[c * W / bw, -s * H / bw, 2 * tx / bw], [s * W / bh, c * H / bh, 2 * ty / bh]]], dtype=torch.float32, device=dev)
        grid = F.affine_grid(theta, (1, 3, H, W), align_corners=False)
        out.append(F.grid_sample(big, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].contiguous())
    return out


def main():
    import torch
    from busca_amd import _lib, ecc, tracking
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ghost_ecc_bench.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    assert torch.cuda.is_available(), "ghost_ecc_bench needs a GPU"
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    rows = []
    for H, W in SIZES:
        frames = sequence(H, W, dev)
        walk = list(range(FRAMES)) + list(range(FRAMES - 2, 0, -1))
        cam = tracking.GhostCameraMotion(CFG, ctx=ctx)
        for k in range(len(walk) + 1):                                       # warm-up: one round of the walk
            cam.estimate(frames[walk[k % len(walk)]])
        t_est, its, norms = [], [], []
        for r in range(reps):
            f = frames[walk[(r + 1) % len(walk)]]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cam.estimate(f)
            t_est.append(time.perf_counter() - t0)
            its.append(cam.iterations)
            norms.append(float(cam.norm))
        plane = torch.empty(H, W, dtype=torch.float32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ecc._ecc_prepare(ctx, frames[0], 3, H, W, 15, plane)
        torch.cuda.synchronize()
        e0.record()
        for r in range(reps):
            ecc._ecc_prepare(ctx, frames[r % FRAMES], 3, H, W, 15, plane)
        e1.record()
        e1.synchronize()
        prepare_us = e0.elapsed_time(e1) * 1e3 / reps
        planes = [torch.empty(H, W, dtype=torch.float32, device=dev) for _ in range(2)]
        for p, f in zip(planes, frames[:2]):
            ecc._ecc_prepare(ctx, f, 3, H, W, 15, p)
        per_iter = []
        for r in range(max(reps // 5, 5)):
            t = []
            for n in (1, 20):
                warp = np.eye(2, 3, dtype=np.float32)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ecc._ecc_align_planes(ctx, planes[1], planes[0], _lib.ECC_EUCLIDEAN, n, -1.0, warp)
                t.append(time.perf_counter() - t0)
            per_iter.append((t[1] - t[0]) / 19)
        t_down = []
        for r in range(max(reps // 5, 5)):
            a, b = frames[r % FRAMES], frames[(r + 1) % FRAMES]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.cpu().numpy(); b.cpu().numpy()
            t_down.append(time.perf_counter() - t0)
        p50 = lambda v: float(np.median(v) * 1e6)
        rows.append(dict(case="%dx%d" % (H, W), estimate_us=p50(t_est), iterations_p50=float(np.median(its)), iterations_min=int(min(its)), iterations_max=int(max(its)),
                         prepare_us=prepare_us, iteration_us=p50(per_iter), download_us=p50(t_down), frame_mbytes=3 * H * W * 4 / 1e6,
                         warp_norm_p50=float(np.median(norms))))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/ghost_ecc_bench.py", settings=dict(CFG, gauss_size=15), frames=FRAMES, reps=reps,
               unit="us; host clock p50 (prepare_us: mean of HIP events)", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, host_threads=torch.get_num_threads(),
               build=_lib.build_info(ctx.lib),
               not_measured="the reference's CPU ECC (cv2.cvtColor x 2 + cv2.findTransformECC, 15 x 15 Gaussian): cv2 is not installed on the machine this ran on; "
                            "download_us is only the two frame downloads that precede it", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
