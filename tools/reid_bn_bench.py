#!/usr/bin/env python3
"""Time the ReID extractor's running-statistics pass against its batch-statistics pass (needs a GPU; bench.py is not involved).

    python tools/reid_bn_bench.py [out.json] [reps=40] [--baseline a.json b.json ...]
    python tools/reid_bn_bench.py --batch-only out.json [reps=40]
    python tools/reid_bn_bench.py --pass PREC N [running|batch]

Default: for each arithmetic flavour (f32, x3, f16) and 40, 88 and 512 smooth synthetic crops (weights synth.reid_state_dict(3), running statistics
set by one adapt(momentum 1) of 16 crops so that they match the weights), the p50 in microseconds of `reps` calls after 5 warm-up calls of each kind,
host clock around a call followed by a synchronise of its stream; the two kinds of a row alternate inside one loop.

  running_us   ReIDEncoderHIP.forward_running (busca_reid_forward_running)
  batch_us     ReIDEncoderHIP.forward (busca_reid_forward_w), same build, same loop
  parent_batch_us   with --baseline: the median over the given files of `batch_us` at the same flavour and n.  Each file is what `--batch-only` wrote on
                    ANOTHER checkout (that mode uses nothing but `forward`, so it runs on a commit without the running-statistics entry points).

`--pass` runs ONE pass of the given kind after loading (running statistics: R1 of tests/golden/reid_bn.npz) and nothing else: the command to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR -o t --`
(tools/kstats.py DIR then lists the kernels of the pass).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAVOURS = ("f32", "x3", "f16")
SIZES = (40, 88, 512)
WARMUP = 5


def smooth_crops(seed, n):
    from busca_amd import synth
    base = synth.randint_u8(seed, "crops", (n, 24, 8, 3)).astype(np.float32)
    up = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    noise = synth.randint_u8(seed, "noise", (n, 384, 128, 3)).astype(np.float32) - 128
    return np.clip(up + 0.25 * noise, 0, 255).astype(np.uint8)


def timed(fn, dev):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.current_stream(dev).synchronize()
    return time.perf_counter() - t0


def extractor(prec, with_stats):
    import torch
    from busca_amd import _lib, synth
    from busca_amd.reid import ReIDEncoderHIP
    ctx = _lib.Context(0)
    m = ReIDEncoderHIP(ctx, synth.reid_state_dict(3), precision=prec)
    if with_stats:
        m.reset_running_stats()
        m.adapt(smooth_crops(900, 16), 1.0)
        torch.cuda.synchronize()
        assert not m.take_status()
    return ctx, m


def one_pass(prec, n, kind):
    """Nothing on the device but the load and ONE pass: the running statistics come from the committed fixture (recorded for these weights), not from a pass."""
    import torch
    ctx, m = extractor(prec, False)
    if kind == "running":
        with np.load(os.path.join(ROOT, "tests", "golden", "reid_bn.npz")) as g:
            m.load_running_stats(g["r1_stats"])
    c = torch.from_numpy(smooth_crops(1000 + n, n)).cuda()
    torch.cuda.synchronize()
    f = m.forward_running(c) if kind == "running" else m.forward(c)
    torch.cuda.synchronize()
    print("%s %s pass of %d crops: reid_status %s" % (prec, kind, n, m.take_status()))
    del f
    ctx.close()


def main():
    import torch
    from busca_amd import _lib
    args = sys.argv[1:]
    if args and args[0] == "--pass":
        return one_pass(args[1], int(args[2]), args[3] if len(args) > 3 else "running")
    batch_only = bool(args) and args[0] == "--batch-only"
    if batch_only:
        args = args[1:]
    baselines = []
    if "--baseline" in args:
        k = args.index("--baseline")
        baselines, args = args[k + 1:], args[:k]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "reid_bn_bench.json")
    reps = int(args[1]) if len(args) > 1 else 40
    assert torch.cuda.is_available(), "reid_bn_bench needs a GPU"
    dev = torch.device("cuda", 0)
    base = [json.load(open(p))["rows"] for p in baselines]
    rows = []
    for prec in FLAVOURS:
        ctx, m = extractor(prec, not batch_only)
        for n in SIZES:
            c = torch.from_numpy(smooth_crops(1000 + n, n)).to(dev)
            m.reserve(n)
            kinds = [("batch_us", lambda: m.forward(c))] + ([] if batch_only else [("running_us", lambda: m.forward_running(c))])
            for _ in range(WARMUP):
                for _, fn in kinds:
                    timed(fn, dev)
            t = {k: [] for k, _ in kinds}
            for _ in range(reps):
                for k, fn in kinds:
                    t[k].append(timed(fn, dev))
            assert not m.take_status()
            row = dict(precision=prec, n=n)
            for k, _ in kinds:
                row[k] = float(np.median(t[k]) * 1e6)
                row[k.replace("_us", "_p10_p90_us")] = [float(np.percentile(t[k], 10) * 1e6), float(np.percentile(t[k], 90) * 1e6)]
            if base:
                vals = [r["batch_us"] for rs in base for r in rs if r["precision"] == prec and r["n"] == n]
                row["parent_batch_us"] = float(np.median(vals))
                row["parent_batch_runs_us"] = vals
            rows.append(row)
            print(json.dumps(row), flush=True)
        ctx.close()
    res = dict(tool="tools/reid_bn_bench.py" + (" --batch-only" if batch_only else ""), reps=reps, warmup=WARMUP, unit="us per pass, p50 (host clock, synchronised)",
               device=torch.cuda.get_device_name(0), build=_lib.build_info(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
