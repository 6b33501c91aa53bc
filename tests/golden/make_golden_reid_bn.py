#!/usr/bin/env python3
"""Record tests/golden/reid_bn.npz from THE REFERENCE's own ReID_Encoder on the CPU (build container only, as make_golden.py): running-statistics
BatchNorm - torch's train-mode update of `running_mean` / `running_var` and the eval-mode forward that reads them.  Run from the repo root:

    python tests/golden/make_golden_reid_bn.py

Weights are synth.reid_state_dict(3), crops smooth_crops(seed, n): the fixture holds seeds, statistics and outputs only.  Statistics are stored in the
order of busca_reid_load_running_stats: per conv in blob order running_mean[Cout], then running_var[Cout].

    R1    reset_running_stats(), momentum 1, one train-mode forward of 6 crops   -> r1_stats, r1_feats (that pass's `plain` features)
    eval  under R1: 1, 3 and 5 crops, `plain` and `norm`                          -> r1_eval_<plain|norm>_n<k>
    R2    from R1, momentum 0.1, one train-mode forward of 4 crops                -> r2_stats, r2_feats; r2_eval_plain_n3: 3 crops evaluated under R2
    *_f64_minus_f32  R1 and R2 once more with model.double(), stored as the float32 DIFFERENCE (float64 statistics - float32 statistics): how far
          float32 statistics are from the exact ones (the tests' statistics bar).  The difference is ~1e-7 of the value, so float32 holds it to
          ~1e-14 of the value, and the four statistics arrays stay below the size limit of a committed file.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

from busca_amd import weights  # noqa: E402

R1_CASE = (6, 61)                                   # (crops, seed) of the pass that sets R1
R2_CASE = (4, 62)                                   # ... that moves R1 to R2
EVAL_CASES = ((1, 71), (3, 73), (5, 75))            # evaluated under R1
R2_EVAL_CASE = (3, 73)                              # evaluated under R2
R2_MOMENTUM = 0.1


def to_input(crops, dtype):
    x = crops.astype(np.float32) / 255.0
    x -= np.array([0.406, 0.456, 0.485])
    x /= np.array([0.225, 0.224, 0.299])
    return torch.from_numpy(x).float()[..., [2, 1, 0]].permute(0, 3, 1, 2).to(dtype)


def bn_modules(model):
    mods = dict(model.named_modules())
    return [mods[bn] for _, bn in weights.reid_conv_names()]


def stats_of(model):
    parts = []
    for m in bn_modules(model):
        parts += [m.running_mean.detach().numpy().ravel(), m.running_var.detach().numpy().ravel()]
    return np.concatenate(parts)


def set_momentum(model, momentum):
    for m in bn_modules(model):
        m.momentum = momentum


def adapt(model, crops, momentum, dtype):
    """One train-mode forward (no gradients): torch updates the running statistics with the batch's."""
    set_momentum(model, momentum)
    model.train()
    with torch.no_grad():
        _, feats = model(to_input(crops, dtype), output_option="plain")
    return feats.numpy()


def evaluate(model, crops, option, dtype):
    model.eval()
    with torch.no_grad():
        _, feats = model(to_input(crops, dtype), output_option=option)
    return feats.numpy()


def record(enc, dtype, out, tag):
    model = enc.model
    for m in bn_modules(model):
        m.reset_running_stats()
    f1 = adapt(model, mg.smooth_crops(R1_CASE[1], R1_CASE[0]), 1.0, dtype)
    out["r1_stats" + tag] = stats_of(model)
    if not tag:
        out["r1_feats"] = f1
        for n, seed in EVAL_CASES:
            for option in ("plain", "norm"):
                out["r1_eval_%s_n%d" % (option, n)] = evaluate(model, mg.smooth_crops(seed, n), option, dtype)
    f2 = adapt(model, mg.smooth_crops(R2_CASE[1], R2_CASE[0]), R2_MOMENTUM, dtype)
    out["r2_stats" + tag] = stats_of(model)
    if not tag:
        out["r2_feats"] = f2
        out["r2_eval_plain_n%d" % R2_EVAL_CASE[0]] = evaluate(model, mg.smooth_crops(R2_EVAL_CASE[1], R2_EVAL_CASE[0]), "plain", dtype)


def main():
    torch.set_num_threads(mg.GOLDEN_THREADS)
    ref_network = mg.import_reference()[0]
    enc = ref_network.ReID_Encoder(num_classes=299, device=torch.device("cpu"), pretrained_path="no",
                                   use_domain_adaptation=False, trainable=False, use_checkpointing=False)
    mg.load_reid_weights(enc, 3)
    out = {}
    record(enc, torch.float32, out, "")
    enc.model.double()
    record(enc, torch.float64, out, "_f64")
    for r in ("r1", "r2"):
        exact = out.pop(r + "_stats_f64")
        assert exact.dtype == np.float64 and out[r + "_stats"].dtype == np.float32
        out[r + "_stats_f64_minus_f32"] = (exact - out[r + "_stats"].astype(np.float64)).astype(np.float32)
    np.savez_compressed(os.path.join(mg.OUT, "reid_bn.npz"), **out)
    print("wrote reid_bn.npz", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
