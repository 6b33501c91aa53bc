"""Oracle (CPU checker, test infrastructure only): the ReID crop feature extractor of
/root/reference/busca/reid/resnet.py (ResNet-50 Bottleneck [3,4,6,3], pool='max', red=4) as driven by
/root/reference/busca/network.py:510-575 - i.e. with every BatchNorm in TRAIN mode (batch statistics)
at inference (network.py:553-556).  Plain torch CPU functional ops, float32, no reference modules.
`running=` evaluates the same network in EVAL mode instead (every BatchNorm on the given running statistics), as the standalone ReID_Encoder does.
"""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)


def _bn(x, sd, name, bn=None):
    """nn.BatchNorm2d defaults, eps 1e-5 (resnet.py:153-154).  `bn` None or without "running": training=True -> biased batch variance; with
    bn["running"]: training=False on those statistics.  bn["batch_stats"] (a dict, train mode) receives name -> (mean, biased variance, samples per
    channel) of this BatchNorm's input."""
    running = bn.get("running") if bn else None
    if running is not None:
        mean, var = running[name] if name in running else (running[name + ".running_mean"], running[name + ".running_var"])
        mean, var = (torch.as_tensor(np.asarray(v), dtype=x.dtype) for v in (mean, var))
        return F.batch_norm(x, mean, var, sd[name + ".weight"], sd[name + ".bias"], False, 0.1, 1e-5)
    if bn and bn.get("batch_stats") is not None:
        bn["batch_stats"][name] = (x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False), x.numel() // x.shape[1])
    return F.batch_norm(x, None, None, sd[name + ".weight"], sd[name + ".bias"], True, 0.1, 1e-5)


def _bottleneck(x, sd, p, stride, has_ds, bn=None):
    """resnet.py:108-128."""
    out = F.relu(_bn(F.conv2d(x, sd[p + "conv1.weight"]), sd, p + "bn1", bn))
    out = F.relu(_bn(F.conv2d(out, sd[p + "conv2.weight"], stride=stride, padding=1), sd, p + "bn2", bn))
    out = _bn(F.conv2d(out, sd[p + "conv3.weight"]), sd, p + "bn3", bn)
    if has_ds:
        x = _bn(F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride), sd, p + "downsample.1", bn)
    return F.relu(out + x)


@torch.no_grad()
def reid_forward(sd, x, return_stages=False, dtype=torch.float32, running=None, batch_stats=None):
    """x: [n,3,384,128] float32 (RGB, CHW, normalised as network.py:470-478,397) -> [n,512] L2-normalised
    features (resnet.py:266-322 with output_option='plain').  One call == one BN batch.
    dtype=torch.float64 evaluates the same network in double precision (used once, in the build container, to tell the float32
    round-off of the reference's own CPU kernels from a defect: tests/golden/make_golden.py reid_cfg4_f64).
    running (None: train mode, the default): a state dict with `<bn>.running_mean` / `<bn>.running_var`, or {<bn>: (mean, var)} - EVAL mode,
    F.batch_norm(training=False) on them, otherwise the same network.  batch_stats (a dict, train mode): filled with <bn> -> (mean, biased variance,
    samples per channel) of every BatchNorm's input, what torch's train-mode update of the running statistics starts from.
    With return_stages, stages["fc7"] is the 512-d output before F.normalize (output_option 'norm')."""
    bn = {"running": running, "batch_stats": batch_stats}
    sd = {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)
    stages = {}
    x = F.relu(_bn(F.conv2d(x, sd["conv1.weight"], stride=2, padding=3), sd, "bn1", bn))
    x = F.max_pool2d(x, 3, 2, 1)
    stages["stem"] = x
    for li, nblk in enumerate(LAYERS):
        for b in range(nblk):
            stride = 2 if (li > 0 and b == 0) else 1
            x = _bottleneck(x, sd, "layer%d.%d." % (li + 1, b), stride, b == 0, bn)
        stages["layer%d" % (li + 1)] = x
    fc7 = torch.flatten(F.adaptive_max_pool2d(x, 1), 1)
    stages["pool"] = fc7
    fc7 = F.linear(fc7, sd["red.weight"], sd["red.bias"])
    stages["fc7"] = fc7
    feats = F.normalize(fc7, p=2, dim=1)
    return (feats, stages) if return_stages else feats


def crops_to_reid_input(crops_u8_bgr):
    """u8 [n,384,128,3] BGR -> float32 [n,3,384,128] RGB normalised (network.py:470-478, 397).
    The reference builds this tensor as `batch[..., [2, 1, 0]].permute(0, 1, 4, 2, 3)` and `.view(-1, C, H, W)`
    (network.py:397,188): an NHWC buffer seen as NCHW, i.e. torch's channels_last memory format, which the conv /
    batch-norm kernels then keep for the whole ResNet.  The same strides are produced here; with them the oracle's
    features are BIT-IDENTICAL to the reference's on the same host (a contiguous NCHW input differs by ~1e-5)."""
    from .geometry import normalize_bgr
    x = torch.from_numpy(normalize_bgr(np.asarray(crops_u8_bgr))).float()
    return x[..., [2, 1, 0]].permute(0, 3, 1, 2)
