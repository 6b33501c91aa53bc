"""Host handle of the ReID feature extractor kernels (busca_reid_* in include/busca_hip.h and include/busca_reid_bn.h)."""
import weakref

import numpy as np
import torch

from . import geometry, weights


PRECISIONS = {"f32": 0, "f16": 1, "x3": 2}          # BUSCA_PREC_F32 / _F16 / _F16X3 (include/busca_hip.h)
OUTPUTS = {"plain": 0, "norm": 1, "neck": 1}        # BUSCA_REID_OUT_* (include/busca_reid_bn.h); the encoder has no neck: `neck` returns fc7 like `norm` (resnet.py:329-334)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class ReIDEncoderHIP:
    """ResNet-50 (max pool, red=4), fp16 MFMA convs.
    `forward(crops_u8)`: u8 [n,384,128,3] BGR -> f32 [n,512] L2-normalised, batch-statistics BatchNorm: one call == one BN batch.
    `forward_running` / `adapt`: torch's eval-mode forward on running statistics and its train-mode update of them (include/busca_reid_bn.h)."""
    PRETRAINED_SIZE = (384, 128)

    def __init__(self, ctx, state_dict, prefix="", precision="f16"):
        """precision "f16": fp16 activations/weights (fastest, features ~6e-3 from the reference); "f32": exact float32 convs on the
        f32 MFMA (reference-exact ~1e-5, ~6x slower); "x3": float32 activations with split-fp16 products, three fp16 MFMAs per block
        (BUSCA_PREC_F16X3: the same ~1e-5 at a third of the fp16 matrix rate)."""
        if precision not in PRECISIONS:
            raise ValueError("ReID precision %r (one of %s)" % (precision, sorted(PRECISIONS)))
        self.ctx = ctx
        self.precision = precision
        self._blob = weights.reid_blob(state_dict, prefix)
        self._running = None                # host copy of the running statistics the context should hold (None: none loaded); stale while `_running_dirty`
        self._running_dirty = False         # an adapt() moved the device's statistics since `_running` was read
        if precision == "x3":
            # a HINT only (a loose static bound: 48 sigma, summed over a layer's bottlenecks): the kernels themselves report an operand that leaves the
            # split-fp16 range at run time (`take_status`), and BUSCA.settle re-runs such a batch on the exact-f32 extractor
            self.x3_activation_bound, self.x3_activation_bound_where = weights.x3_activation_bound(state_dict, prefix)
        want = ctx.lib.busca_reid_blob_floats()
        assert self._blob.size == want, (self._blob.size, want)
        self._upload()

    def _upload(self):
        ctx = self.ctx
        ctx.check(ctx.lib.busca_reid_load_weights_ex(ctx.h, self._blob.ctypes.data, self._blob.size, PRECISIONS[self.precision]))
        if self._running is not None:       # the weight load dropped them
            ctx.check(ctx.lib.busca_reid_load_running_stats(ctx.h, self._running.ctypes.data, self._running.size))
        ctx.reid_owner = weakref.ref(self)

    def _ensure_loaded(self):
        """A busca_ctx holds ONE ReID weight set and its running statistics; restore this model's if another handle replaced them (see dt.py).
        The handle that is replaced saves statistics an adapt() has moved first (`_yield_context`)."""
        owner = getattr(self.ctx, "reid_owner", None)
        other = owner() if owner is not None else None
        if other is not self:
            if other is not None:
                other._yield_context()
            self._upload()

    def _yield_context(self):
        """Another handle is about to load its weights into this context: keep what adapt() did to the running statistics."""
        if self._running_dirty:
            self._running = self._read_running()
            self._running_dirty = False

    def _read_running(self):
        out = np.empty(self.ctx.lib.busca_reid_running_floats(), np.float32)
        s = torch.cuda.current_stream(torch.device("cuda", self.ctx.device)).cuda_stream
        self.ctx.check(self.ctx.lib.busca_reid_get_running_stats(self.ctx.h, out.ctypes.data, out.size, s))
        return out

    # ---- running-statistics BatchNorm (include/busca_reid_bn.h) ----------------------------------------------------------
    def load_running_stats(self, sd_or_blob, prefix=""):
        """A state_dict with `running_mean` / `running_var` of every BatchNorm (weights.reid_running_blob) or the flat blob itself."""
        blob = weights.reid_running_blob(sd_or_blob, prefix) if hasattr(sd_or_blob, "keys") else np.ascontiguousarray(sd_or_blob, dtype=np.float32).ravel()
        self._ensure_loaded()
        self.ctx.check(self.ctx.lib.busca_reid_load_running_stats(self.ctx.h, blob.ctypes.data, blob.size))
        self._running, self._running_dirty = blob.copy(), False

    def reset_running_stats(self):
        """BatchNorm2d.reset_running_stats() on every BatchNorm: mean 0, variance 1."""
        self._ensure_loaded()
        self.ctx.check(self.ctx.lib.busca_reid_reset_running_stats(self.ctx.h))
        self._running, self._running_dirty = weights.reid_running_reset(), False

    def running_stats(self):
        """The running statistics as the device holds them now (numpy [2 x 26 560], the layout of weights.reid_running_blob); synchronises the current stream."""
        self._ensure_loaded()
        self._running, self._running_dirty = self._read_running(), False
        return self._running.copy()

    def _crops(self, crops_u8):
        dev = torch.device("cuda", self.ctx.device)
        if not torch.is_tensor(crops_u8):
            crops_u8 = torch.from_numpy(np.ascontiguousarray(crops_u8))
        crops_u8 = crops_u8.to(dev).contiguous()
        assert crops_u8.dtype == torch.uint8 and tuple(crops_u8.shape[1:]) == (384, 128, 3), crops_u8.shape
        return dev, crops_u8

    def _flags(self, zero_norm, n, dev, stream):
        """`zero_norm` as the kernels read it: n bytes on the context's device (or None).  A cuda uint8 / bool tensor of shape [n] on that device passes as it
        is - no copy, no synchronising call; a numpy array or a sequence of n flags is staged on the stream of the call (h2d_async); the caller keeps the result
        alive until the pass is enqueued.  Anything else - another dtype, shape or device, a host tensor - would be read as bytes that are not there: ValueError."""
        if zero_norm is None:
            return None
        if torch.is_tensor(zero_norm):
            if zero_norm.dtype not in (torch.uint8, torch.bool) or tuple(zero_norm.shape) != (n,) or zero_norm.device != dev or not zero_norm.is_contiguous():
                raise ValueError("zero_norm: a contiguous uint8 / bool tensor of shape (%d,) on %s (or a numpy array / sequence of %d flags), not %s %s on %s"
                                 % (n, dev, n, zero_norm.dtype, tuple(zero_norm.shape), zero_norm.device))
            return zero_norm
        flags = np.asarray(zero_norm)
        if flags.dtype.kind not in "bui" or flags.shape != (n,):
            raise ValueError("zero_norm: %d flags (bool / integer), not %s %s" % (n, flags.dtype, flags.shape))
        return geometry.h2d_async((flags != 0).astype(np.uint8), dev, stream)

    def forward_running(self, crops_u8, output="plain", stream=None, zero_norm=None):
        """Eval-mode forward: BatchNorm on the running statistics, so crop i's features depend on crop i alone.  `output`: "plain" (L2-normalised, as
        `forward`), "norm" (fc7 as it is) or "neck" (= "norm": the encoder has no neck)."""
        self._ensure_loaded()
        dev, crops_u8 = self._crops(crops_u8)
        n = crops_u8.shape[0]
        feats = torch.empty(n, 512, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        zn = self._flags(zero_norm, n, dev, stream)
        self.ctx.check(self.ctx.lib.busca_reid_forward_running(self.ctx.h, crops_u8.data_ptr(), n, _ptr(zn), OUTPUTS[output], feats.data_ptr(), s))
        return feats

    def adapt(self, crops_u8, momentum, output="plain", stream=None, zero_norm=None):
        """Train-mode forward: batch-statistics features (those of `forward`) and torch's update of the running statistics,
        running = (1 - momentum) running + momentum batch with the unbiased batch variance, on the stream.  momentum 0 changes nothing and needs no
        running statistics: a batch-statistics forward with an `output` choice."""
        self._ensure_loaded()
        dev, crops_u8 = self._crops(crops_u8)
        n = crops_u8.shape[0]
        feats = torch.empty(n, 512, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        zn = self._flags(zero_norm, n, dev, stream)
        self.ctx.check(self.ctx.lib.busca_reid_adapt(self.ctx.h, crops_u8.data_ptr(), n, _ptr(zn), float(momentum), OUTPUTS[output], feats.data_ptr(), s))
        if float(momentum) != 0.0 and n > 0:
            self._running_dirty = True
        return feats

    def take_status(self):
        """Call once the streams of this extractor's forwards are SYNCHRONISED.  True: a split-fp16 (x3) forward since the last call staged an activation beyond
        |x| = 1023.5 (`reid_status` 2, include/busca_hip.h) - its BatchNorm statistics, hence the features of that batch, are not finite / not valid, and the caller
        must compute the batch again on an exact-f32 extractor (BUSCA.settle does).  The status is cleared.  Always False for the f32 / f16 flavours."""
        if self.precision != "x3":
            return False
        st = self.ctx.get_option("reid_status")
        if st:
            self.ctx.set_option("reid_status", 0)
        return st != 0

    def reserve(self, n, stream=None):
        """Size the workspace that forwards on `stream` (default: the current stream) use for batches of up to n crops NOW
        (busca_reid_reserve), so that no later forward synchronises the device and allocates."""
        self._ensure_loaded()
        dev = torch.device("cuda", self.ctx.device)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        self.ctx.check(self.ctx.lib.busca_reid_reserve(self.ctx.h, int(n), s))

    def forward(self, crops_u8, stream=None, zero_norm=None, weights=None):
        """`zero_norm` (cuda u8 / bool [n], a numpy array / sequence of n flags, or None; `_flags`): crops flagged 1 are 0.0 after normalisation (busca_reid_forward_ex).
        `weights` (numpy / sequence of n multiplicities, or None): crop i stands for weights[i] identical crops of the BatchNorm
        batch - each distinct crop is computed once, the batch statistics count it weights[i] times (busca_reid_forward_w)."""
        self._ensure_loaded()
        dev = torch.device("cuda", self.ctx.device)
        if not torch.is_tensor(crops_u8):
            crops_u8 = torch.from_numpy(np.ascontiguousarray(crops_u8))
        crops_u8 = crops_u8.to(dev).contiguous()
        assert crops_u8.dtype == torch.uint8 and tuple(crops_u8.shape[1:]) == (384, 128, 3), crops_u8.shape
        n = crops_u8.shape[0]
        feats = torch.empty(n, 512, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        zn = self._flags(zero_norm, n, dev, stream)
        wd, wsum = None, 0.0
        if weights is not None and not (np.asarray(weights) != 1).any():
            weights = None                      # every crop once: the plain forward (same schedule, bit for bit)
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            assert w.shape == (n,) and (w >= 1).all()
            wsum = float(w.astype(np.float64).sum())
            wd = geometry.h2d_async(w, dev, stream)     # ordered on the stream the pass runs on
        self.ctx.check(self.ctx.lib.busca_reid_forward_w(self.ctx.h, crops_u8.data_ptr(), n, _ptr(zn), _ptr(wd), wsum, feats.data_ptr(), s))
        return feats
