"""Image crops of one frame and the host classes that stand for them while they live in the device crop pool.  Fronts busca_crop_gather_ex,
busca_crop_gather_sized and busca_gather_crops of include/busca_hip.h through busca_amd/geometry.py; restates get_bbox_crop / _cutout_with_pad
(busca/tracking.py:62-113) and get_image_crops with its normalisation (busca/network.py:470-507)."""
import numpy as np
import torch

from . import geometry
from .crop_pool import Slot
from .geometry import box_extents

_PIXEL_MEAN = np.array([0.406, 0.456, 0.485])   # BGR
_PIXEL_STD = np.array([0.225, 0.224, 0.299])    # BGR; 0.299 is the reference's "ghost" normalisation


def normalize_crops(u8):
    """(x/255 - mean)/std in BGR order, float32 (busca/network.py:470-478)."""
    x = np.asarray(u8).astype(np.float32) / 255.0
    x -= _PIXEL_MEAN
    x /= _PIXEL_STD
    return x


class DeviceBackedCrops(np.ndarray):
    """Host uint8 crops that remember their device-resident twins (device-resident track memory).

    `get_image_crops(..., normalize=False)` returns this ndarray subclass: to the trackers it is an ordinary uint8
    array ([N,384,128,3] with REAL host bytes; `crops[i]` is what they append to `images_mem`), but `crops[i]` also
    carries `.slot`, its slot in the bounded device pool (busca_amd/crop_pool.py).  `associate_embeddings` gathers
    slots on the GPU and skips the per-frame host->device copy of B*(L+P) crops (147 KB each).  Anything that loses
    the slot (np.array(...) copies, pickling, arithmetic) is still a correct host crop and takes the host path."""

    def __new__(cls, host, slots):
        host = np.asarray(host)
        obj = host.view(cls)
        obj._slots = slots
        obj._host = host                    # the plain array: slot.host views must not reference this subclass (no cycles)
        obj.slot = None
        return obj

    def __array_finalize__(self, obj):
        self._slots = None                  # generic views/copies do not know which pool slots they cover
        self._host = None
        self.slot = None

    def __getitem__(self, key):
        if self._slots is not None and self.ndim == 4 and isinstance(key, (int, np.integer)):
            # the crop is a view of the PLAIN host array: it keeps the frame's host bytes alive (as the reference's
            # np.stack'ed crops do) but not this container, so the other crops' pool slots are free to go
            k = int(key)
            out = self._host[k].view(DeviceBackedCrops)
            out.slot = self._slots[k]
            if out.slot.host is None:
                out.slot.host = self._host[k]             # a spill of this crop needs no device->host copy
            return out
        return super().__getitem__(key)

    def __reduce__(self):                   # pickling / copy.deepcopy: a plain host array (the slot stays with this process)
        return np.asarray(self).__reduce__()

    @property
    def dev(self):
        """cuda u8 view of this crop's slot ([384,128,3]); None for non-crop views and after a spill."""
        return self.slot.tensor() if self.slot is not None else None


class FrameHostCopy:
    """The host bytes of one get_image_crops call, ON DEMAND (round 5): the crops live in pool slots; nothing is copied to the host until somebody
    reads a pixel.  The first host read of ANY crop of the call fetches the WHOLE batch in one go - one index-gather launch over the call's slots
    (busca_gather_crops) and one device->host copy - so a tracker that looks at every crop pays one transfer per call, and one that never looks
    (the five adapters only store the crops and hand them back to associate_embeddings) pays nothing: no pinned buffer, no copy, no side stream
    (rounds 3-4 enqueued a 17 MB pinned copy per call whether or not anyone read it: 0.12 ms of host time per call).
    A slot that was released and reused before the read shows another crop's bytes in its row - a row nobody can ask for any more."""
    __slots__ = ("ctx", "ptrs", "event", "_np", "expired")

    def __init__(self, ctx=None, ptrs=None, event=None):
        self.ctx, self.ptrs, self.event, self._np, self.expired = ctx, ptrs, event, None, False

    def rows(self):
        """uint8 [n,384,128,3] host view of the batch (fetched on the first call)."""
        if self._np is None:
            if self.event is not None:
                torch.cuda.current_stream(geometry.dev_of(self.ctx)).wait_event(self.event)      # the crop kernel may have run on another stream
            self._np = geometry.gather_crops(self.ctx, self.ptrs).cpu().numpy()
            self.event = None
        return self._np


DeviceCrop = Slot                       # one object per crop: the pool slot IS what the tracker stores (busca_amd/crop_pool.py)


class DeviceCrops:
    """Sequence of DeviceCrop ([N,384,128,3] uint8 to duck-typing callers); `crops[i]` is what a tracker stores."""
    dtype, ndim = np.dtype(np.uint8), 4

    def __init__(self, slots):
        self._items = list(slots)

    @property
    def shape(self):
        return (len(self._items), 384, 128, 3)

    def __len__(self):
        return len(self._items)

    def __iter__(self):
        return iter(self._items)

    def __getitem__(self, key):
        if isinstance(key, (int, np.integer)):
            return self._items[int(key)]
        return np.asarray(self)[key]

    def __array__(self, dtype=None, copy=None):
        a = np.stack([np.asarray(c) for c in self._items]) if self._items else np.zeros((0, 384, 128, 3), np.uint8)
        return a if dtype is None else a.astype(dtype)


def get_image_crops(im, bboxes, normalize=True, ctx=None, device_only=False, host_copy=None, output_size=None):
    """All crops of one frame in one launch: u8 BGR [N,384,128,3] (float32 normalised if `normalize`).
    With normalize=False every crop is written into a slot of the device crop pool and the returned crops remember
    their slot.  `host_copy` says what happens to the HOST bytes of those crops (147 KB each - the bulk of this call when it
    is waited for; busca/network.py:492-507 returns host arrays):
      "lazy"  (default) nothing is copied until somebody reads a pixel: the returned `DeviceCrops` fetch the whole batch with one
              gather + one device->host copy on the first host read of any of its crops;
      "eager" wait for it: a real uint8 ndarray (`DeviceBackedCrops`) - for callers that need ndarray instances;
      "never" (`device_only=True`) no copy at all; a host read copies that one crop back synchronously."""
    rects = box_extents(bboxes)
    sized = output_size is not None and tuple(int(v) for v in output_size) != (128, 384)
    if len(rects) == 0:
        return np.zeros([0, int(output_size[0]), int(output_size[1]), 3]) if sized else np.zeros([0, 128, 384, 3])     # the reference's (transposed) empty shape, network.py:503
    ctx = ctx or geometry.default_context()
    if sized:
        # `output_size` = (width, height) as cv2.resize takes it (tracking.py:71): plain host arrays [N, height, width, 3], no pool slots -
        # only the 384 x 128 crops are ReID inputs
        u8 = geometry.crop_gather_sized(ctx, im, rects, int(output_size[0]), int(output_size[1])).cpu().numpy()
        return normalize_crops(u8) if normalize else u8
    if normalize:
        u8, _ = geometry.crop_gather(ctx, im, rects, want_u8=True)
        return normalize_crops(u8.cpu().numpy())
    if host_copy is None:
        host_copy = "never" if device_only else "lazy"
    if host_copy not in ("lazy", "eager", "never"):
        raise ValueError("host_copy must be 'lazy', 'eager' or 'never', not %r" % (host_copy,))
    pool = geometry.crop_pool(ctx)
    frame = FrameHostCopy() if host_copy == "lazy" else None
    slots = pool.alloc(len(rects), frame)
    ptrs = np.fromiter((s.ptr for s in slots), dtype=np.uint64, count=len(slots))
    if host_copy == "eager":
        packed, _ = geometry.crop_gather(ctx, im, rects, want_u8=True, dst_ptrs=ptrs)    # the same launch also writes the batch as one contiguous buffer (the slots need not be adjacent)
        return DeviceBackedCrops(packed.cpu().numpy(), slots)
    geometry.crop_gather(ctx, im, rects, want_u8=False, dst_ptrs=ptrs)
    if host_copy == "lazy":                                   # pool slots only; the host bytes are fetched by the first host read (FrameHostCopy)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(geometry.dev_of(ctx)))
        frame.ctx, frame.ptrs, frame.event = ctx, ptrs, ev
    return DeviceCrops(slots)


def get_bbox_crop(im, bbox_real_scale, output_size=(128, 384), normalize=True, ghost_normalize=True, ctx=None):
    """Single crop (busca/tracking.py:62-78); `output_size` = (width, height) as cv2.resize takes it."""
    crop = np.asarray(get_image_crops(im, [bbox_real_scale], normalize=False, ctx=ctx, output_size=output_size)[0])
    if normalize:
        crop = crop.astype(np.float32) / 255.0
        crop -= _PIXEL_MEAN
        crop /= (_PIXEL_STD if ghost_normalize else np.array([0.225, 0.224, 0.229]))
    return crop
