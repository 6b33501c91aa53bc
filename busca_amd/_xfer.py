"""Host -> device plumbing shared by every module that fronts libbusca_hip.so: the device and the raw current stream of a Context, and the two
upload routes.  A leaf module (torch and numpy only); it fronts no header and restates nothing of the reference.

The two routes are not interchangeable - which call site takes which is what the stream-order tests pin and what the benchmark times:
  to_dev         a pageable `.to(dev)`: a SYNCHRONOUS copy on the current stream (cost matrices, features, index vectors of the association calls)
  h2d_async / small_to_dev   pinned staging and an asynchronous copy: the host does not wait for the stream (GhostMotion's slot lists, ECC frames)"""
import numpy as np
import torch

_NP_DTYPE = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32}


def dev_of(ctx):
    return torch.device("cuda", ctx.device)


def stream_of(where):
    """The raw handle of torch's current stream on a Context's device, or on a torch.device."""
    return torch.cuda.current_stream(where if isinstance(where, torch.device) else dev_of(where)).cuda_stream


def to_dev(x, dev, dtype, flat=False):
    """A contiguous device tensor of `dtype` (float64, float32 or int32) of a host array or a tensor; None stays None.  A device tensor that already
    is contiguous and of that dtype is used in place (same data_ptr, no copy).  A host array is converted on the host - `flat`: and reshaped to one
    dimension - and uploaded with a pageable, synchronous copy; a read-only array is copied first (torch.from_numpy wants a writeable one)."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = np.ascontiguousarray(np.asarray(x, dtype=_NP_DTYPE[dtype]))
        if flat:
            x = x.reshape(-1)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())
    return x.to(device=dev, dtype=dtype).contiguous()


def h2d_async(arr, dev, stream=None):
    """Small host array -> device tensor without the host waiting for the stream: pinned staging (torch's caching host allocator keeps the block until the copy has
    run) + an asynchronous copy.  A plain `.to(dev)` of a pageable array is a SYNCHRONOUS copy on the current stream: enqueued behind a ReID pass it parks the host
    until the pass is done, and everything the host still has to enqueue (index gathers, the Decision-Transformer launch) then starts late.
    `stream` (a raw HIP stream, or None for torch's current one): the stream of the kernel that reads the tensor - the copy is ordered on it."""
    t = arr.contiguous() if torch.is_tensor(arr) else torch.from_numpy(np.ascontiguousarray(arr))
    if t.device.type != "cpu":
        return t.to(dev)
    if stream is None:
        return t.pin_memory().to(dev, non_blocking=True)
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
        return t.pin_memory().to(dev, non_blocking=True)


def small_to_dev(x, dev, dtype):
    """A small index / flag vector on the device; a host array goes through pinned staging (h2d_async), so the host does not wait for the stream."""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x.to(device=dev, dtype=dtype).contiguous().view(-1)
    return h2d_async(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dtype), dev)
