"""Camera-motion estimation (ECC image alignment) and the two trackers' compensation steps on top of it.  Fronts busca_ecc_align of
include/busca_hip.h (u8 BGR frames, ByteTrack) and include/busca_ecc.h (float32 frames with a Gaussian pre-blur, GHOST); restates
BYTETracker.camera_motion_compensation (adapters/ByteTrack/yolox/tracker/byte_tracker.py:626-650) and BaseTracker.motion_compensation
(adapters/GHOST/src/base_tracker.py:60-65,600-633).  OpenCV's findTransformECC arithmetic is third-party and restated: see oracle/ecc.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib, geometry
from ._xfer import h2d_async, stream_of
from .track_boxes import warp_pos

_GHOST_WARP_MODES = {"Translation": _lib.ECC_TRANSLATION, "Affine": _lib.ECC_AFFINE, "Euclidean": _lib.ECC_EUCLIDEAN}     # warp_mode_dct, base_tracker.py:60-65


def _start_warp(warp_matrix):
    """The float32 [2,3] warp an alignment starts from and updates in place: the identity, or a copy of the caller's."""
    return np.eye(2, 3, dtype=np.float32) if warp_matrix is None else np.ascontiguousarray(warp_matrix, dtype=np.float32).reshape(2, 3).copy()


def find_transform_ecc(prev_frame, cur_frame, warp_matrix=None, motion="MOTION_EUCLIDEAN", number_of_iterations=100,
                       termination_eps=1e-5, ctx=None):
    """cv2.cvtColor(BGR2GRAY) + cv2.findTransformECC(templateImage=prev, inputImage=cur, ...) on the GPU (busca_ecc_align;
    third-party OpenCV arithmetic restated, see oracle/ecc.py).  Frames: u8 BGR [H,W,3] (numpy or cuda tensors).
    Returns (cc, warp float32 [2,3]); raises BuscaError where OpenCV raises (no convergence / NaN)."""
    ctx, dev = geometry.ctx_dev(ctx)
    if motion not in ("MOTION_EUCLIDEAN", "MOTION_AFFINE"):
        raise ValueError("Invalid warp_mode: {}".format(motion))
    fr = []
    for f in (prev_frame, cur_frame):
        if not torch.is_tensor(f):
            f = torch.from_numpy(np.ascontiguousarray(f))
        f = f.to(dev).contiguous()
        assert f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3
        fr.append(f)
    assert fr[0].shape == fr[1].shape
    H, W = fr[0].shape[:2]
    warp = _start_warp(warp_matrix)
    cc, its = C.c_double(0.0), C.c_int32(0)
    ctx.check(ctx.lib.busca_ecc_align(ctx.h, fr[0].data_ptr(), fr[1].data_ptr(), H, W, fr[0].stride(0), fr[1].stride(0),
                                      0 if motion == "MOTION_EUCLIDEAN" else 1, int(number_of_iterations), float(termination_eps),
                                      warp.ctypes.data, C.byref(cc), C.byref(its), stream_of(dev)))
    find_transform_ecc.last_iterations = its.value
    return cc.value, warp


def camera_motion_compensation(track_pool, last_image, current_frame, frame_id=2, number_of_iterations=100, termination_eps=0.00001,
                               warp_mode="MOTION_EUCLIDEAN", ctx=None):
    """BYTETracker.camera_motion_compensation (byte_tracker.py:626-650): estimate the previous->current frame warp and move every
    track of `track_pool` by it (`STrack.apply_camera_motion`, :123-137: position (mean[:2] or _tlwh[:2]) * scale -> warp ->
    / scale).  Returns the correlation coefficient (1.0 on the first frame, as the reference does)."""
    cc = 1.0
    if frame_id > 1 and last_image is not None:
        cc, warp = find_transform_ecc(last_image, current_frame, None, warp_mode, number_of_iterations, termination_eps, ctx=ctx)
        for t in track_pool:
            if hasattr(t, "apply_camera_motion"):
                t.apply_camera_motion(warp)
                continue
            holder = t.mean if getattr(t, "mean", None) is not None else t._tlwh
            new_pos = warp_pos(np.asarray(holder[:2], dtype=np.float64) * t.scale, warp) / t.scale
            holder[:2] = new_pos
    return cc


def ghost_ecc_check_config(motion_cfg):
    """motion_config['warp_mode'] -> the motion code of busca_ecc_align_planes.  'Homography' is refused; an unknown name raises KeyError, as
    `self.warp_mode_dct[...]` does."""
    mode = motion_cfg["warp_mode"]
    if mode == "Homography":
        raise ValueError("GHOST warp_mode 'Homography' is refused: the reference always passes np.eye(2, 3) (base_tracker.py:613) and OpenCV asserts a "
                         "3-row warp matrix for homographies, so this branch raises in the reference and there is nothing to reproduce")
    return _GHOST_WARP_MODES[mode]


def _ecc_frame(frame, dev):
    """A float32 frame [3,H,W] or [H,W] on the device, strides kept (a host frame through pinned staging) -> (tensor, channels, H, W)."""
    if not torch.is_tensor(frame):
        frame = torch.from_numpy(np.asarray(frame))
    if frame.dtype != torch.float32 or frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[0] != 3):
        raise ValueError("an ECC frame is float32 [3,H,W] or [H,W], not %s %s" % (frame.dtype, tuple(frame.shape)))
    if frame.device.type == "cpu":
        frame = h2d_async(frame, dev)
    elif frame.device != dev:
        frame = frame.to(dev)
    if any(s < 0 for s in frame.stride()) or frame.stride(-1) == 0:
        frame = frame.contiguous()
    return frame, (3 if frame.dim() == 3 else 1), int(frame.shape[-2]), int(frame.shape[-1])


def _ecc_prepare(ctx, frame, channels, H, W, ksize, out):
    """busca_ecc_prepare of a device frame into the [H,W] float32 plane `out`, on the current stream."""
    st = frame.stride()
    ctx.check(ctx.lib.busca_ecc_prepare(ctx.h, frame.data_ptr(), channels, H, W, st[0] if channels == 3 else 0, st[-2], st[-1], int(ksize),
                                        out.data_ptr(), stream_of(out.device)))


def _ecc_align_planes(ctx, templ, inp, motion, iters, eps, warp):
    """busca_ecc_align_planes on two [H,W] planes; `warp` (host float32 [2,3]) is updated in place -> (cc, iterations)."""
    H, W = templ.shape
    cc, its = C.c_double(0.0), C.c_int32(0)
    ctx.check(ctx.lib.busca_ecc_align_planes(ctx.h, templ.data_ptr(), inp.data_ptr(), H, W, int(motion), int(iters), float(eps), warp.ctypes.data,
                                             C.byref(cc), C.byref(its), stream_of(templ.device)))
    return cc.value, its.value


def _ecc_motion_code(motion):
    if isinstance(motion, str):
        if motion == "MOTION_HOMOGRAPHY" or motion == "Homography":
            raise ValueError("Invalid warp_mode: {}".format(motion))
        return _GHOST_WARP_MODES[motion[7:].capitalize() if motion.startswith("MOTION_") else motion]
    return int(motion)


def find_transform_ecc_f32(template, input, warp_matrix=None, motion="Euclidean", gauss_size=15, number_of_iterations=100, termination_eps=1e-5,
                           ctx=None):
    """cv2.cvtColor(RGB2GRAY) + cv2.findTransformECC(template, input, warp_matrix, motion, criteria, None, gauss_size) on float32 frames, on the
    GPU (busca_ecc_prepare x2 + busca_ecc_align_planes; OpenCV's arithmetic restated, parity unpinned: include/busca_ecc.h).  Frames: float32
    [3,H,W] RGB or [H,W] grey, host arrays or cuda tensors of any strides.  motion: 'Translation' | 'Euclidean' | 'Affine' (GHOST's names) or
    'MOTION_...' (OpenCV's).  Returns (cc, warp float32 [2,3]); raises BuscaError where OpenCV raises.  The stateless form, for callers with two
    frames in hand: a tracker prepares every frame once with GhostCameraMotion."""
    code = _ecc_motion_code(motion)
    ctx, dev = geometry.ctx_dev(ctx)
    planes = []
    for f in (template, input):
        f, ch, H, W = _ecc_frame(f, dev)
        planes.append(torch.empty(H, W, dtype=torch.float32, device=dev))
        _ecc_prepare(ctx, f, ch, H, W, gauss_size, planes[-1])
    if planes[0].shape != planes[1].shape:
        raise ValueError("template %s and input %s differ in size" % (tuple(planes[0].shape), tuple(planes[1].shape)))
    warp = _start_warp(warp_matrix)
    cc, its = _ecc_align_planes(ctx, planes[0], planes[1], code, number_of_iterations, termination_eps, warp)
    find_transform_ecc_f32.last_iterations = its
    return cc, warp


class GhostCameraMotion:
    """The estimate of GHOST's motion_compensation on the device (base_tracker.py:605-622, :633): every frame is prepared once - grey, 15-pixel
    Gaussian (busca_ecc_prepare) - and its plane serves as the template of this frame's alignment and as the input of the next one's, so no
    `last_image` is kept and no frame leaves the device.  Reads motion_cfg['warp_mode'], ['num_iter_mc'] and ['termination_eps_mc'].
      estimate(whole_image)  float32 [3,H,W] cuda tensor of any strides (or a host tensor / array, uploaded through pinned staging) -> None on
                             the first frame, then the float32 [2,3] warp of cv2.findTransformECC(current, previous, eye(2,3), ...)
      norm, cc, iterations   of the last estimate: np.linalg.norm(warp[:, -1]) (the reference's warp_matrix_nomr; None on a first frame), the
                             correlation coefficient, the iterations run
      prepared               busca_ecc_prepare calls so far
      reset()                a new sequence: the next frame is a first frame
    Where OpenCV raises (no convergence, singular Hessian) estimate raises BuscaError and the stored plane stays the one of the last good frame,
    as self.last_image does in the reference.  The two planes are allocated with the first frame and swapped from then on."""

    def __init__(self, motion_cfg, gauss_size=15, ctx=None):
        self.motion = ghost_ecc_check_config(motion_cfg)
        self.iters, self.eps = int(motion_cfg["num_iter_mc"]), float(motion_cfg["termination_eps_mc"])
        self.gauss_size = int(gauss_size)
        if self.gauss_size < 1 or self.gauss_size > _lib.ECC_KSIZE_MAX or self.gauss_size % 2 == 0:
            raise ValueError("gauss_size %d is not an odd size in 1 .. %d" % (self.gauss_size, _lib.ECC_KSIZE_MAX))
        self.ctx, self.dev = geometry.ctx_dev(ctx)
        self._planes, self._cur = None, 0               # two [H,W] planes; _planes[_cur] is the stored (previous) frame's
        self.prepared = 0
        self.reset()

    def reset(self):
        self._have = False
        self.norm = self.cc = self.iterations = None

    def estimate(self, whole_image):
        frame, ch, H, W = _ecc_frame(whole_image, self.dev)
        if self._planes is None:
            self._planes = [torch.empty(H, W, dtype=torch.float32, device=self.dev) for _ in range(2)]
        elif tuple(self._planes[0].shape) != (H, W):
            raise ValueError("GhostCameraMotion: a %d x %d frame in a sequence of %d x %d frames" % ((H, W) + tuple(self._planes[0].shape)))
        new = self._planes[1 - self._cur]
        _ecc_prepare(self.ctx, frame, ch, H, W, self.gauss_size, new)
        self.prepared += 1
        self.norm = None
        warp = None
        if self._have:
            warp = np.eye(2, 3, dtype=np.float32)
            self.cc, self.iterations = _ecc_align_planes(self.ctx, new, self._planes[self._cur], self.motion, self.iters, self.eps, warp)
            self.norm = np.linalg.norm(warp[:, -1])
        self._cur, self._have = 1 - self._cur, True
        return warp


def ghost_motion_compensation(camera, motion_state, whole_image, is_moving, enabled=True):
    """BaseTracker.motion_compensation (base_tracker.py:600-633) on the device: the warp of this frame against the previous one
    (camera: GhostCameraMotion) and, when the sequence has a moving camera (`is_moving`) and motion_config['motion_compensation'] (`enabled`),
    every stored position of every track through it (motion_state: GhostMotion).  Returns the warp, None on the first frame."""
    warp = camera.estimate(whole_image)
    if warp is not None and is_moving and enabled:
        motion_state.compensate(warp)
    return warp
