"""Device tracking: the box, the crop intrinsics and the crop of frame t + 1 from frame t's device pose, without a host round trip
(opt-in; ``frameloop.project_bbox`` / ``crop_geometry`` / ``crop_query`` on host values stay the default).

The work is HIP (``csrc/track_box.hip``, ``csrc/track_crop.hip`` in ``libonepose_track.so``, include/onepose_track.h).  CPU tensors raise
:class:`hip.HipLibraryError` (no CPU fallback).  The specification (``tests/track_device_oracle.py`` restates the two
box entries in numpy float64 with every sum in one fixed order):

* a :class:`TrackState` is what a frame is cropped and solved with: ``box`` int32 ``[x0, y0, x1, y1]``, ``flag`` int32, ``K_crop`` and
  ``trans`` float64 ``[3, 3]`` (``crop_geometry``'s pair for that box), all on the device;
* :func:`set_box` writes a box the host chose (the detector's) with flag 0;
* :func:`next_box` writes the state of the next frame from one frame of a ``pnp_device.DevicePoses``: flag 0 and ``project_bbox``'s box
  when the host loop would have projected, otherwise the previous box carried over and the reason in the flag -- ``LOST_POSE`` (no pose,
  or fewer than ``min_inliers`` inliers), ``NEEDS_HOST`` (the solve asks for more trials than ran), ``STALE`` (the previous state was
  flagged already), and, only when none of these is set, ``LOST_BOX`` (the projection is empty, non-finite or outside int32);
* :func:`crop` is ``ophip_crop_resize_gray`` with the box read from the state.

Nothing is synchronised or read back: ``state.K_crop`` goes to ``pnp_device.ransac_pnp`` / ``enqueue_after`` as the device tensor they
accept, and :meth:`TrackState.blob` is one contiguous byte block for a packed read-back.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
LOST_POSE, LOST_BOX, STALE, NEEDS_HOST, MAX_BOX_SIDE, MAX_CROP = map(_BINDING.constant, (
    "LOST_POSE", "LOST_BOX", "STALE", "NEEDS_HOST", "MAX_BOX_SIDE", "MAX_CROP"))
# byte offsets of a state's fields in its block: box 16, flag 4 (+ 4 of padding), K_crop 72, trans 72
_O_BOX, _O_FLAG, _O_KCROP, _O_TRANS, STATE_BYTES = 0, 16, 24, 96, 168


class TrackState:
    """``box [4]`` int32, ``flag [1]`` int32, ``K_crop [3, 3]`` and ``trans [3, 3]`` float64: views of one device block (``blob``,
    ``STATE_BYTES`` bytes), written by :func:`set_box` or :func:`next_box`."""

    def __init__(self, device):
        self.blob = torch.empty(STATE_BYTES, dtype=torch.uint8, device=device)
        self.box = self.blob[_O_BOX:_O_BOX + 16].view(torch.int32)
        self.flag = self.blob[_O_FLAG:_O_FLAG + 4].view(torch.int32)
        self.K_crop = self.blob[_O_KCROP:_O_KCROP + 72].view(torch.float64).view(3, 3)
        self.trans = self.blob[_O_TRANS:_O_TRANS + 72].view(torch.float64).view(3, 3)

    @staticmethod
    def unpack(raw):
        """``(box int32[4], flag, K_crop [3, 3], trans [3, 3])`` of a block's bytes on the host (a uint8 numpy array)"""
        raw = np.ascontiguousarray(raw[:STATE_BYTES])
        return (raw[_O_BOX:_O_BOX + 16].view(np.int32).copy(), int(raw[_O_FLAG:_O_FLAG + 4].view(np.int32)[0]),
                raw[_O_KCROP:_O_KCROP + 72].view(np.float64).reshape(3, 3).copy(), raw[_O_TRANS:_O_TRANS + 72].view(np.float64).reshape(3, 3).copy())

    def to_host(self):
        """:meth:`unpack` of this state: one read-back (a synchronisation)"""
        return TrackState.unpack(self.blob.cpu().numpy())


def check_K(K) -> torch.Tensor:
    """The intrinsics as float64 ``[9]``: a tensor where it lies, host numbers as a host tensor"""
    if not isinstance(K, torch.Tensor):
        K = torch.as_tensor(np.ascontiguousarray(np.asarray(K, dtype=np.float64)))
    if K.dtype != torch.float64 or K.numel() != 9:
        raise ValueError("K: float64 [3, 3]")
    return K.contiguous().view(9)


def _device_K(K, device):
    """:func:`check_K` on the device: a device tensor as it is, host numbers uploaded"""
    if isinstance(K, torch.Tensor):
        hip.on_device([K])
        return check_K(K)
    K = check_K(K)
    if device is None or torch.device(device).type != "cuda":
        raise hip.HipLibraryError("the HIP path needs a HIP device (no CPU fallback)")
    return K.to(device)


def check_crop_size(crop_size) -> int:
    if int(crop_size) != crop_size or not 1 <= crop_size <= MAX_CROP:
        raise ValueError(f"crop_size: an integer in [1, {MAX_CROP}]")
    return int(crop_size)


def set_box(bbox, K, crop_size: int = 512, device=None) -> TrackState:
    """The state of a box the host chose: ``bbox`` four host integers ``[x0, y0, x1, y1]`` with ``x1 > x0`` and ``y1 > y0``; ``K`` the
    full-frame intrinsics, a float64 device tensor (or host numbers, uploaded to ``device``).  Enqueued on the current stream."""
    x0, y0, x1, y1 = [int(v) for v in bbox]
    if not all(-2 ** 31 <= v < 2 ** 31 for v in (x0, y0, x1, y1)):
        raise ValueError("bbox: four int32")
    S = check_crop_size(crop_size)
    if isinstance(K, torch.Tensor) and K.is_cuda:
        device = K.device
    Kd = _device_K(K, device)
    st = TrackState(Kd.device)
    with hip.enqueue_on(Kd.device):
        launch("optrk_box_set", dict(x0=x0, y0=y0, x1=x1, y1=y1, K=Kd, S=S, box=st.box, flag=st.flag, K_crop=st.K_crop, trans=st.trans))
    return st


def next_box(poses, prev_state: TrackState, K, bbox3d, *, frame: int = 0, min_inliers: int = 20, crop_size: int = 512) -> TrackState:
    """The state of the frame after the one ``poses`` (a ``pnp_device.DevicePoses``) holds at index ``frame``; ``prev_state`` is the
    state that frame was cropped with; ``K`` full-frame intrinsics and ``bbox3d [8, 3]`` float64 device tensors.  Enqueued on the current
    stream -- the one the solve was enqueued on, so that the stream orders the two and the allocator may reuse the inputs afterwards;
    nothing is read back."""
    for named in (("poses.pose", poses.pose), ("poses.n_inliers", poses.n_inliers), ("poses.status", poses.status), ("bbox3d", bbox3d)):
        hip.need_device([named])                    # one at a time: the first input that is wrong in either way is the one reported
    if not isinstance(prev_state, TrackState):
        raise TypeError("prev_state: a TrackState")
    F = poses.pose.shape[0]
    if int(frame) != frame or not 0 <= frame < F:
        raise ValueError(f"frame: an integer in [0, {F})")
    if int(min_inliers) != min_inliers or min_inliers < 0:
        raise ValueError("min_inliers: an integer >= 0")
    if bbox3d.dtype != torch.float64 or tuple(bbox3d.shape) != (8, 3):
        raise ValueError("bbox3d: float64 [8, 3]")
    S = check_crop_size(crop_size)
    Kd = _device_K(K, bbox3d.device)
    bbox3d = bbox3d.contiguous()
    pose = poses.pose[frame].contiguous()
    n_in, status = poses.n_inliers[frame:frame + 1], poses.status[frame:frame + 1]
    st = TrackState(Kd.device)                           # no reference to the inputs: a chain of states must not keep every solve's workspace
    with hip.enqueue_on(Kd.device):
        launch("optrk_box_from_pose", dict(K=Kd, pose=pose, n_inliers=n_in, status=status, bbox3d=bbox3d, prev_box=prev_state.box,
                                           prev_flag=prev_state.flag, min_inliers=min_inliers, S=S, box=st.box, flag=st.flag, K_crop=st.K_crop,
                                           trans=st.trans))
    return st


def crop(frame_u8: torch.Tensor, state: TrackState, crop_size: int = 512) -> torch.Tensor:
    """uint8 ``[H, W]`` frame on the HIP device -> ``[1, 1, S, S]`` float query image in [0, 1]: ``frameloop.crop_query`` with the box of
    ``state``, bit for bit; an empty box gives zeros."""
    if not isinstance(frame_u8, torch.Tensor) or frame_u8.dtype != torch.uint8 or frame_u8.dim() != 2 or not frame_u8.is_cuda:
        raise hip.HipLibraryError("crop needs a uint8 [H, W] frame on the HIP device (no CPU fallback)")
    S = check_crop_size(crop_size)
    frame_u8 = frame_u8.contiguous()
    out = torch.empty(1, 1, S, S, dtype=torch.float32, device=frame_u8.device)
    with hip.enqueue_on(frame_u8.device):
        launch("optrk_crop", dict(image=frame_u8, H=frame_u8.shape[0], W=frame_u8.shape[1], box=state.box, S=S, out=out))
    return out
