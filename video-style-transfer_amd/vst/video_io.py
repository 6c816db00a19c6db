"""Host side of the video inference paths (vst.reconet.inference, vst.adaattn.inference,
vst.rtnstv.inference): the
cv2.VideoCapture-like frame reader, the per-frame check / host resize, and the pinned staging buffer
that uploads a chunk of uint8 frames with one async copy and turns it into fp32 planes on the device.
"""
import numpy as np
import torch

from . import ops


def cv2_module():
    try:
        import cv2  # noqa: PLC0415
    except ImportError as e:  # pragma: no cover - cv2 is absent in this image
        raise ImportError("reading video files / resizing frames needs OpenCV (cv2), as the reference does") from e
    return cv2


class FrameSource:
    """cv2.VideoCapture-like reader: `.read() -> (ret, frame)` over a path or in-memory frames."""

    def __init__(self, video):
        if isinstance(video, (str, bytes)) or hasattr(video, "__fspath__"):
            self._cap = cv2_module().VideoCapture(str(video))
            self._it = None
        else:
            self._cap = None
            self._it = iter(video)

    def read(self):
        if self._cap is not None:
            return self._cap.read()
        try:
            return True, next(self._it)
        except StopIteration:
            return False, None

    def release(self):
        if self._cap is not None:
            self._cap.release()


def host_frame(frame, hw, interpolation):
    """Check one cv2-style frame (HxWx3 uint8) and bring it to hw = (H, W): frames already at that
    size need no cv2, others go through cv2.resize with the named interpolation, as the reference's."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frames must be HxWx3 uint8 (cv2 BGR), got {frame.dtype} {frame.shape}")
    if frame.shape[:2] != tuple(hw):
        cv2 = cv2_module()
        frame = cv2.resize(frame, (hw[1], hw[0]), interpolation=getattr(cv2, interpolation))
    return np.ascontiguousarray(frame)


class PinnedUploader:
    """One pinned uint8 buffer of `capacity` frames, reused chunk after chunk."""

    def __init__(self, device, capacity):
        self.device, self.capacity = device, max(1, int(capacity))
        self.pinned = None

    def upload_u8(self, frames):
        """k <= capacity host frames (HxWx3 uint8) -> the same bytes, (k, H, W, 3) uint8 on the device
        (for consumers that read the frames themselves: ops.conv_stem_u8)."""
        dev = self._stage(frames)
        torch.cuda.current_stream().synchronize()  # the pinned buffer is reused by the next chunk
        return dev

    def upload(self, frames, bgr=True):
        """k <= capacity host frames (HxWx3 uint8) -> (k, 3, H, W) fp32 RGB planes on the device."""
        out = ops.frames_to_tensor(self._stage(frames), bgr=bgr)
        # the pinned buffer is reused by the next chunk: wait for this copy first
        torch.cuda.current_stream().synchronize()
        return out

    def _stage(self, frames):
        k = len(frames)
        H, W = frames[0].shape[:2]
        shape = (max(self.capacity, k), H, W, 3)
        if self.pinned is None or tuple(self.pinned.shape) != shape:
            self.pinned = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        host = self.pinned[:k].numpy()
        for i, f in enumerate(frames):
            host[i] = f
        return self.pinned[:k].to(self.device, non_blocking=True)
