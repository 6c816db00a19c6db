"""MI355X RTNSTV video inference: drop-in for `Inference` (RT/utilities.py:296-332, the class
RT/infer.py drives) and `cvframe_to_tensor` (RT/utilities.py:182-191).

Per frame the reference runs: cv2 BGR uint8 frame -> RGB -> cv2.resize to 640x360 -> `toTensor255` ->
`StylizingNetwork.forward` under no_grad -> HWC -> RGB2BGR -> `astype("uint8")`.  The network is tiny
(16 / 32 / 48 channels), and at one frame per forward its cost is passes and launches, not MFMA time;
`forward_frames` therefore walks the network from the model's own parameters with the inference-only
kernels:
  * the stem: conv1 straight from the uint8 frame (`ops.conv_stem_u8`; no fp32 copy of the frame);
  * every InstanceNorm (+ ReLU, + the residual add) through `ops.instance_norm_infer`, which cuts the
    few large planes of a single frame over many workgroups (split-plane moments + apply);
  * conv2 / conv3 / the residual trunk / the two transposed convs on the existing GEMM kernels
    (`ops.conv2d`, `ops.conv_transpose2d`), conv4 (16 -> 3) on the thin forward (`ops.conv_thin_fwd`);
  * the tail -- conv4's InstanceNorm, Tanh, (t + 1) / 2 * 255, clamp, HWC, BGR, truncation to uint8 --
    in one pass (`ops.instance_norm_tanh_frames`).  The network's output lies in [0, 255] already, so the
    clamp the frame kernels apply changes nothing the reference's `astype("uint8")` sees.
`VST_IN_SPLIT=0` (read at import of vst.ops) runs every norm on the one-workgroup-per-plane kernel and
the tail as three kernels, for A/B runs.

Frames are read on the host in chunks of `batch_frames` (extension; default 1 = the reference's
schedule), staged in one pinned uint8 buffer and uploaded with one copy per chunk, exactly as
vst.reconet.inference does (vst.video_io).  `video_path` may be a file path (cv2.VideoCapture: cv2 must
be importable), a (T,H,W,3) uint8 array or an iterable of cv2-style BGR frames; `model_path` may be a
state dict.  Frames of another size than `resize` = (width, height) go through cv2.resize on the host
like the reference's; `resize=None` (extension) takes the frames as they are and needs H and W to be
multiples of 4 (the two stride-2 convs and their transposes must return to the frame's size).

`calculate_mse` has no counterpart here on purpose: RT/utilities.py:243-293 is an unedited copy of
ReCoNet's that calls `model_class(input_frame_num)` and unpacks `*_, out`, neither of which RTNSTV's
`StylizingNetwork` supports, so there is no behaviour to be faithful to.
"""
import numpy as np
import torch

from .. import ops
from .._lib import VstError
from ..video_io import FrameSource, PinnedUploader, host_frame

FRAME_RESIZE = (640, 360)  # RT/utilities.py:324: cvframe_to_tensor(frame, resize=(640, 360)), (width, height)


def _need_device(device):
    if torch.device(device).type != "cuda":
        raise VstError(f"RTNSTV inference runs on HIP (cuda) devices; there is no CPU path (got {device})")


def _sized(frame, resize):
    """RT/utilities.py:186-189 host part: check, and cv2.resize(INTER_LINEAR) to resize = (width, height)."""
    frame = np.asarray(frame)
    hw = frame.shape[:2] if resize is None else (int(resize[1]), int(resize[0]))
    return host_frame(frame, hw, "INTER_LINEAR")


def _host_frame(frame, resize):
    frame = _sized(frame, resize)
    if frame.shape[0] % 4 or frame.shape[1] % 4:
        raise VstError(f"RTNSTV frames need a height and width that are multiples of 4, got {frame.shape[:2]}")
    return frame


def cvframe_to_tensor(frame, resize=None, device="cuda"):
    """RT/utilities.py:182-191: cv2 BGR uint8 frame [-> cv2.resize to (width, height)] -> (3,H,W) fp32 RGB
    in [0,255], computed by the HIP frame kernel on `device` (the reference returns a CPU tensor that its
    callers `.to(device)`)."""
    _need_device(device)
    f = torch.from_numpy(_sized(frame, resize)).to(device)
    return ops.frames_to_tensor(f.unsqueeze(0), bgr=True)[0]


def _norm(x, norm, relu=False, res=None):
    return ops.instance_norm_infer(x, norm.weight, norm.bias, relu=relu, res=res, eps=norm.eps)


def _conv(block, x, relu=False, res=None):
    """Conv (RT/network.py:10-26) without its activation module: reflect pad, conv, InstanceNorm."""
    c = block.conv
    y = ops.conv2d(x, c.weight, c.bias, stride=c.stride[0], pad=block.pad_size, pad_mode="reflect")
    return _norm(y, block.norm, relu=relu, res=res)


def forward_frames(model, frames_u8, bgr=True):
    """StylizingNetwork.forward (RT/network.py:80-94) on (N,H,W,3) uint8 device frames (cv2 BGR with
    `bgr`, else RGB), down to the (N,H,W,3) uint8 frames of Inference.__iter__ (same channel order as the
    input), under no_grad, from the model's own parameters."""
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise VstError(f"frames must be (N,H,W,3) uint8, got {tuple(frames_u8.shape)}")
    H, W = frames_u8.shape[1:3]
    if H % 4 or W % 4:
        raise VstError(f"RTNSTV frames need a height and width that are multiples of 4, got {(H, W)}")
    with torch.no_grad(), ops.gemm_scope("stylizer"):
        c1 = model.conv1
        x = ops.conv_stem_u8(frames_u8, c1.conv.weight, c1.conv.bias, bgr=bgr)
        x = _norm(x, c1.norm, relu=True)
        x = _conv(model.conv2, x, relu=True)
        x = _conv(model.conv3, x, relu=True)
        for r in (model.res1, model.res2, model.res3, model.res4, model.res5):
            x = _conv(r.conv2, _conv(r.conv1, x, relu=True), res=x)
        for d in (model.deconv1, model.deconv2):
            t = d.deconv
            y = ops.conv_transpose2d(x, t.weight, t.bias, stride=t.stride[0], pad=t.padding[0],
                                     out_pad=t.output_padding[0])
            x = _norm(y, d.norm, relu=True)
        c4 = model.conv4
        if W >= 8:
            y = ops.conv_thin_fwd(x, c4.conv.weight, c4.conv.bias, reflect=True)
        else:
            y = ops.conv2d(x, c4.conv.weight, c4.conv.bias, stride=1, pad=1, pad_mode="reflect")
        return ops.instance_norm_tanh_frames(y, c4.norm.weight, c4.norm.bias, eps=c4.norm.eps, bgr=bgr)


class Inference:
    """RT/utilities.py:296-332: iterate a video, yielding stylised HxWx3 uint8 BGR frames.
    `batch_frames` (extension, default 1 = the reference's schedule) stylises that many frames per
    forward; `resize` = (width, height) as the reference's cvframe_to_tensor takes it, None = as read."""

    def __init__(self, model_class, model_path, video_path, device="cuda", batch_frames=1, resize=FRAME_RESIZE):
        _need_device(device)
        self.model = model_class().to(device)
        sd = model_path if isinstance(model_path, dict) else torch.load(model_path, weights_only=True,
                                                                       map_location=device)
        self.model.load_state_dict(sd, strict=True)
        self.model.eval()
        self.video_path = video_path
        self.device = device
        self.resize = resize
        self.batch_frames = max(1, int(batch_frames))
        self.cap = FrameSource(video_path)
        self._uploader = PinnedUploader(device, self.batch_frames)

    def __del__(self):
        cap = getattr(self, "cap", None)
        if cap is not None:
            cap.release()

    def _chunk(self):
        frames = []
        while len(frames) < self.batch_frames:
            ret, frame = self.cap.read()
            if not ret:
                break
            frames.append(_host_frame(frame, self.resize))
        return frames

    def __iter__(self):
        host = None
        while True:
            chunk = self._chunk()
            if not chunk:
                return
            frames = forward_frames(self.model, self._uploader.upload_u8(chunk), bgr=True)
            if host is None or host.shape[0] < frames.shape[0] or host.shape[1:] != frames.shape[1:]:
                host = torch.empty(tuple(frames.shape), dtype=torch.uint8, pin_memory=True)
            h = host[:frames.shape[0]]
            h.copy_(frames)
            for img in h.numpy():
                yield img.copy()
