"""MI355X AdaAttN inference: drop-in for the flows of AA/infer_video.py and AA/infer_image.py.

Per frame the reference runs `cv2_to_tensor` -> VGG19 -> `StylizingNetwork(fc, fs)` -> `clamp(0, 255)`
-> HWC -> `astype(uint8)` (AA/infer_video.py:54-68) with the style's VGG features `fs` computed once.
`StylizingNetwork.forward` still recomputes, per frame, everything else that depends on the style
alone.  Here:
  * `encode_style` runs the style side ONCE -- VGG, `feature_down_sample`, IN, the g / h 1x1 convs
    and, per attention level, for cosine attention G = Kh U^T, ksum, us (all the linear form reads
    from the style, attention.py) or for softmax K and [V; V^2] -- and keeps only that (`StyleState`);
  * `stylize` runs the content side with the same helpers `LinearCosineAttnFn.forward` /
    `AdaAttnFn.forward` are made of, so its attention output is bitwise the training forward's, then
    the decoder; its last conv (64 -> 3) runs on the thin VALU forward (`ops.conv_thin_fwd`), which
    can write the clamped, truncated uint8 HWC frame in the same pass;
  * everything runs under `torch.no_grad()`: no autograd Functions' saved tensors, no side streams.
`VideoInference` reads frames like `vst.reconet.inference.Inference` (a path through
cv2.VideoCapture, or in-memory cv2-style BGR frames), stages `batch_frames` of them in pinned memory
per upload and yields HxWx3 uint8 RGB frames (the reference's `frames` list; `bgr=True` for cv2).
"""
import os

import numpy as np
import torch

from .. import ops
from .._lib import VstError, lib, ptr, stream
from ..video_io import FrameSource, PinnedUploader, host_frame
from . import attention as A
from .attention import COSINE, SOFTMAX, instance_norm_plain
from .network import StylizingNetwork
from .utilities import feature_down_sample
from .vgg19 import VGG19


class StyleState:
    """What the content side needs from `Nk` styles, per attention level: cosine (G [Nk][d][2dv],
    ksum [Nk][d], us [Nk][2dv], Ns); softmax (K [Nk][d][Ns], VV2 [Nk][2dv][Ns]).  Nothing else is
    kept -- no VGG features of the style.  Frame n of a batch uses style n % Nk."""

    def __init__(self, activation, levels):
        self.activation, self.levels = activation, levels

    @property
    def num_styles(self):
        return self.levels[0][0].shape[0]

    def tensors(self):
        return [t for lv in self.levels for t in lv if torch.is_tensor(t)]


def _activation(model):
    return model.adaattn[0].activation.kind


def style_level(K, V, activation):
    """One level of a StyleState from the projected style features K (Nk,d,hs,ws), V (Nk,dv,hs,ws)."""
    K, V = ops._check(K, "adaattn operand", 4), ops._check(V, "adaattn operand", 4)
    Nk, d, hs, ws = K.shape
    if V.shape[0] != Nk or V.shape[2:] != K.shape[2:]:
        raise VstError(f"adaattn: K{tuple(K.shape)} V{tuple(V.shape)}")
    if activation == COSINE:
        _, _, _, G, ksum, us = A.cosine_style_side(K, V)
        return (G, ksum, us, hs * ws)
    if activation == SOFTMAX:
        return (K.view(Nk, d, hs * ws), A.square_concat(V))
    raise ValueError(f"Unknown activation function: {activation}")


def attend(level, activation, Q, cn):
    """`adaattn(Q, K, V, cn)` from a cached style level: the content side only."""
    Q, cn = ops._check(Q, "adaattn operand", 4), ops._check(cn, "adaattn operand", 4)
    Nq, d, h, w = Q.shape
    Nk = level[0].shape[0]
    if level[0].shape[1] != d or cn.shape[0] != Nq or cn.shape[2:] != Q.shape[2:] or Nq % Nk:
        raise VstError(f"adaattn: Q{tuple(Q.shape)} c{tuple(cn.shape)} over {Nk} cached styles of {level[0].shape[1]} channels")
    if activation == COSINE:
        G, ksum, us, Ns = level
        qn, _, Qh = A.cosine_query_side(Q)
        return A.cosine_content_side(Q, qn, Qh, cn, G, ksum, us, Ns)[0]
    K, VV2 = level
    r = Nq // Nk
    MV, _, _ = A.softmax_moments(Q.view(Nq, d, h * w), A._repeat(K, r), A._repeat(VV2, r))
    out = torch.empty((Nq, cn.shape[1], h, w), device=Q.device, dtype=torch.float32)
    lib.vst_adaattn_out(ptr(MV), ptr(cn), ptr(out), Nq, cn.shape[1] * h * w, stream())
    return out


def encode_style(vgg, model, style):
    """style (Nk,3,H,W) fp32 RGB in [0,255] on the device -> StyleState."""
    act = _activation(model)
    with torch.no_grad():
        fs = list(vgg(style).values())
        levels = []
        with ops.gemm_scope("stylizer"):
            for i in range(3):
                idx = i + 2
                K, V = model.adaattn[i].key_value(fs[idx], feature_down_sample(fs, idx))
                levels.append(style_level(K, V, act))
    return StyleState(act, levels)


THIN_FWD = os.environ.get("VST_THIN_FWD", "1") != "0"  # A/B: the last conv on the thin VALU forward


def _thin_ok(x):
    return THIN_FWD and x.shape[2] >= 2 and x.shape[3] >= 8 and x.shape[3] % 4 == 0


def stylize(vgg, model, state, content, frames=None, bgr=False):
    """content (N,3,H,W) fp32 RGB in [0,255] -> the stylised image: fp32 (N,3,H,W), or, when `frames`
    ((N,H,W,3) uint8) is given, the clamped, truncated frames written by the last conv itself (RGB;
    bgr: BGR)."""
    with torch.no_grad():
        fc = list(vgg(content).values())
        with ops.gemm_scope("stylizer"):
            outs = []
            for i in range(3):
                idx = i + 2
                m = model.adaattn[i]
                Q = m.query(feature_down_sample(fc, idx))
                outs.append(attend(state.levels[i], state.activation, Q, instance_norm_plain(fc[idx])))
            dec = model.decoder
            with ops.gemm_scope("dec"):
                x = dec.trunk(outs[2], outs[1], outs[0])
                c8 = dec.conv8.conv
                if _thin_ok(x):
                    return ops.conv_thin_fwd(x, c8.weight, c8.bias, reflect=True, frames=frames, bgr=bgr)
                # (the A/B route: the GEMM forward, then the frame kernel)
                y = dec.conv8.run(x)
                return y if frames is None else ops.tensor_to_frames(y, bgr=bgr, frames=frames)


# ---------------------------------------------------------------------------------------------
# inputs
def _load_picture(p):
    from PIL import Image  # noqa: PLC0415

    return np.asarray(Image.open(os.fspath(p)).convert("RGB"))


def image_tensor(img, size, device="cuda"):
    """A path, a PIL image or a (H,W,3) uint8 RGB array -> (1,3,H,W) fp32 in [0,255] resized to
    size = (H, W) exactly as `toTensor255(img.resize((W, H), Image.BILINEAR))` (Pillow's 8-bit
    resampler, on the device); a ready (1,3,H,W) tensor is taken as it is."""
    if torch.is_tensor(img):
        if img.dim() != 4 or img.shape[1] != 3:
            raise VstError(f"image tensor must be (N,3,H,W), got {tuple(img.shape)}")
        return img.detach().to(device=device, dtype=torch.float32).contiguous()
    if isinstance(img, (str, bytes)) or hasattr(img, "__fspath__"):
        img = _load_picture(img)
    elif not isinstance(img, np.ndarray):
        img = np.asarray(img.convert("RGB"))  # PIL image
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise VstError(f"images must be HxWx3 uint8 RGB, got {img.dtype} {img.shape}")
    dev = torch.from_numpy(np.array(img, copy=True)).to(device).unsqueeze(0)
    return ops.pil_resize_to_tensor255(dev, (size[1], size[0]))


def load_model(model, activation="cosine", device="cuda"):
    """A StylizingNetwork, a state dict or a checkpoint path -> the network on `device` (eval)."""
    if isinstance(model, torch.nn.Module):
        if _activation(model) != activation:
            raise VstError(f"the model's activation is {_activation(model)}, not {activation}")
        return model.to(device).eval()
    net = StylizingNetwork(activation=activation).to(device)
    sd = model if isinstance(model, dict) else torch.load(model, weights_only=True, map_location=device)
    net.load_state_dict(sd, strict=True)
    return net.eval()


def load_vgg(vgg, device="cuda"):
    """A VGG19 module, a state dict in its layout, or a torchvision weights path / None (VGG19(weights))."""
    if isinstance(vgg, torch.nn.Module):
        return vgg.to(device).eval()
    if isinstance(vgg, dict):
        net = VGG19()
        net.load_state_dict(vgg, strict=True)
        return net.to(device).eval()
    return VGG19(weights=vgg).to(device).eval()


class VideoInference:
    """AA/infer_video.py:30-69 as an iterator of stylised HxWx3 uint8 frames (RGB, the reference's
    `frames` list; `bgr=True`: BGR for cv2 display).  `video`: a path (cv2.VideoCapture) or in-memory
    cv2-style BGR frames ((T,H,W,3) uint8 array or an iterable); frames not at `size` = (H, W) are
    resized on the host with cv2 INTER_AREA like the reference's `cv2_to_tensor(frame, resize=(W, H))`
    (ImportError without cv2).  `style`: a path, a PIL image, a (H,W,3) uint8 RGB array (resized to
    `size` Pillow-exactly) or a ready (Nk,3,H,W) tensor.  `vgg` (extension): the encoder -- a VGG19
    module, its state dict, or a torchvision weights path.  `batch_frames` (extension, default 1 = the
    reference's schedule) stylises that many frames per forward."""

    def __init__(self, model_path_or_state_dict, style, video, activation="cosine", size=(256, 512), device="cuda",
                 batch_frames=1, bgr=False, vgg=None):
        self.device, self.size, self.bgr = device, tuple(size), bool(bgr)
        self.B = max(1, int(batch_frames))
        self.model = load_model(model_path_or_state_dict, activation, device)
        self.vgg = load_vgg(vgg, device)
        self.state = encode_style(self.vgg, self.model, image_tensor(style, self.size, device))
        self.cap = FrameSource(video)
        self._uploader = PinnedUploader(device, self.B)

    def __del__(self):
        cap = getattr(self, "cap", None)
        if cap is not None:
            cap.release()

    def _chunks(self):
        while True:
            new = []
            while len(new) < self.B:
                ret, frame = self.cap.read()
                if not ret:
                    break
                new.append(host_frame(frame, self.size, "INTER_AREA"))
            if not new:
                return
            yield self._uploader.upload(new, bgr=True)  # cv2 BGR -> RGB planes (cv2_to_tensor)
            if len(new) < self.B:
                return

    def __iter__(self):
        host = None
        Nk = self.state.num_styles
        for c in self._chunks():
            k = c.shape[0]
            if k % Nk:
                raise VstError(f"a chunk of {k} frames over {Nk} styles (frame n uses style n % {Nk})")
            frames = torch.empty((k,) + tuple(c.shape[2:]) + (3,), dtype=torch.uint8, device=c.device)
            stylize(self.vgg, self.model, self.state, c, frames=frames, bgr=self.bgr)
            if host is None or host.shape[0] < k or host.shape[1:] != frames.shape[1:]:
                host = torch.empty((max(k, self.B),) + tuple(frames.shape[1:]), dtype=torch.uint8, pin_memory=True)
            h = host[:k]
            h.copy_(frames)
            for img in h.numpy():
                yield img.copy()


def stylize_image(model, vgg, content, style, activation="softmax", size=(256, 256), device="cuda"):
    """AA/infer_image.py:56-68: content and style (each a path, PIL image, (H,W,3) uint8 RGB array
    or ready tensor; pictures are resized to `size` Pillow-exactly) -> (the stylised image clamped
    to [0, 255], fp32 (1,3,H,W); the same as an HxWx3 uint8 RGB array, the reference's `.byte()`)."""
    model, vgg = load_model(model, activation, device), load_vgg(vgg, device)
    c, s = image_tensor(content, size, device), image_tensor(style, size, device)
    state = encode_style(vgg, model, s)
    cs = stylize(vgg, model, state, c)
    clamped = torch.empty_like(cs)
    u8 = ops.tensor_to_frames(cs, bgr=False, clamped=clamped)
    return clamped, u8[0].cpu().numpy()
