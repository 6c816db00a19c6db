"""Evaluation metrics on the MI355X: the temporal (warping) error of RT/utilities.py:194-240 and
AA/exps_sintel.py:66-110, and SSIM / Gram distance / histogram KL / LPIPS of AA/eval.py, on the HIP
kernels of csrc/metrics.hip and csrc/lpips.hip (the LPIPS model itself is vst.lpips).  As everywhere in this package there is no CPU path: tensors on the host raise
`VstError`.  SSIM is also a differentiable score and a training loss (`ssim_scores`, `SSIMLoss`, on the fused
backward of csrc/ssim_grad.hip); the metric entries stay forward only.

Out of scope: SIFID (an InceptionV3 trunk whose weights are a download), RAFT flow
estimation, and the three grey-level histogram metrics of AA/eval.py:111-164 (OpenCV's BGR2GRAY
cannot be pinned without OpenCV).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import VstError, lib, ptr, stream

SINTEL_TAG = 202021.25  # RT/utilities.py:114


# ------------------------------------------------------------------------------------------------
# temporal error
class TemporalError:
    """Masked warping error over a sequence of frame pairs, accumulated on the device.

    Each `update` adds, for its B pairs, sum(mask * |frame_t - warp(frame_t1_to_warp, flow)|^power)
    / (C H W) to a device accumulator and B to the pair count (one fused kernel pass: the warped
    frame is never written, the sum runs in fp64 in a fixed order); nothing synchronises until
    `result()`.

    power: 2 = squared error (RT/utilities.py:235), 1 = absolute error (AA/exps_sintel.py:100).
    clamp_unit: both frames go through clamp(0, 255) / 255 first (AA/exps_sintel.py:79-83).
    convention:
      "rt": sqrt(sum over pairs of the pair's mean / pairs)   (RT/utilities.py:236-239);
      "aa": sqrt(sum over pairs of the pair's sum / (C H W)) / pairs   (AA/exps_sintel.py:100-110).
            The reference really takes the root of the SUM over pairs and then divides by the
            count -- not the root of the mean; this mirrors it.
    """

    def __init__(self, power, clamp_unit=False, convention="rt"):
        if power not in (1, 2):
            raise ValueError(f"power must be 1 or 2, got {power}")
        if convention not in ("rt", "aa"):
            raise ValueError(f"convention must be 'rt' or 'aa', got {convention}")
        self.power, self.clamp_unit, self.convention = int(power), bool(clamp_unit), convention
        self._acc = None

    def reset(self):
        self._acc = None

    def update(self, frame_t, frame_t1_to_warp, flow, mask=None, flow_hwc=False):
        """frame_t, frame_t1_to_warp: (B,C,H,W) fp32; flow: (B,2,H,W), or (B,H,W,2) with
        flow_hwc=True (a .flo payload uploaded as it is); mask: (B,H,W), broadcast over channels."""
        a = ops._check(frame_t, "frame_t", 4)
        b = ops._check(frame_t1_to_warp, "frame_t1_to_warp", 4)
        B, C, H, W = a.shape
        if b.shape != a.shape:
            raise VstError(f"temporal error: frames {tuple(a.shape)} and {tuple(b.shape)} differ")
        flo = ops._check(flow, "flow")
        want = (B, H, W, 2) if flow_hwc else (B, 2, H, W)
        if flo.dim() == 3 and B == 1:
            flo = flo.unsqueeze(0)
        if tuple(flo.shape) != want:
            raise VstError(f"temporal error: flow shape {tuple(flo.shape)} is not {want}")
        if mask is not None:
            mask = ops._check(mask, "mask")
            if mask.numel() != B * H * W or tuple(mask.shape[-2:]) != (H, W):
                raise VstError(f"temporal error: mask shape {tuple(mask.shape)} is not {(B, H, W)}")
        if self._acc is None:
            self._acc = torch.zeros(2, dtype=torch.float64, device=a.device)
        elif self._acc.device != a.device:
            raise VstError("temporal error: updates from different devices")
        ws = torch.empty(max(1, lib.vst_temporal_error_workspace(B, H, W) // 8), dtype=torch.float64, device=a.device)
        lib.vst_temporal_error(ptr(a), ptr(b), ptr(flo), ptr(mask), B, C, H, W, self.power, int(bool(flow_hwc)),
                               int(self.clamp_unit), 1.0 / (C * H * W), ws.data_ptr(), self._acc.data_ptr(), stream())
        return self

    def state(self):
        """(sum, pairs) as a 2-element float64 device tensor (no sync)."""
        if self._acc is None:
            raise VstError("temporal error: no update yet")
        return self._acc

    def result(self):
        """The scene's error as a Python float: the one host synchronisation."""
        total, pairs = self.state().tolist()
        if self.convention == "rt":
            return math.sqrt(total / pairs)
        return math.sqrt(total) / pairs


# ------------------------------------------------------------------------------------------------
# SSIM
SSIM_MAX_WINDOW = 11
SSIM_TILES = {"default": 0, "32x32": 1, "64x16": 2}


def _gauss_1d(window_size, sigma):
    """The reference's own fp32 expressions for the 1-D window (AA/eval.py:180-182)."""
    _1D = torch.linspace(-(window_size // 2), window_size // 2, window_size)
    gauss = torch.exp(-(_1D**2) / (2 * sigma**2))
    return gauss / gauss.sum()


def _ssim_call(img1, img2, taps, per_image, want_map, tile="default"):
    a = ops._check(img1, "img1", 4)
    b = ops._check(img2, "img2", 4)
    if a.shape != b.shape:
        raise VstError(f"ssim: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    B, C, H, W = a.shape
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    # the mean over images of the mean over channels is the mean over all B * C planes
    nb, nc = (B, C) if per_image else (1, B * C)
    out = torch.empty(nb, dtype=torch.float32, device=a.device)
    smap = torch.empty_like(a) if want_map else None
    ws = torch.empty(max(1, lib.vst_ssim_workspace(nb, nc, H, W) // 8), dtype=torch.float64, device=a.device)
    lib.vst_ssim(ptr(a), ptr(b), taps.ctypes.data, len(taps), nb, nc, H, W, ptr(out), ptr(smap), ws.data_ptr(),
                 SSIM_TILES[tile], stream())
    return (out if per_image else out[0]), smap


class SSIMMetric(nn.Module):
    """AA/eval.py:167-223: same constructor, same `kernel` buffer (channel x 1 x win x win, the outer
    product of the 1-D Gaussian), same `forward(img1, img2)` -- the five windowed moments, the SSIM
    map and both means in one fused kernel (`vst_ssim`), which applies the 1-D window along each axis
    (the reference's 2-D window is its outer product, so only the summation order differs).
    Odd windows up to 11."""

    def __init__(self, window_size=11, channel=3, sigma=1.5, reduction="mean"):
        super().__init__()
        if window_size % 2 != 1 or not 1 <= window_size <= SSIM_MAX_WINDOW:
            raise VstError(f"SSIMMetric: window_size must be odd and <= {SSIM_MAX_WINDOW}, got {window_size}")
        self.window_size = window_size
        self.channel = channel
        self.reduction = reduction
        gauss = _gauss_1d(window_size, sigma)
        _2D = gauss[:, None] @ gauss[None, :]
        self.register_buffer("kernel", _2D.expand(channel, 1, window_size, window_size).contiguous())
        self._taps = gauss.numpy().copy()  # host copy: a kernel argument of every launch
        self.C1 = 0.01**2
        self.C2 = 0.03**2

    def forward(self, img1, img2, return_map=False, tile="default"):
        """img1, img2: (B,C,H,W) -> the scalar mean (reduction='mean') or the (B,) per-image scores;
        return_map (extension): also the (B,C,H,W) SSIM map."""
        if img1.dim() != 4 or img1.shape != img2.shape:
            raise VstError("SSIMMetric: inputs must be [B,C,H,W] of one shape")
        if img1.shape[1] != self.channel:
            raise VstError(f"SSIMMetric: built for {self.channel} channels, got {img1.shape[1]}")
        score, smap = _ssim_call(img1, img2, self._taps, self.reduction != "mean", return_map, tile)
        return (score, smap) if return_map else score


def ssim(img1, img2, window_size=11, sigma=1.5, reduction="mean", return_map=False):
    """SSIMMetric(window_size, C, sigma, reduction)(img1, img2) without the module."""
    if window_size % 2 != 1 or not 1 <= window_size <= SSIM_MAX_WINDOW:
        raise VstError(f"ssim: window_size must be odd and <= {SSIM_MAX_WINDOW}, got {window_size}")
    score, smap = _ssim_call(img1, img2, _gauss_1d(window_size, sigma).numpy(), reduction != "mean", return_map)
    return (score, smap) if return_map else score


# ------------------------------------------------------------------------------------------------
# SSIM as a differentiable score and a training loss
def _ssim_constants(data_range):
    """C1 = (0.01 L)^2, C2 = (0.03 L)^2 as Python doubles (the C entries take them as fp32): L = 1 gives
    the metric's own constants bit for bit."""
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


class _SSIMScoresFn(torch.autograd.Function):
    """The (B,) per-image scores of `vst_ssim_c`; the backward is one `vst_ssim_bwd` launch, which
    recomputes the moments (nothing but the two images is saved) and also gives img2's gradient when
    img2 requires grad."""

    @staticmethod
    def forward(ctx, a, b, taps, c1, c2):
        B, C, H, W = a.shape
        out = torch.empty(B, dtype=torch.float32, device=a.device)
        ws = torch.empty(max(1, lib.vst_ssim_workspace(B, C, H, W) // 8), dtype=torch.float64, device=a.device)
        lib.vst_ssim_c(ptr(a), ptr(b), taps.ctypes.data, len(taps), B, C, H, W, c1, c2, ptr(out), None, ws.data_ptr(),
                       SSIM_TILES["default"], stream())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, b)
        ctx.args = (taps, c1, c2)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        a, b = ctx.saved_tensors
        taps, c1, c2 = ctx.args
        B, C, H, W = a.shape
        d1 = torch.empty_like(a)
        d2 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        lib.vst_ssim_bwd(ptr(a), ptr(b), taps.ctypes.data, len(taps), B, C, H, W, c1, c2, ptr(g.contiguous()), ptr(d1),
                         ptr(d2), stream())
        return (d1 if ctx.needs_input_grad[0] else None), d2, None, None, None


def ssim_scores(img1, img2, window_size=11, sigma=1.5, data_range=1.0):
    """The (B,) per-image SSIM of two (B,C,H,W) fp32 device tensors with values in [0, data_range],
    differentiable in img1 and -- when it requires grad -- in img2 (one fused backward kernel,
    `vst_ssim_bwd`, for both).  `SSIMMetric` / `ssim` stay the forward-only metric; with data_range = 1
    the scores here are theirs bit for bit.  Nothing is recorded when neither input requires grad or
    grad mode is off."""
    if window_size % 2 != 1 or not 1 <= window_size <= SSIM_MAX_WINDOW:
        raise VstError(f"ssim_scores: window_size must be odd and <= {SSIM_MAX_WINDOW}, got {window_size}")
    a = ops._check(img1, "img1", 4)
    b = ops._check(img2, "img2", 4)
    if a.shape != b.shape:
        raise VstError(f"ssim_scores: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    taps = np.ascontiguousarray(_gauss_1d(window_size, sigma).numpy(), dtype=np.float32)
    c1, c2 = _ssim_constants(data_range)
    return _SSIMScoresFn.apply(a, b, taps, c1, c2)


class _SSIMLossFn(torch.autograd.Function):
    """weight * (1 - mean_b score[b]) as a 0-d tensor (`vst_ssim_loss` / `vst_ssim_loss_bwd`)."""

    @staticmethod
    def forward(ctx, score, weight):
        out = torch.empty((), dtype=torch.float32, device=score.device)
        lib.vst_ssim_loss(ptr(score), score.numel(), float(weight), ptr(out), stream())
        ctx.args = (score.numel(), float(weight))
        return out

    @staticmethod
    def backward(ctx, g):
        B, weight = ctx.args
        gl = torch.empty(B, dtype=torch.float32, device=g.device)
        lib.vst_ssim_loss_bwd(ptr(g.contiguous()), B, weight, ptr(gl), stream())
        return gl, None


class SSIMLoss(nn.Module):
    """SSIM as a training-loss term over what the trainers hold (fp32 planes in [0, data_range], 255
    by default): `set_target(frames)` keeps the target (a video trainer's content frame, or the warped
    previous output); `forward(pred)` returns `weight * (1 - mean_b SSIM(pred, target)_b)` as a 0-d
    tensor, differentiable in pred, which composes with `ops.sum_scalars`."""

    def __init__(self, window_size=11, sigma=1.5, data_range=255.0, weight=1.0):
        super().__init__()
        if window_size % 2 != 1 or not 1 <= window_size <= SSIM_MAX_WINDOW:
            raise VstError(f"SSIMLoss: window_size must be odd and <= {SSIM_MAX_WINDOW}, got {window_size}")
        self.window_size, self.sigma = int(window_size), float(sigma)
        self.data_range, self.weight = float(data_range), float(weight)
        self.target = None

    def set_target(self, frames):
        self.target = ops._check(frames, "frames", 4).detach()
        return self

    def forward(self, pred):
        if self.target is None:
            raise VstError("SSIMLoss: set_target(frames) first")
        p = ops._check(pred, "pred", 4)
        if p.shape != self.target.shape:
            raise VstError(f"SSIMLoss: pred {tuple(p.shape)} does not match the target's {tuple(self.target.shape)}")
        score = ssim_scores(p, self.target, self.window_size, self.sigma, self.data_range)
        return _SSIMLossFn.apply(score, self.weight)


# ------------------------------------------------------------------------------------------------
# Gram distance
GRAM_FEATURES = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")


def gram_distance(vgg19, img, style):
    """AA/eval.py:78-108 without the file reads: the mean over relu1_1 .. relu5_1 of
    mse(gram(vgg19(img)) , gram(vgg19(style))), gram = F F^T / (H W).  img, style: (N,3,H,W) fp32
    RGB in [0, 255] on the device; returns a 0-d device tensor.  Existing kernels only (the VGG19
    forward, vst_gram, vst_mse_fwd)."""
    with torch.no_grad():
        fcs, fs = vgg19(img), vgg19(style)
        terms = [ops.mse(ops.gram_matrix(fcs[k], per_hw=True), ops.gram_matrix(fs[k], per_hw=True),
                         1.0 / len(GRAM_FEATURES)) for k in GRAM_FEATURES]
        return ops.sum_scalars(*terms)


# ------------------------------------------------------------------------------------------------
# LPIPS
def lpips_distance(model, img0_u8, img1_u8, bgr=True):
    """AA/eval.py:26-30 / AA/exps_image.py's lpips columns on N pairs at once: (N,H,W,3) uint8 device
    frames (bgr: cv2's order) -> the (N,) distances of `model` (a vst.lpips.LPIPS), no host sync."""
    return model.forward_u8(img0_u8, img1_u8, bgr=bgr).reshape(-1)


class LPIPSMean:
    """The mean LPIPS distance over a folder of pairs, accumulated on the device: `update` adds the
    distances of its N pairs to a device accumulator (vst_sum_scaled, vst_sum4) and N to the pair count;
    nothing synchronises until `result()`.  The accumulator is fp32 (the library's sum entries are),
    unlike TemporalError's fp64 one: each update adds about 2^-24 relative, which is fine for folders of
    thousands of pairs and not meant for millions.  The model must give one distance per pair
    (spatial=False)."""

    def __init__(self, model, bgr=True):
        self.model, self.bgr = model, bool(bgr)
        self.reset()

    def reset(self):
        self._acc, self._pairs = None, 0

    def update(self, img0_u8, img1_u8):
        if getattr(self.model, "spatial", False):
            raise VstError("LPIPSMean: the model must return one distance per pair (spatial=False)")
        d = lpips_distance(self.model, img0_u8, img1_u8, bgr=self.bgr)
        if d.numel() != img0_u8.shape[0]:
            raise VstError(f"LPIPSMean: {d.numel()} distances for {img0_u8.shape[0]} pairs")
        if self._acc is None:
            self._acc = torch.zeros(1, dtype=torch.float32, device=d.device)
        elif self._acc.device != d.device:
            raise VstError("LPIPSMean: updates from different devices")
        ws = torch.empty(ops.LOSS_WS, dtype=torch.float32, device=d.device)
        part = torch.empty(3, dtype=torch.float32, device=d.device)
        lib.vst_sum_scaled(ptr(d), d.numel(), 1.0, ptr(ws), ptr(part), stream())
        ops.sum_into(self._acc, [self._acc, part[:1]])
        self._pairs += d.numel()
        return self

    def state(self):
        """(device sum (1,), pairs) (no sync)."""
        if self._acc is None:
            raise VstError("LPIPSMean: no update yet")
        return self._acc, self._pairs

    def result(self):
        """The mean as a Python float: the one host synchronisation."""
        acc, pairs = self.state()
        return acc.item() / pairs


# ------------------------------------------------------------------------------------------------
# histograms / KL
def histogram_u8(images):
    """(N,H,W,C) uint8 on the device (C = 1 or 3) -> (N,C,256) int32 counts, np.bincount per image
    and channel (compute_histogram, AA/eval.py:38-46, without its + 1)."""
    if images.dim() == 3:
        images = images.unsqueeze(-1)
    if images.dim() != 4 or images.shape[-1] not in (1, 3):
        raise VstError(f"histogram: images must be (N,H,W,C) uint8 with C = 1 or 3, got {tuple(images.shape)}")
    N, H, W, C = images.shape
    hist = torch.empty((N, C, 256), dtype=torch.int32, device=images.device)
    lib.vst_hist_u8(ops._ptr_u8(images, "images"), hist.data_ptr(), N, H, W, C, stream())
    return hist


def _entropy(pk, qk):
    """scipy.stats.entropy(pk, qk) in float64: both normalised to sum 1, then sum(rel_entr(pk, qk))."""
    pk = np.asarray(pk, dtype=np.float64)
    qk = np.asarray(qk, dtype=np.float64)
    pk = pk / np.sum(pk, axis=0, keepdims=True)
    qk = qk / np.sum(qk, axis=0, keepdims=True)
    return float(np.sum(pk * np.log(pk / qk), axis=0))  # (every bin is >= 1 count: no 0 log 0 case)


def kl_divergence(img_u8, style_u8):
    """AA/eval.py:49-67 on (H,W,3) uint8 device images (they may differ in size): per channel
    entropy(hist(img) + 1, hist(style) + 1), averaged.  The histograms come from `vst_hist_u8`; the
    + 1 smoothing and the 768-number entropy stay on the host in float64."""
    hi = histogram_u8(img_u8.unsqueeze(0) if img_u8.dim() == 3 else img_u8)
    hs = histogram_u8(style_u8.unsqueeze(0) if style_u8.dim() == 3 else style_u8)
    if hi.shape[0] != 1 or hs.shape[0] != 1 or hi.shape[1] != 3 or hs.shape[1] != 3:
        raise VstError("kl_divergence: one (H,W,3) image each")
    hi, hs = hi[0].cpu().numpy().astype(np.int64) + 1, hs[0].cpu().numpy().astype(np.int64) + 1
    return sum(_entropy(hi[c], hs[c]) for c in range(3)) / 3.0


# ------------------------------------------------------------------------------------------------
# files
def read_sintel_flow(path):
    """RT/utilities.py:113-152: a Middlebury / Sintel .flo file -> (H,W,2) float32, with the
    reference's errors.  Upload the array as it is and pass `flow_hwc=True`."""
    path = os.fspath(path)
    raw = np.fromfile(path, dtype=np.uint8)
    tag = raw[:4].view("<f4")[0] if raw.size >= 4 else None
    if tag != np.float32(SINTEL_TAG):
        raise ValueError(f"ReadFlowFile({path}): wrong tag (possibly due to big-endian machine?)")
    if raw.size < 12:
        raise ValueError(f"ReadFlowFile({path}): file is too short")
    width, height = (int(v) for v in raw[4:12].view("<i4"))
    if width < 1 or width > 99999:
        raise ValueError(f"ReadFlowFile({path}): illegal width {width}")
    if height < 1 or height > 99999:
        raise ValueError(f"ReadFlowFile({path}): illegal height {height}")
    need = 12 + height * width * 2 * 4
    if raw.size < need:
        raise ValueError(f"ReadFlowFile({path}): file is too short")
    if raw.size > need:
        raise ValueError(f"ReadFlowFile({path}): file is too long")
    return raw[12:].view("<f4").reshape(height, width, 2).astype(np.float32, copy=True)


def imread(path, gray=False):
    """cv2.imread(path[, cv2.IMREAD_GRAYSCALE]): (H,W,3) uint8 BGR, or (H,W) uint8.  cv2 when it is
    importable, Pillow otherwise (a PNG decodes to the same bytes; BGR is the reversed RGB)."""
    path = os.fspath(path)
    try:
        import cv2  # noqa: PLC0415
    except ImportError:
        cv2 = None
    if cv2 is not None and hasattr(cv2, "imread"):
        img = cv2.imread(path, cv2.IMREAD_GRAYSCALE) if gray else cv2.imread(path)
        if img is None:
            raise FileNotFoundError(path)
        return img
    from PIL import Image  # noqa: PLC0415

    with Image.open(path) as im:
        if gray:
            return np.asarray(im.convert("L"))
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
