"""CPU restatement of the reference's evaluation metrics, for the tests of vst.metrics.

TEST INFRASTRUCTURE ONLY.  Written from the formulas (RT/utilities.py:59-77, 194-240,
AA/exps_sintel.py:79-110, AA/eval.py:38-108, 167-223) on torch-CPU / numpy in a chosen dtype: float32
is the reference's own arithmetic (torch `grid_sample`, `conv2d`, `mean`), float64 is the yardstick
the GPU tests measure both against.  tests/golden/eval_metrics.npz (gen_golden_eval.py) pins it to
the reference's own outputs (tests/test_metrics_ref.py).  Also the shared synthetic inputs and the
file writers (.flo, PNG, the Sintel folder layout) that the generator and the tests both use.
"""
import os
import struct

import numpy as np
import torch
import torch.nn.functional as F

SINTEL_TAG = 202021.25


# ------------------------------------------------------------------------------------------------
# temporal error
def warp(x, flo):
    """Bilinear warp of x (B,C,H,W) by flo (B,2,H,W): grid normalised by W-1 / H-1, sampled with
    align_corners=False and zeros padding."""
    B, C, H, W = x.shape
    xx = torch.arange(W, dtype=x.dtype).view(1, 1, 1, W).expand(B, 1, H, W)
    yy = torch.arange(H, dtype=x.dtype).view(1, 1, H, 1).expand(B, 1, H, W)
    v = torch.cat((xx, yy), 1) + flo
    gx = 2.0 * v[:, 0] / max(W - 1, 1) - 1.0
    gy = 2.0 * v[:, 1] / max(H - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((gx, gy), dim=3), mode="bilinear", padding_mode="zeros", align_corners=False)


def temporal_map(a, b, flo, mask, power, clamp_unit):
    """mask * |a - warp(b, flo)|^power, (B,C,H,W); mask (B,H,W) or None."""
    if clamp_unit:
        a, b = a.clamp(0, 255) / 255.0, b.clamp(0, 255) / 255.0
    d = a - warp(b, flo)
    d = d * d if power == 2 else d.abs()
    return d if mask is None else mask.unsqueeze(1) * d


def temporal_pair_sum(a, b, flo, mask, power, clamp_unit, dtype, mean=False):
    """One update's contribution: sum of the map / (C H W) (`mean`: the reference's `.mean()` form,
    the same number for B = 1), as a Python float computed in `dtype`."""
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    m = temporal_map(cast(a), cast(b), cast(flo), cast(mask), power, clamp_unit)
    if mean:
        return m.mean().item() * a.shape[0]
    return (m.sum() / (a.shape[1] * a.shape[2] * a.shape[3])).item()


def temporal_error(pairs, power, clamp_unit, convention, dtype, mean=None):
    """pairs: iterable of (a, b, flo, mask) with flo planar (B,2,H,W).  "rt": sqrt(sum / pairs) of
    the pairs' means; "aa": sqrt(sum of the pairs' sums / (C H W)) / pairs."""
    mean = convention == "rt" if mean is None else mean
    total, n = 0.0, 0
    for a, b, flo, mask in pairs:
        total += temporal_pair_sum(a, b, flo, mask, power, clamp_unit, dtype, mean=mean)
        n += a.shape[0]
    return float(np.sqrt(total / n)) if convention == "rt" else float(np.sqrt(total)) / n


# ------------------------------------------------------------------------------------------------
# SSIM
def gauss_window(window_size, sigma):
    """The fp32 window values: linspace, exp, normalise, outer product (channel-independent)."""
    x = torch.linspace(-(window_size // 2), window_size // 2, window_size)
    g = torch.exp(-(x**2) / (2 * sigma**2))
    g = g / g.sum()
    return g, g[:, None] @ g[None, :]


def ssim_map(img1, img2, window_size=11, sigma=1.5, dtype=torch.float32):
    """The SSIM map (B,C,H,W) in `dtype` from the fp32 2-D window: five zero-padded depthwise
    windows, C1 = 0.01^2, C2 = 0.03^2."""
    C = img1.shape[1]
    k = gauss_window(window_size, sigma)[1].to(dtype).expand(C, 1, window_size, window_size).contiguous()
    a, b = img1.to(dtype), img2.to(dtype)
    conv = lambda t: F.conv2d(t, k, padding=window_size // 2, groups=C)  # noqa: E731
    C1, C2 = 0.01**2, 0.03**2
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def ssim(img1, img2, window_size=11, sigma=1.5, dtype=torch.float32, reduction="none"):
    per_image = ssim_map(img1, img2, window_size, sigma, dtype).mean(dim=[2, 3]).mean(dim=1)
    return per_image.mean() if reduction == "mean" else per_image


SSIM_SHAPES = [(1, 3, 11, 11), (2, 3, 13, 37), (1, 1, 40, 70), (1, 1, 33, 65)]
SSIM_KINDS = ("u255", "unit")


def ssim_inputs(shape, kind, seed):
    """A uniform-noise image (integers in [0,255], or reals in [0,1]) and the same plus Gaussian
    noise of 20 % of the range, clipped; float32 (B,C,H,W)."""
    rng = np.random.default_rng(seed)
    top = 255.0 if kind == "u255" else 1.0
    x = rng.integers(0, 256, size=shape).astype(np.float64) if kind == "u255" else rng.random(shape)
    y = np.clip(x + 0.2 * top * rng.standard_normal(shape), 0.0, top)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))


def ssim_cases():
    """(key, shape, kind, seed) of the parity set: every shape in both value ranges."""
    return [(f"ssim_{i}_{kind}", shape, kind, 100 + 10 * i + j)
            for i, shape in enumerate(SSIM_SHAPES) for j, kind in enumerate(SSIM_KINDS)]


# ------------------------------------------------------------------------------------------------
# Gram distance, histogram KL
def to255(u8_hwc_rgb):
    """toTensor255 of an (H,W,3) uint8 array: x / 255 * 255 in fp32, (1,3,H,W)."""
    t = torch.from_numpy(np.ascontiguousarray(u8_hwc_rgb.transpose(2, 0, 1)))
    return t.float().div(255).mul(255).unsqueeze(0)


def gram_distance(VP, img, style, dtype=torch.float32):
    """Mean over relu1_1 .. relu5_1 of mse(gram / HW) with VGG19 parameters VP (oracle.adaattn_ref)."""
    from oracle import adaattn_ref as A  # noqa: PLC0415

    VP = {k: v.to(dtype) for k, v in VP.items()}
    with torch.no_grad():
        fa, fb = A.vgg19(VP, img.to(dtype), dtype), A.vgg19(VP, style.to(dtype), dtype)
        loss = 0.0
        for k in ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1"):
            grams = []
            for f in (fa[k], fb[k]):
                b, ch, h, w = f.shape
                feat = f.reshape(b, ch, h * w)
                grams.append(feat.bmm(feat.transpose(1, 2)) / (h * w))
            loss = loss + F.mse_loss(grams[0], grams[1])
    return loss.item() / 5.0


def histograms(img_u8):
    """(H,W,C) uint8 -> (C,256) counts."""
    return np.stack([np.bincount(img_u8[:, :, c].reshape(-1), minlength=256) for c in range(img_u8.shape[2])])


def kl(img_u8, style_u8):
    """Mean over the 3 channels of KL(hist(img) + 1 || hist(style) + 1), both normalised, float64."""
    total = 0.0
    for c in range(3):
        p = (histograms(img_u8)[c] + 1).astype(np.float64)
        q = (histograms(style_u8)[c] + 1).astype(np.float64)
        p, q = p / p.sum(), q / q.sum()
        total += float(np.sum(p * np.log(p / q)))
    return total / 3.0


# ------------------------------------------------------------------------------------------------
# files
def write_flo(path, flow):
    """(H,W,2) float32 -> a Middlebury / Sintel .flo file."""
    flow = np.ascontiguousarray(flow, dtype="<f4")
    with open(path, "wb") as f:
        f.write(struct.pack("<f", SINTEL_TAG))
        f.write(struct.pack("<ii", flow.shape[1], flow.shape[0]))
        f.write(flow.tobytes())


def write_png(path, arr_bgr_or_gray):
    """cv2.imwrite of a uint8 array: (H,W,3) BGR or (H,W) grey, lossless PNG."""
    from PIL import Image  # noqa: PLC0415

    a = np.asarray(arr_bgr_or_gray)
    Image.fromarray(np.ascontiguousarray(a[..., ::-1]) if a.ndim == 3 else a).save(path, format="PNG")


def read_png(path, gray=False):
    """cv2.imread: (H,W,3) uint8 BGR, or (H,W) with gray."""
    from PIL import Image  # noqa: PLC0415

    with Image.open(path) as im:
        return np.asarray(im.convert("L")) if gray else np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def write_sintel_scene(root, scene, frames_bgr, occlusions, flows):
    """The MPI-Sintel-complete layout under `root`: training/final|occlusions|flow/<scene>/frame_NNNN."""
    for sub in ("final", "occlusions", "flow"):
        os.makedirs(os.path.join(root, "training", sub, scene), exist_ok=True)
    for i, f in enumerate(frames_bgr):
        write_png(os.path.join(root, "training", "final", scene, f"frame_{i + 1:04d}.png"), f)
    for i, (o, fl) in enumerate(zip(occlusions, flows)):
        write_png(os.path.join(root, "training", "occlusions", scene, f"frame_{i + 1:04d}.png"), o)
        write_flo(os.path.join(root, "training", "flow", scene, f"frame_{i + 1:04d}.flo"), fl)


SCENES = {"scene_a": (4, 32, 64, 311), "scene_b": (3, 36, 60, 322)}  # frames, H, W, seed


def sintel_scene(name):
    """Synthetic scene: BGR uint8 frames (T,H,W,3), occlusion maps (T-1,H,W) with about 30 % of the
    pixels occluded (255), flows (T-1,H,W,2) of a few pixels that leave the frame along the right and
    top edges."""
    from vst.synthetic import video_frames  # noqa: PLC0415

    T, H, W, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    frames = video_frames(seed, T, H, W)
    occ = np.where(rng.random((T - 1, H, W)) < 0.3, 255, 0).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flows = np.empty((T - 1, H, W, 2), dtype=np.float32)
    for t in range(T - 1):
        flows[t, ..., 0] = 2.75 + 1.5 * np.sin(0.21 * yy + 0.13 * xx + t) + 0.25 * rng.standard_normal((H, W))
        flows[t, ..., 1] = -1.5 + 1.25 * np.cos(0.17 * xx - 0.11 * yy + t) + 0.25 * rng.standard_normal((H, W))
    return frames, occ, flows
