"""CPU restatement of LPIPS (VGG), for the tests of vst.lpips and csrc/lpips.hip.

TEST INFRASTRUCTURE ONLY.  Written from the formulas (AA/lpips/__init__.py:13-15, 86-88,
AA/lpips/lpips.py:129-171, AA/lpips/pretrained_networks.py:98-136):
  * `head64`: the distance head in float64 -- per pixel na = sqrt(sum a^2), nb likewise,
    d = sum_c w_c (a_c / (na + 1e-10) - b_c / (nb + 1e-10))^2, layer = mean over the pixels -- the yardstick;
  * `head32`: the reference's own fp32 op sequence on torch-CPU for the same features (square, channel
    sum, sqrt, add, divide, subtract, square, 1x1 conv or channel sum, spatial mean);
  * `trunk`: torchvision VGG16 features[0:30] as plain F.conv2d / max_pool2d in fp32 with the seeded
    weights (`trunk_params`), returning relu1_2 .. relu5_3;
  * the input builders (`im2tensor`, `scaling`, the image pairs of the golden fixture, the head's
    adversarial feature maps).
tests/golden/lpips_vgg.npz (gen_golden_lpips.py) pins it to the reference's own outputs
(tests/test_lpips_ref.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.seeding import seeded_arrays

EPS = 1e-10
CHNS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchvision vgg16.features indices of the convolutions of each LPIPS slice; slices 2..5 start with a pool
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
_WIDTHS = (64, 128, 256, 512, 512)

TRUNK_SEED = 511
# key: (N, H, W, seed) of the fixture's uint8 image pairs
PAIRS = {"p16": (1, 16, 16, 521), "p32": (2, 32, 48, 522), "p36": (1, 36, 60, 523)}
NOISE = 24  # the second image of a pair: the first plus integer noise in [-NOISE, NOISE], clipped


# ------------------------------------------------------------------------------------------------
# the head
def head64(f0, f1, w=None):
    """f0, f1: (N,C,h,w); w: (C,) or None (ones).  -> (layer (N,), map (N,h,w)) in float64."""
    a, b = f0.to(torch.float64), f1.to(torch.float64)
    na = a.pow(2).sum(dim=1, keepdim=True).sqrt()
    nb = b.pow(2).sum(dim=1, keepdim=True).sqrt()
    d = (a / (na + EPS) - b / (nb + EPS)).pow(2)
    if w is not None:
        d = d * w.to(torch.float64).view(1, -1, 1, 1)
    m = d.sum(dim=1)
    return m.mean(dim=[1, 2]), m


def _normalize32(t):
    return t / (torch.sqrt(torch.sum(t**2, dim=1, keepdim=True)) + EPS)


def head32(f0, f1, w=None):
    """The reference's fp32 sequence.  -> (layer (N,), map (N,h,w)) in float32."""
    diff = (_normalize32(f0) - _normalize32(f1)) ** 2
    m = diff.sum(dim=1, keepdim=True) if w is None else F.conv2d(diff, w.view(1, -1, 1, 1))
    return m.mean([2, 3]).reshape(-1), m[:, 0]


HEAD_SHAPES = [(2, 64, 7, 9), (1, 512, 1, 1), (2, 512, 2, 3), (1, 128, 16, 64), (1, 256, 5, 4)]


def head_inputs(shape, seed=0):
    """Non-negative features (a ReLU output's) and learned-weight-like w >= 0, with -- where the plane
    has the pixels for it -- a pixel that is all-zero in f0 only (pixel 0), one all-zero in both (1), one
    of magnitude 1e4 (2) and one whose norm is near eps, values ~1e-11 (3)."""
    N, C, h, w_ = shape
    g = torch.Generator().manual_seed(1000 + seed + C + h * w_)
    f0 = torch.relu(torch.randn(shape, generator=g))
    f1 = torch.relu(f0 + 0.3 * torch.randn(shape, generator=g))
    P = h * w_
    a, b = f0.view(N, C, P), f1.view(N, C, P)
    if P > 1:
        a[:, :, 0] = 0.0
    if P > 2:
        a[:, :, 1] = 0.0
        b[:, :, 1] = 0.0
    if P > 3:
        a[:, :, 2] *= 1e4
        b[:, :, 2] *= 1e4
    if P > 4:
        a[:, :, 3] *= 1e-11
        b[:, :, 3] *= 1e-11
    w = torch.rand(C, generator=g) * 0.05
    return f0, f1, w


# ------------------------------------------------------------------------------------------------
# inputs
def im2tensor(u8):
    """(H,W,3) or (N,H,W,3) uint8 RGB -> (N,3,H,W) fp32 = float(double(v) / 127.5 - 1.0)."""
    a = np.asarray(u8)
    a = a[None] if a.ndim == 3 else a
    return torch.from_numpy((a.astype(np.float64) / 127.5 - 1.0).astype(np.float32).transpose(0, 3, 1, 2).copy())


def unit01(u8):
    """(N,H,W,3) uint8 -> (N,3,H,W) fp32 in [0,1] (the `normalize=True` input form)."""
    a = np.asarray(u8)
    a = a[None] if a.ndim == 3 else a
    return torch.from_numpy(a.transpose(0, 3, 1, 2).copy()).float() / 255.0


def scaling(x):
    """ScalingLayer in fp32."""
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    return (x - shift) / scale


def image_pair(key):
    """The fixture's pair `key`: two (N,H,W,3) uint8 RGB arrays."""
    N, H, W, seed = PAIRS[key]
    rng = np.random.default_rng(seed)
    img0 = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    noise = rng.integers(-NOISE, NOISE + 1, size=(N, H, W, 3))
    img1 = np.clip(img0.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return img0, img1


# ------------------------------------------------------------------------------------------------
# the trunk
def trunk_shapes():
    """(name, shape) of the trunk's parameters in the reference's state_dict order (`model.net`)."""
    out, cin = [], 3
    for s, (idxs, width) in enumerate(zip(SLICES, _WIDTHS)):
        for i in idxs:
            out.append((f"slice{s + 1}.{i}.weight", (width, cin, 3, 3)))
            out.append((f"slice{s + 1}.{i}.bias", (width,)))
            cin = width
    return out


def trunk_params(seed=TRUNK_SEED):
    """What oracle.seeding.seed_module(model.net, seed) writes into the reference's trunk."""
    return {k: torch.from_numpy(v) for k, v in seeded_arrays(trunk_shapes(), seed).items()}


def trunk(params, x):
    """relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of x (N,3,H,W), in x's dtype."""
    outs, h = [], x
    for s, idxs in enumerate(SLICES):
        if s > 0:
            h = F.max_pool2d(h, 2, 2)
        for i in idxs:
            h = F.relu(F.conv2d(h, params[f"slice{s + 1}.{i}.weight"].to(x.dtype),
                                params[f"slice{s + 1}.{i}.bias"].to(x.dtype), padding=1))
        outs.append(h)
    return outs


def lpips64(params, lins, in0, in1, scale=True):
    """The metric with fp32 trunk features and the float64 head: in0, in1 (N,3,H,W) fp32 in [-1,1];
    lins: five (C,) tensors or None (the lpips=False baseline).  -> (total (N,), layers (5,N), maps)."""
    with torch.no_grad():
        x0, x1 = (scaling(in0), scaling(in1)) if scale else (in0, in1)
        f0, f1 = trunk(params, x0), trunk(params, x1)
        res = [head64(a, b, None if lins is None else lins[k]) for k, (a, b) in enumerate(zip(f0, f1))]
    layers = torch.stack([r[0] for r in res])
    return layers.sum(dim=0), layers, [r[1] for r in res]
