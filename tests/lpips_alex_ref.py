"""CPU restatement of LPIPS over the AlexNet trunk, for the tests of vst.lpips (net="alex") and csrc/alex.hip.

TEST INFRASTRUCTURE ONLY.  Written from the formulas (AA/lpips/pretrained_networks.py:57-95 and
torchvision's documented alexnet.features; the head, `im2tensor`, `scaling` and the image-pair
construction are tests/lpips_ref.py's):
  * `trunk_shapes` / `trunk_params`: the trunk's parameter names and shapes in the reference's state_dict
    order (`model.net`), and what oracle.seeding.seed_module writes into them;
  * `trunk`: features[0:12] as plain F.conv2d / max_pool2d in the input's dtype (fp32 or float64),
    returning relu1 .. relu5;
  * `lpips64`: fp32 trunk features and the float64 head (lpips_ref.head64);
  * `stem_inputs`: the stem kernel's test inputs.
tests/golden/lpips_alex.npz (gen_golden_lpips_alex.py) pins it to the reference's own outputs
(tests/test_lpips_alex_ref.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref as L
from oracle.seeding import seeded_arrays

CHNS = (64, 192, 384, 256, 256)
# (slice, torchvision alexnet.features index, Cin, Cout, kernel, stride, pad); slices 2 and 3 start with MaxPool2d(3, 2)
CONVS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
         (5, 10, 256, 256, 3, 1, 1))
POOL_BEFORE = (2, 3)
MIN_SIDE = 31

TRUNK_SEED = 511
# key: (N, H, W, seed) of the fixture's uint8 image pairs (lpips_ref.image_pair's construction, NOISE = 24)
PAIRS = {"a31": (1, 31, 31, 531), "a35": (2, 35, 67, 532), "a64": (1, 64, 98, 533)}
# the level grids of the pairs
GRIDS = {"a31": ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1)), "a35": ((8, 16), (3, 7), (1, 3), (1, 3), (1, 3)),
         "a64": ((15, 23), (7, 11), (3, 5), (3, 5), (3, 5))}


def image_pair(key):
    """The fixture's pair `key`: two (N,H,W,3) uint8 RGB arrays, built as lpips_ref.image_pair builds its own."""
    N, H, W, seed = PAIRS[key]
    rng = np.random.default_rng(seed)
    img0 = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    noise = rng.integers(-L.NOISE, L.NOISE + 1, size=(N, H, W, 3))
    img1 = np.clip(img0.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return img0, img1


def trunk_shapes():
    """(name, shape) of the trunk's parameters in the reference's state_dict order (`model.net`)."""
    out = []
    for s, i, cin, cout, k, _, _ in CONVS:
        out.append((f"slice{s}.{i}.weight", (cout, cin, k, k)))
        out.append((f"slice{s}.{i}.bias", (cout,)))
    return out


def trunk_params(seed=TRUNK_SEED):
    """What oracle.seeding.seed_module(model.net, seed) writes into the reference's trunk."""
    return {k: torch.from_numpy(v) for k, v in seeded_arrays(trunk_shapes(), seed).items()}


def trunk(params, x):
    """relu1 .. relu5 of x (N,3,H,W), in x's dtype."""
    outs, h = [], x
    for s, i, _, _, _, stride, pad in CONVS:
        if s in POOL_BEFORE:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, params[f"slice{s}.{i}.weight"].to(x.dtype), params[f"slice{s}.{i}.bias"].to(x.dtype),
                            stride=stride, padding=pad))
        outs.append(h)
    return outs


def lpips64(params, lins, in0, in1, scale=True, dtype=torch.float32):
    """The metric with trunk features in `dtype` (fp32: the reference's own; float64: the exact form) and the
    float64 head: in0, in1 (N,3,H,W) fp32 in [-1,1]; lins: five (C,) tensors or None (the lpips=False
    baseline).  -> (total (N,), layers (5,N), maps)."""
    with torch.no_grad():
        x0, x1 = (L.scaling(in0), L.scaling(in1)) if scale else (in0, in1)
        f0, f1 = trunk(params, x0.to(dtype)), trunk(params, x1.to(dtype))
        res = [L.head64(a, b, None if lins is None else lins[k]) for k, (a, b) in enumerate(zip(f0, f1))]
    layers = torch.stack([r[0] for r in res])
    return layers.sum(dim=0), layers, [r[1] for r in res]


def stem_inputs(N, H, W, Cout, seed=0):
    """(x, w, b) for the stem kernel: x of both signs over the ScalingLayer's range (about -2.2 .. 2.7: the
    images of [-1, 1] under (t - shift) / scale), w and b from seeded_arrays (He init, 0.1 N(0,1))."""
    rng = np.random.default_rng(7000 + seed + 31 * H + W)
    x = torch.from_numpy(rng.uniform(-2.2, 2.7, size=(N, 3, H, W)).astype(np.float32))
    arrs = seeded_arrays([("weight", (Cout, 3, 11, 11)), ("bias", (Cout,))], 7100 + seed + Cout)
    return x, torch.from_numpy(arrs["weight"]), torch.from_numpy(arrs["bias"])
