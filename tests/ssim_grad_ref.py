"""CPU references for the gradient of SSIM (vst_ssim_bwd, vst.metrics.ssim_scores / SSIMLoss).

TEST INFRASTRUCTURE ONLY.  Two independent forms in a chosen dtype, both on the fp32 2-D window of
metrics_ref.gauss_window cast up (what metrics_ref.ssim_map uses):
  * `autograd_grads`: torch autograd through the five-conv2d formulation of metrics_ref.ssim_map,
    generalised to C1 / C2 -- float64 is the yardstick, float32 the reference's own arithmetic;
  * `closed_form_grads`: the formulas the kernel implements (three / four D maps, then the window's
    adjoint, which for a symmetric zero-padded window is the same zero-padded window).
tests/test_ssim_grad_ref.py holds the two against each other.
"""
import numpy as np
import torch
import torch.nn.functional as F

import metrics_ref as M

SHAPES = list(M.SSIM_SHAPES) + [(1, 1, 12, 76), (2, 2, 45, 33), (1, 1, 1, 1), (1, 2, 3, 50)]
KINDS = M.SSIM_KINDS
WINDOWS = (11, 3)


def constants(data_range=1.0):
    """C1, C2 as Python doubles, as vst.metrics.ssim_scores forms them."""
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def inputs(shape, kind, seed):
    """metrics_ref.ssim_inputs plus a random signed upstream gradient of the (B,) scores."""
    x, y = M.ssim_inputs(shape, kind, seed)
    g = torch.Generator().manual_seed(seed + 7)
    return x, y, torch.randn(shape[0], generator=g)


def cases():
    """(id, shape, kind, window, seed): every shape in both value ranges with both windows."""
    return [(f"{'x'.join(map(str, shape))}-{kind}-w{win}", shape, kind, win, 300 + 10 * i + j)
            for i, shape in enumerate(SHAPES) for j, kind in enumerate(KINDS) for win in WINDOWS]


def _window(window_size, sigma, C, dtype):
    return M.gauss_window(window_size, sigma)[1].to(dtype).expand(C, 1, window_size, window_size).contiguous()


def ssim_map_c(a, b, window_size=11, sigma=1.5, C1=0.01**2, C2=0.03**2):
    """metrics_ref.ssim_map in the dtype (and on the device: tools/ssim_grad_bench.py times it on the
    GPU) of a and b with explicit constants (differentiable)."""
    C = a.shape[1]
    k = _window(window_size, sigma, C, a.dtype).to(a.device)
    conv = lambda t: F.conv2d(t, k, padding=window_size // 2, groups=C)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def scores(x, y, window_size=11, sigma=1.5, C1=0.01**2, C2=0.03**2, dtype=torch.float64):
    """(B,) per-image scores in `dtype`."""
    return ssim_map_c(x.to(dtype), y.to(dtype), window_size, sigma, C1, C2).mean(dim=[2, 3]).mean(dim=1)


def autograd_grads(x, y, gout, window_size=11, sigma=1.5, C1=0.01**2, C2=0.03**2, dtype=torch.float64):
    """(scores, dL/dx, dL/dy) with L = sum_b gout[b] score[b], by torch autograd in `dtype`."""
    a = x.to(dtype).clone().requires_grad_(True)
    b = y.to(dtype).clone().requires_grad_(True)
    s = ssim_map_c(a, b, window_size, sigma, C1, C2).mean(dim=[2, 3]).mean(dim=1)
    da, db = torch.autograd.grad((s * gout.to(dtype)).sum(), (a, b))
    return s.detach(), da, db


def closed_form_grads(x, y, gout, window_size=11, sigma=1.5, C1=0.01**2, C2=0.03**2, dtype=torch.float64):
    """(dL/dx, dL/dy) from the D maps: Dm, Dm', D11 (= D22), D12 and the zero-padded window."""
    a, b = x.to(dtype), y.to(dtype)
    B, C, H, W = a.shape
    k = _window(window_size, sigma, C, dtype)
    conv = lambda t: F.conv2d(t, k, padding=window_size // 2, groups=C)  # noqa: E731
    mu1, mu2, e11, e22, e12 = conv(a), conv(b), conv(a * a), conv(b * b), conv(a * b)
    A1 = 2 * mu1 * mu2 + C1
    A2 = 2 * (e12 - mu1 * mu2) + C2
    B1 = mu1 * mu1 + mu2 * mu2 + C1
    B2 = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    S = A1 * A2 / (B1 * B2)
    w = (gout.to(dtype) / (C * H * W)).view(B, 1, 1, 1)
    dA, dB = 2 * (A2 - A1) / (B1 * B2), 2 * S * (1 / B1 - 1 / B2)
    Dm1, Dm2 = w * (mu2 * dA - mu1 * dB), w * (mu1 * dA - mu2 * dB)
    D11, D12 = w * (-S / B2), w * (2 * A1 / (B1 * B2))
    dx = conv(Dm1) + 2 * a * conv(D11) + b * conv(D12)
    dy = conv(Dm2) + 2 * b * conv(D11) + a * conv(D12)
    return dx, dy


_CACHE = {}


def reference(shape, kind, win, seed, data_range=1.0):
    """The shared, cached reference of one case: inputs, float64 and float32 autograd results
    (numpy, read-only)."""
    key = (shape, kind, win, seed, data_range)
    if key not in _CACHE:
        x, y, g = inputs(shape, kind, seed)
        C1, C2 = constants(data_range)
        s64, dx64, dy64 = autograd_grads(x, y, g, win, 1.5, C1, C2, torch.float64)
        s32, dx32, dy32 = autograd_grads(x, y, g, win, 1.5, C1, C2, torch.float32)
        ref = {"x": x, "y": y, "g": g, "C1": C1, "C2": C2}
        for name, v in (("s64", s64), ("dx64", dx64), ("dy64", dy64), ("s32", s32), ("dx32", dx32), ("dy32", dy32)):
            arr = v.numpy().astype(np.float64)
            arr.setflags(write=False)
            ref[name] = arr
        _CACHE[key] = ref
    return _CACHE[key]
