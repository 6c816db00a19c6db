"""CPU references for the gradient of LPIPS (VGG), for the tests of `vst_lpips_head_bwd` and
`vst.lpips.LPIPS.distance_to`.

TEST INFRASTRUCTURE ONLY.  With the notation of tests/lpips_ref.py (`head64`): per pixel a, b are the two
features, na = sqrt(sum a^2), ra = 1 / (na + 1e-10), likewise nb, rb; delta_c = a_c ra - b_c rb;
layer[n] = (1 / P) sum_p sum_c w_c delta_c^2.  For an upstream gradient gl[n] of layer[n]:
  s_c  = 2 w_c delta_c gl[n] / P
  dA_c =  s_c ra - (sum_k s_k a_k) ra^2 a_c / na      (second term := 0 where na == 0)
  dB_c = -s_c rb + (sum_k s_k b_k) rb^2 b_c / nb      (second term := 0 where nb == 0)
  * `head_grad64`: that closed form in float64 (finite at zero-norm pixels, where autograd gives NaN);
  * `head_grad32`: the fp32 torch-autograd gradient of the reference's own op sequence (`lpips_ref.head32`);
  * `metric_grad`: the gradient of sum_n gl[n] total[n] with respect to in0 through `lpips_ref.scaling`,
    `lpips_ref.trunk` and the head, by torch autograd in fp32 (`head32`) or float64 (`head64`).
"""
import torch

import lpips_ref as L


def head_grad64(f0, f1, w, gl):
    """f0, f1: (N,C,h,w); w: (C,) or None; gl: (N,).  -> (dA, dB) float64, shaped like f0."""
    return head_terms64(f0, f1, w, gl)[:2]


def head_terms64(f0, f1, w, gl):
    """-> (dA, dB, s ra, s rb): the gradients and their first terms, whose size is the scale of the
    rounding error where the two terms cancel (s parallel to the feature: a half-zero pixel with w = ones)."""
    a, b = f0.to(torch.float64), f1.to(torch.float64)
    N, C, h, w_ = a.shape
    P = h * w_
    na = a.pow(2).sum(dim=1, keepdim=True).sqrt()
    nb = b.pow(2).sum(dim=1, keepdim=True).sqrt()
    ra, rb = 1.0 / (na + L.EPS), 1.0 / (nb + L.EPS)
    delta = a * ra - b * rb
    wc = torch.ones(C, dtype=torch.float64) if w is None else w.to(torch.float64)
    s = 2.0 * wc.view(1, C, 1, 1) * delta * gl.to(torch.float64).view(N, 1, 1, 1) / P
    ua = torch.where(na > 0, a / torch.where(na > 0, na, torch.ones_like(na)), torch.zeros_like(a))
    ub = torch.where(nb > 0, b / torch.where(nb > 0, nb, torch.ones_like(nb)), torch.zeros_like(b))
    dA = s * ra - (s * a).sum(dim=1, keepdim=True) * ra * ra * ua
    dB = -s * rb + (s * b).sum(dim=1, keepdim=True) * rb * rb * ub
    return dA, dB, s * ra, s * rb


def _head_autograd(head, f0, f1, w, gl, dtype):
    a = f0.to(dtype).clone().requires_grad_(True)
    b = f1.to(dtype).clone().requires_grad_(True)
    layer, _ = head(a, b, None if w is None else w.to(dtype))
    (layer * gl.to(dtype)).sum().backward()
    return a.grad, b.grad


def head_grad32(f0, f1, w, gl):
    """(dA, dB) of `lpips_ref.head32` by fp32 autograd (NaN where a norm is exactly 0)."""
    return _head_autograd(L.head32, f0, f1, w, gl, torch.float32)


def head_autograd64(f0, f1, w, gl):
    """(dA, dB) of `lpips_ref.head64` by float64 autograd (NaN where a norm is exactly 0)."""
    return _head_autograd(L.head64, f0, f1, w, gl, torch.float64)


def metric(params, lins, in0, in1, dtype, scale=True):
    """total (N,) of the whole metric in `dtype`, with the graph of in0 (a leaf of `dtype`), and the
    two sides' trunk features."""
    head = L.head32 if dtype == torch.float32 else L.head64
    x0, x1 = in0, in1.to(dtype)
    if scale:
        x0, x1 = L.scaling(x0), L.scaling(x1)
    f0 = L.trunk(params, x0)
    with torch.no_grad():
        f1 = L.trunk(params, x1)
    total = 0
    for k, (a, b) in enumerate(zip(f0, f1)):
        total = total + head(a, b, None if lins is None else lins[k].to(dtype))[0]
    return total, f0, f1


def metric_grad(params, lins, in0, in1, dtype, gl=None):
    """-> (total (N,) detached, d sum_n gl[n] total[n] / d in0) in `dtype` (gl None: ones)."""
    x = in0.to(dtype).clone().requires_grad_(True)
    total, _, _ = metric(params, lins, x, in1, dtype)
    seed = torch.ones_like(total) if gl is None else gl.to(dtype)
    (total * seed).sum().backward()
    return total.detach(), x.grad


def zero_norm_pixels(feats):
    """Pixels of each level whose channel norm is exactly 0."""
    return [int((f.detach().pow(2).sum(dim=1) == 0).sum()) for f in feats]
