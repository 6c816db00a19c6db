"""The LPIPS gradient references of tests/lpips_grad_ref.py without a GPU: the closed form against
float64 autograd, its zero-norm limit, the whole-metric gradient's fp32 / float64 distance on the fixture
pairs, and the new C entries' header and host-side validation."""
import os

import numpy as np
import pytest
import torch

import lpips_grad_ref as G
import lpips_ref as L
from vst import _lib

built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built (run __graft_entry__.build())")
# float64 closed form against float64 autograd: two orderings of ~C double-precision operations per
# element, C <= 512 -> far below 1e-10 of the pixel's largest gradient
REL64 = 1e-10
# the whole-metric fp32 autograd gradient against the float64 one, relative to the norm: 13 fp32
# convolutions deep, measured 3-6e-6 on these pairs; 1e-4 keeps the reference two orders of magnitude
# inside the GPU test's 2e-3 bar
REL32 = 1e-4


def _gl(N, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(N, generator=g)
    v[0] = -abs(v[0])  # mixed sign whatever the seed
    if N > 1:
        v[1] = abs(v[1])
    return v


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", L.HEAD_SHAPES)
def test_closed_form_equals_float64_autograd(shape, weighted):
    N, C, h, w_ = shape
    P = h * w_
    f0, f1, w = L.head_inputs(shape)
    w = w if weighted else None
    gl = _gl(N, 11)
    dA, dB, tA, tB = (t.reshape(N, C, P) for t in G.head_terms64(f0, f1, w, gl))
    rA, rB = (t.reshape(N, C, P) for t in G.head_autograd64(f0, f1, w, gl))
    assert torch.isfinite(dA).all() and torch.isfinite(dB).all()
    na = f0.double().pow(2).sum(dim=1).reshape(N, P)
    nb = f1.double().pow(2).sum(dim=1).reshape(N, P)
    for got, want, first, norm2 in ((dA, rA, tA, na), (dB, rB, tB, nb)):
        for p in range(P):
            if bool((norm2[:, p] == 0).any()):
                assert not torch.isfinite(want[:, :, p]).all()  # autograd: sqrt'(0) * 0
                continue
            # the two terms may cancel (f0 zero, w = ones: s is parallel to b), so the scale is the first term's
            scale = float(first[:, :, p].abs().max())
            assert float((got[:, :, p] - want[:, :, p]).abs().max()) <= REL64 * scale, (shape, p)
    if P > 2:
        # all-zero in both features: delta = 0, so exactly 0; all-zero in f0 only: the second term is 0 and
        # dA = s ra with delta = -b rb, ra = 1e10
        assert float(dA[:, :, 1].abs().max()) == 0.0 and float(dB[:, :, 1].abs().max()) == 0.0
        b = f1.double().reshape(N, C, P)[:, :, 0]
        rb = 1.0 / (b.pow(2).sum(dim=1, keepdim=True).sqrt() + L.EPS)
        wc = torch.ones(C, dtype=torch.float64) if w is None else w.double()
        want = 2.0 * wc.view(1, C) * (-b * rb) * gl.double().view(N, 1) / P * (1.0 / L.EPS)
        assert float((dA[:, :, 0] - want).abs().max()) <= REL64 * float(want.abs().max())
        assert float(want.abs().max()) > 0.0


@pytest.mark.parametrize("key", ["p16", "p32"])
def test_metric_gradient_fp32_against_float64(golden, key):
    g = golden("lpips_vgg")
    params = L.trunk_params(int(g["trunk_seed"]))
    lins = [torch.from_numpy(g[f"lin{k}"]) for k in range(5)]
    t0, t1 = L.im2tensor(g[key + "_img0"]), L.im2tensor(g[key + "_img1"])
    with torch.no_grad():
        _, f0, f1 = G.metric(params, lins, t0, t1, torch.float32)
    assert G.zero_norm_pixels(f0) == [0] * 5 and G.zero_norm_pixels(f1) == [0] * 5  # so autograd is finite
    total64, g64 = G.metric_grad(params, lins, t0, t1, torch.float64)
    total32, g32 = G.metric_grad(params, lins, t0, t1, torch.float32)
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all()
    assert np.abs(total64.numpy() - g[key + "_total"]).max() <= 1e-5 * np.abs(g[key + "_total"]).max()
    rel = float((g32.double() - g64).norm() / g64.norm())
    print(f"{key}: fp32 autograd gradient {rel:.2e} of the float64 gradient's norm")
    assert rel <= REL32


def test_header_declares_the_gradient_entries():
    protos = _lib.parse_header()
    assert protos["vst_lpips_head_bwd"] == ("int", ["float*", "long", "float*", "long", "float*", "float*", "int", "int",
                                                    "long", "float*", "long", "float*", "long", "void*"])
    assert protos["vst_lpips_input_bwd"] == ("int", ["float*", "float*", "int", "int", "int", "int", "int", "void*"])
    for name in ("vst_lpips_mean", "vst_lpips_mean_bwd"):
        assert protos[name][0] == "int" and protos[name][1][-1] == "void*", name


@built
def test_gradient_entries_validate_on_the_host():
    lib = _lib.lib.load()

    def bwd(f0=1, f1=1, gl=1, d0=1, N=1, C=64, P=63, bs=None, bsd=None):
        bs = C * P if bs is None else bs
        return lib.vst_lpips_head_bwd(f0, bs, f1, bs, None, gl, N, C, P, d0, C * P if bsd is None else bsd, None, 0, None)

    for bad in (dict(C=24), dict(C=1024), dict(C=8), dict(N=0), dict(f0=None), dict(f1=None), dict(gl=None), dict(d0=None),
                dict(P=0), dict(bs=10), dict(bsd=10)):
        assert bwd(**bad) == -1, bad
    assert lib.vst_lpips_head_bwd(1, 64 * 63, 1, 64 * 63, None, 1, 1, 64, 63, 1, 64 * 63, 1, 10, None) == -1  # d1's stride
    assert lib.vst_lpips_input_bwd(None, 1, 1, 16, 16, 0, 1, None) == -1
    assert lib.vst_lpips_input_bwd(1, 1, 1, 16, 16, 3, 1, None) == -1
    assert lib.vst_lpips_mean(None, 1, 1.0, 1, None) == -1
    assert lib.vst_lpips_mean_bwd(1, 0, 1.0, 1, None) == -1
