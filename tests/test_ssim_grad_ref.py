"""The SSIM gradient references of tests/ssim_grad_ref.py without a GPU: the closed form the kernel
implements against float64 autograd of the five-conv2d formulation, the fp32 autograd gradient's own
distance from float64 (what the GPU bar is a multiple of), and the new C entries' header and host-side
validation."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as M
import ssim_grad_ref as G
from vst import _lib

built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built (run __graft_entry__.build())")
# float64 closed form against float64 autograd: two orderings of a few hundred double-precision
# operations per element (two 121-tap windows deep), so a few hundred x 1.1e-16 of the largest element
REL64 = 1e-10


@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("key,shape,kind,win,seed", G.cases())
def test_closed_form_equals_float64_autograd(key, shape, kind, win, seed, data_range):
    ref = G.reference(shape, kind, win, seed, data_range)
    dx, dy = G.closed_form_grads(ref["x"], ref["y"], ref["g"], win, 1.5, ref["C1"], ref["C2"], torch.float64)
    for got, want, what in ((dx, ref["dx64"], "dx"), (dy, ref["dy64"], "dy")):
        scale = float(np.abs(want).max())
        assert scale > 0 and np.isfinite(want).all()
        assert float(np.abs(got.numpy() - want).max()) <= REL64 * scale, (key, what)


def test_reference_generalises_the_metric_reference():
    """With the metric's constants the generalised map is metrics_ref.ssim_map's, bit for bit."""
    x, y = M.ssim_inputs((2, 3, 13, 37), "unit", 5)
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(G.ssim_map_c(x.to(dtype), y.to(dtype)), M.ssim_map(x, y, dtype=dtype))
    assert G.constants(1.0) == (0.01**2, 0.03**2)


def test_fp32_autograd_distance_from_float64():
    """The reference's own fp32 error on the case set (printed): small against the gradient, not zero, so
    a bar of 4x it is neither vacuous nor out of fp32's reach."""
    worst, best = 0.0, 1.0
    for key, shape, kind, win, seed in G.cases():
        ref = G.reference(shape, kind, win, seed)
        for a, b in (("dx32", "dx64"), ("dy32", "dy64")):
            rel = float(np.abs(ref[a] - ref[b]).max() / np.abs(ref[b]).max())
            worst, best = max(worst, rel), min(best, rel)
    print(f"fp32 autograd gradient: {best:.2e} .. {worst:.2e} of the largest element from float64")
    assert 0.0 < best and worst <= 1e-4


def test_header_declares_the_ssim_gradient_entries():
    protos = _lib.parse_header()
    assert protos["vst_ssim_c"] == ("int", ["float*", "float*", "float*", "int", "int", "int", "int", "int", "float",
                                            "float", "float*", "float*", "void*", "int", "void*"])
    assert protos["vst_ssim_bwd"] == ("int", ["float*", "float*", "float*", "int", "int", "int", "int", "int", "float",
                                              "float", "float*", "float*", "float*", "void*"])
    assert protos["vst_ssim_loss"] == ("int", ["float*", "int", "float", "float*", "void*"])
    assert protos["vst_ssim_loss_bwd"] == ("int", ["float*", "int", "float", "float*", "void*"])


@built
def test_ssim_gradient_entries_validate_on_the_host():
    lib = _lib.lib.load()
    taps = np.ones(11, dtype=np.float32).ctypes.data

    def bwd(img1=1, img2=1, t=taps, win=11, B=1, C=3, H=8, W=8, gout=1, d1=1):
        return lib.vst_ssim_bwd(img1, img2, t, win, B, C, H, W, 1e-4, 9e-4, gout, d1, None, None)

    for bad in (dict(img1=None), dict(img2=None), dict(t=None), dict(gout=None), dict(d1=None), dict(win=4), dict(win=13),
                dict(win=0), dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=65536, C=1), dict(H=1 << 16, W=1 << 15)):
        assert bwd(**bad) == -1, bad

    def fwd(out=1, ws=8, win=11, tile=0, c1=1e-4):
        return lib.vst_ssim_c(1, 1, taps, win, 1, 3, 8, 8, c1, 9e-4, out, None, ws, tile, None)

    for bad in (dict(out=None), dict(ws=None), dict(ws=12), dict(win=2), dict(tile=3), dict(c1=float("nan"))):
        assert fwd(**bad) == -1, bad
    assert lib.vst_ssim_loss(None, 1, 1.0, 1, None) == -1
    assert lib.vst_ssim_loss(1, 0, 1.0, 1, None) == -1
    assert lib.vst_ssim_loss_bwd(1, 1, 1.0, None, None) == -1
    assert lib.vst_ssim_loss_bwd(1, 65536, 1.0, 1, None) == -1
