"""The SSIM gradient on the GPU (vst_ssim_bwd, vst_ssim_c, vst.metrics.ssim_scores / SSIMLoss) against
the float64 references of tests/ssim_grad_ref.py.

Bar: that of tests/test_gpu_metrics.py (`_bar`, imported): the worst element may sit at most 4x as far
from float64 as torch's own fp32 autograd gradient of the five-conv2d formulation sits on the same
inputs, with a floor of 1e-6 of the largest element.  The measured distances are printed and recorded in
DESIGN.md 4.16.
"""
import numpy as np
import pytest
import torch

import metrics_ref as M
import ssim_grad_ref as G
from test_gpu_metrics import _bar

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _taps(win):
    return np.ascontiguousarray(M.gauss_window(win, 1.5)[0].numpy(), dtype=np.float32)


def _bwd(x, y, g, win, C1, C2, want_d2):
    """One vst_ssim_bwd call on device tensors into NaN-filled outputs -> (d1, d2 or None) on the device."""
    from vst._lib import lib, ptr, stream

    B, C, H, W = x.shape
    taps = _taps(win)
    d1 = torch.full_like(x, NAN)
    d2 = torch.full_like(x, NAN) if want_d2 else None
    lib.vst_ssim_bwd(ptr(x), ptr(y), taps.ctypes.data, win, B, C, H, W, C1, C2, ptr(g), ptr(d1), ptr(d2), stream())
    return d1, d2


def _fwd(x, y, win, C1, C2, tile, constants=True):
    """vst_ssim_c (or vst_ssim) -> (scores, map) on the device."""
    from vst._lib import lib, ptr, stream

    B, C, H, W = x.shape
    taps = _taps(win)
    out, smap = torch.full((B,), NAN, device=x.device), torch.full_like(x, NAN)
    ws = torch.empty(max(1, lib.vst_ssim_workspace(B, C, H, W) // 8), dtype=torch.float64, device=x.device)
    if constants:
        lib.vst_ssim_c(ptr(x), ptr(y), taps.ctypes.data, win, B, C, H, W, C1, C2, ptr(out), ptr(smap), ws.data_ptr(), tile,
                       stream())
    else:
        lib.vst_ssim(ptr(x), ptr(y), taps.ctypes.data, win, B, C, H, W, ptr(out), ptr(smap), ws.data_ptr(), tile, stream())
    return out, smap


def _check_case(key, shape, kind, win, seed, want_d2, data_range):
    ref = G.reference(shape, kind, win, seed, data_range)
    x, y, g = (ref[k].cuda() for k in ("x", "y", "g"))
    d1, d2 = _bwd(x, y, g, win, ref["C1"], ref["C2"], want_d2)
    assert torch.isfinite(d1).all(), "an element of d1 was not written"
    _bar(d1.cpu().numpy(), ref["dx32"], ref["dx64"], f"{key} L{data_range:g} d1")
    if want_d2:
        assert torch.isfinite(d2).all(), "an element of d2 was not written"
        _bar(d2.cpu().numpy(), ref["dy32"], ref["dy64"], f"{key} L{data_range:g} d2")


@pytest.mark.parametrize("want_d2", [False, True])
@pytest.mark.parametrize("key,shape,kind,win,seed", G.cases())
def test_ssim_bwd_vs_float64(key, shape, kind, win, seed, want_d2):
    _check_case(key, shape, kind, win, seed, want_d2, 1.0)


@pytest.mark.parametrize("want_d2", [False, True])
@pytest.mark.parametrize("key,shape,kind,win,seed", [c for c in G.cases() if c[2] == "u255"])
def test_ssim_bwd_vs_float64_data_range_255(key, shape, kind, win, seed, want_d2):
    _check_case(key, shape, kind, win, seed, want_d2, 255.0)


@pytest.mark.parametrize("win", [1, 5, 7, 9])
def test_ssim_bwd_other_windows(win):
    """The template's other radii (11 and 3 are the main set), several tiles, both gradients."""
    key, shape, kind, _, seed = [c for c in G.cases() if c[1] == (2, 2, 45, 33) and c[2] == "unit"][0]
    _check_case(key.replace("w11", f"w{win}"), shape, kind, win, seed, True, 1.0)


@pytest.mark.parametrize("shape", G.SHAPES)
def test_ssim_bwd_writes_every_element(shape):
    x, y, g = (t.cuda() for t in G.inputs(shape, "unit", 41))
    C1, C2 = G.constants(1.0)
    for win in G.WINDOWS:
        for want_d2 in (False, True):
            for d in _bwd(x, y, g, win, C1, C2, want_d2):
                assert d is None or bool(torch.isfinite(d).all()), (shape, win, want_d2)


def test_ssim_bwd_bitwise_reproducible():
    shape, win = (2, 2, 45, 33), 11
    ref = G.reference(shape, "unit", win, 77)
    x, y, g = (ref[k].cuda() for k in ("x", "y", "g"))
    C1, C2 = ref["C1"], ref["C2"]
    d1, d2 = _bwd(x, y, g, win, C1, C2, True)
    e1, e2 = _bwd(x, y, g, win, C1, C2, True)
    assert torch.equal(d1, e1) and torch.equal(d2, e2)  # run to run
    only1, none = _bwd(x, y, g, win, C1, C2, False)
    assert none is None and torch.equal(only1, d1)  # d1 does not depend on whether d2 is wanted
    for n in range(shape[0]):  # image n alone gives image n's bits
        a1, a2 = _bwd(x[n:n + 1].contiguous(), y[n:n + 1].contiguous(), g[n:n + 1].contiguous(), win, C1, C2, True)
        assert torch.equal(a1[0], d1[n]) and torch.equal(a2[0], d2[n])
    # swapped inputs: d1 <-> d2, to the bar (the two directions do not share every rounding)
    s1, s2 = _bwd(y, x, g, win, C1, C2, True)
    _bar(s1.cpu().numpy(), ref["dy32"], ref["dy64"], "swapped d1 = dL/dy")
    _bar(s2.cpu().numpy(), ref["dx32"], ref["dx64"], "swapped d2 = dL/dx")
    # a zero upstream gradient gives zeros
    z1, z2 = _bwd(x, y, torch.zeros_like(g), win, C1, C2, True)
    assert float(z1.abs().max()) == 0.0 and float(z2.abs().max()) == 0.0


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("key,shape,kind,seed", M.ssim_cases())
def test_ssim_c_bitwise_equals_ssim(key, shape, kind, seed, tile):
    x, y = (t.cuda() for t in M.ssim_inputs(shape, kind, seed))
    C1, C2 = G.constants(1.0)
    for win in G.WINDOWS:
        s_c, m_c = _fwd(x, y, win, C1, C2, tile)
        s_0, m_0 = _fwd(x, y, win, C1, C2, tile, constants=False)
        assert torch.isfinite(s_0).all() and torch.isfinite(m_0).all()
        assert torch.equal(s_c, s_0) and torch.equal(m_c, m_0), (key, win)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("key,shape,kind,win,seed", [c for c in G.cases() if c[2] == "u255"])
def test_ssim_c_data_range_255_vs_float64(key, shape, kind, win, seed, tile):
    x, y = M.ssim_inputs(shape, kind, seed)
    C1, C2 = G.constants(255.0)
    score, smap = _fwd(x.cuda(), y.cuda(), win, C1, C2, tile)
    m64, m32 = (G.ssim_map_c(x.to(dt), y.to(dt), win, 1.5, C1, C2) for dt in (torch.float64, torch.float32))
    per = lambda m: m.mean(dim=[2, 3]).mean(dim=1).numpy()  # noqa: E731
    _bar(score.cpu().numpy(), per(m32), per(m64), f"{key} L255 tile{tile} score")
    _bar(smap.cpu().numpy(), m32.numpy(), m64.numpy(), f"{key} L255 tile{tile} map")


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("data_range,kind", [(1.0, "unit"), (255.0, "u255")])
def test_ssim_scores_autograd(data_range, kind, both):
    from vst.metrics import ssim_scores

    shape, win = (2, 3, 13, 37), 11
    ref = G.reference(shape, kind, win, 55, data_range)
    a = ref["x"].cuda().requires_grad_(True)
    b = ref["y"].cuda().requires_grad_(both)
    s = ssim_scores(a, b, window_size=win, data_range=data_range)
    assert s.shape == (shape[0],) and s.grad_fn is not None
    _bar(s.detach().cpu().numpy(), ref["s32"], ref["s64"], f"ssim_scores L{data_range:g} value")
    (s * ref["g"].cuda()).sum().backward()
    _bar(a.grad.cpu().numpy(), ref["dx32"], ref["dx64"], f"ssim_scores L{data_range:g} img1.grad")
    if both:
        _bar(b.grad.cpu().numpy(), ref["dy32"], ref["dy64"], f"ssim_scores L{data_range:g} img2.grad")
    else:
        assert b.grad is None
    if data_range == 1.0:  # the metric's own bits
        from vst.metrics import ssim

        assert torch.equal(s.detach(), ssim(a.detach(), b.detach(), window_size=win, reduction="none"))


def test_ssim_scores_records_nothing_without_grad():
    from vst.metrics import SSIMMetric, ssim, ssim_scores

    x, y = (t.cuda() for t in M.ssim_inputs((2, 3, 13, 37), "unit", 5))
    assert ssim_scores(x, y).grad_fn is None
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert ssim_scores(xr, y).grad_fn is None
    # only img2 requires grad: its gradient alone comes back
    yr = y.clone().requires_grad_(True)
    ssim_scores(x, yr).sum().backward()
    assert yr.grad is not None and bool(torch.isfinite(yr.grad).all()) and float(yr.grad.abs().max()) > 0
    # the metric stays forward-only
    out = SSIMMetric(11, 3, 1.5, reduction="none").cuda()(xr, y)
    assert out.grad_fn is None and not out.requires_grad
    assert ssim(xr, y).grad_fn is None


@pytest.mark.parametrize("weight", [1.0, 2.5])
def test_ssim_loss_value_and_gradient(weight):
    from vst import ops
    from vst.metrics import SSIMLoss

    shape, win = (2, 3, 13, 37), 11
    ref = G.reference(shape, "u255", win, 66, 255.0)
    B = shape[0]
    loss = SSIMLoss(window_size=win, weight=weight).set_target(ref["y"].cuda())
    pred = ref["x"].cuda().requires_grad_(True)
    val = loss(pred)
    assert val.dim() == 0 and val.grad_fn is not None
    # the float64 / fp32 references of the loss and of its gradient (upstream gradient -weight / B per image)
    gl = torch.full((B,), -weight / B)
    want = {}
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        s, dx, _ = G.autograd_grads(ref["x"], ref["y"], gl, win, 1.5, ref["C1"], ref["C2"], dt)
        want["s" + tag], want["d" + tag] = float(s.double().mean()), dx.numpy()
    total = ops.sum_scalars(val, val.detach() * 0)  # composes with the trainers' loss sum
    total.backward()
    # 1 - mean SSIM drops the digits of the mean that cancel against 1, so the value is held to the bar
    # as the mean score it encodes: 1 - loss / weight
    assert 0.0 < want["s64"] < 1.0
    _bar(1.0 - val.item() / weight, want["s32"], want["s64"], f"SSIMLoss w{weight} mean score")
    _bar(pred.grad.cpu().numpy(), want["d32"], want["d64"], f"SSIMLoss w{weight} pred.grad")
    with torch.no_grad():
        assert loss(pred).grad_fn is None


def test_error_cases_raise_vsterror():
    from vst._lib import VstError
    from vst.metrics import SSIMLoss, ssim_scores

    x, y = (t.cuda() for t in M.ssim_inputs((1, 3, 11, 11), "unit", 5))
    with pytest.raises(VstError):
        ssim_scores(x.cpu(), y)
    with pytest.raises(VstError):
        ssim_scores(x, y.cpu())
    with pytest.raises(VstError):
        ssim_scores(x, y[:, :2].contiguous())
    with pytest.raises(VstError):
        ssim_scores(x, y, window_size=4)
    with pytest.raises(VstError):
        ssim_scores(x, y, window_size=13)
    with pytest.raises(VstError):
        ssim_scores(x.double(), y.double())
    with pytest.raises(VstError):
        SSIMLoss(window_size=12)
    loss = SSIMLoss()
    with pytest.raises(VstError):
        loss(x)  # no target
    with pytest.raises(VstError):
        loss.set_target(y.cpu())
    loss.set_target(y)
    with pytest.raises(VstError):
        loss(x.cpu())
    with pytest.raises(VstError):
        loss(x[:, :, :5].contiguous())


def test_cases_outside_the_bar_return_without_error():
    """Not held to a bar: a flat region of a [0,255] image at data range 1, where
    sigma^2 = E[x^2] - mu^2 cancels to noise far above C2 in fp32 -- in the reference's own arithmetic as
    much as here -- and the exactly identical pair, whose exact gradient is zero.  Only: the kernel
    returns, and what it gives is printed."""
    shape, win = (1, 1, 40, 70), 11
    x, y, g = G.inputs(shape, "u255", 88)
    x[..., 8:32, 20:60] = 200.0
    y[..., 8:32, 20:60] = 180.0
    C1, C2 = G.constants(1.0)
    d1, d2 = _bwd(x.cuda(), y.cuda(), g.cuda(), win, C1, C2, True)
    torch.cuda.synchronize()
    _, dx64, _ = G.autograd_grads(x, y, g, win, 1.5, C1, C2, torch.float64)
    _, dx32, _ = G.autograd_grads(x, y, g, win, 1.5, C1, C2, torch.float32)
    scale = float(dx64.abs().max())
    print(f"flat region, data range 1: |hip - f64| {float((d1.cpu().double() - dx64).abs().max()) / scale:.2e} rel, "
          f"|torch fp32 - f64| {float((dx32.double() - dx64).abs().max()) / scale:.2e} rel")
    xs, ys, gs = (t.cuda() for t in G.inputs((2, 3, 13, 37), "u255", 89))
    i1, i2 = _bwd(xs, xs.clone(), gs, win, *G.constants(255.0), True)
    torch.cuda.synchronize()
    print(f"identical pair: largest |d1| {float(i1.abs().max()):.3e}, |d2| {float(i2.abs().max()):.3e} (exact: 0)")
