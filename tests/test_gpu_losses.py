"""The loss, warp, mask, normalisation and Adam kernels (loss_misc.hip, the warp / mask part of
pool_warp.hip) against the float64 references of tests/losses_ref.py, on a real MI355X.

Every comparison is with the float64 reference, never with another kernel.  The inputs, the bounds
and their derivations live in tests/losses_ref.py; tests/test_losses_ref.py shows on the CPU that the
plain float32 form of each operation meets every bound applied here on these very inputs, that the
mask test's guard band holds at most 1% of the pixels, and that the warp flows reach the sort tiers
named below.  A margin is error / bound: <= 1 passes.

What the shapes are for:
  * temporal losses, MSE, TV, TV-sqrt, sum: one grid is at most 1024 blocks of 256 threads; the
    262,656-item cases run the grid-stride loop and the 1024-partial finisher ("tail": only the
    strided second pass sees a non-zero mask);
  * Adam: K = 4 steps from step 7 with non-zero moments, so b1, b2, both bias corrections and the
    moments themselves are compared (at step 1 from zero the update is lr g / (|g| + eps') whatever
    the kernel does with them).  Moment bounds: 4x the error of float32 torch.optim.Adam against the
    float64 reference on these inputs (measured m 6.42e-08, v 3.05e-08 -> bounds 2.6e-07, 1.25e-07,
    relative to |ref| + max_t |g_t| resp. |ref| + max_t g_t^2);
  * warp backward, gather form: the per-source tap lists are sorted in four tiers -- <= 8 and <= 16
    entries in registers, <= 512 by rank in LDS, longer ones by insertion on one lane; "mid" reaches
    the second and third, "insertion" the fourth (lists of 768), and the 1025 x 1024 case is the
    smallest with more than 1024 scan blocks, where the totals scan carries between chunks.
"""
import functools

import pytest
import torch

import losses_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def G(t):
    return None if t is None else t.to(DEV)


def C(t):
    return t.detach().cpu()


def _gout():
    return torch.tensor(L.GOUT, device=DEV)


def _workspace():
    from vst import ops

    return torch.empty(ops.LOSS_WS, device=DEV), torch.empty(3, device=DEV)


# ------------------------------------------------------------------ 1. temporal losses
def _temporal_cases():
    for mode in (0, 1):
        for shape in L.TEMPORAL_SHAPES[mode]:
            for kind in L.TEMPORAL_MASKS:
                for needs in ("a", "b", "ab"):
                    yield mode, shape, kind, needs
        for kind in L.TEMPORAL_BIG_MASKS:
            yield mode, L.TEMPORAL_BIG[mode], kind, "ab"


@functools.lru_cache(maxsize=None)
def _temporal_ref(mode, shape, kind):
    args = L.temporal_case(mode, shape, kind)
    return args, L.temporal_ref(mode, *args)


@pytest.mark.parametrize("mode,shape,kind,needs", list(_temporal_cases()))
def test_temporal_losses(mode, shape, kind, needs):
    from vst import ops

    (a, b, c, d, mask, weight), (loss64, count, ga64, gb64) = _temporal_ref(mode, shape, kind)
    ag, bg = G(a).requires_grad_("a" in needs), G(b).requires_grad_("b" in needs)
    if mode == 0:
        loss = ops.feature_temporal_loss(ag, bg, G(mask), weight)
    else:
        loss = ops.output_temporal_loss(ag, bg, G(c), G(d), G(mask), weight)
    dev_count = float(loss.grad_fn.saved_tensors[-1][2])  # out[2]: the device-side count
    loss.backward(_gout())
    margins = {"loss": L.loss_margin(loss.item(), loss64)}
    for name, t, ref in (("a", ag, ga64), ("b", bg, gb64)):
        if name in needs:
            margins["d" + name] = L.elem_margin(C(t.grad), ref * L.GOUT)
        else:
            assert t.grad is None
    print(mode, shape, kind, needs, "count", dev_count, "margins", margins)
    assert dev_count == count  # C * nnz, exactly
    assert torch.isfinite(loss).item() and max(margins.values()) <= 1.0, margins
    if count == 0:  # defined as a zero loss with zero gradients (margins above demand the exact zeros)
        assert loss.item() == 0.0


# ------------------------------------------------------------------ 2. MSE, TV, TV-sqrt, sum_scaled
@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse(name):
    from vst import ops

    a, b = L.mse_case(name)
    loss64, ga64, gb64 = L.mse(a, b, L.MSE_WEIGHT)
    full = a.numel() == b.numel()
    ag, bg = G(a).requires_grad_(True), G(b).requires_grad_(full)
    loss = ops.mse(ag, bg, L.MSE_WEIGHT)
    loss.backward(_gout())
    margins = {"loss": L.loss_margin(loss.item(), loss64), "da": L.elem_margin(C(ag.grad), ga64 * L.GOUT)}
    if full:
        margins["db"] = L.elem_margin(C(bg.grad).reshape(gb64.shape), gb64 * L.GOUT)
    print(name, margins)
    assert max(margins.values()) <= 1.0, margins


@pytest.mark.parametrize("shape", L.TV_SHAPES)
@pytest.mark.parametrize("which", ["tv", "tv_sqrt"])
def test_tv(which, shape):
    from vst import ops

    s = L.tv_case(shape, flat=which == "tv_sqrt")
    loss64, g64 = (L.tv if which == "tv" else L.tv_sqrt)(s, L.TV_WEIGHT)
    sg = G(s).requires_grad_(True)
    loss = (ops.tv_loss if which == "tv" else ops.tv_sqrt_loss)(sg, L.TV_WEIGHT)
    loss.backward(_gout())
    margins = {"loss": L.loss_margin(loss.item(), loss64), "ds": L.elem_margin(C(sg.grad), g64 * L.GOUT)}
    print(which, shape, margins)
    assert max(margins.values()) <= 1.0, margins


@pytest.mark.parametrize("shape", [(1, 2, 1, 5), (1, 2, 5, 1)])
def test_tv_rejects_single_row_or_column(shape):
    """The entries refuse H == 1 / W == 1 (no term exists) before any launch."""
    from vst import ops
    from vst._lib import VstError

    for fn in (ops.tv_loss, ops.tv_sqrt_loss):
        with pytest.raises(VstError):
            fn(torch.zeros(shape, device=DEV).requires_grad_(True), 1.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", L.SUM_SIZES)
def test_sum_scaled(n):
    from vst._lib import lib, ptr, stream

    x = L.sum_case(n)
    ws, out = _workspace()
    xd = G(x)
    lib.vst_sum_scaled(ptr(xd), n, L.SUM_WEIGHT, ptr(ws), ptr(out), stream())
    out = C(out)
    margin = L.loss_margin(out[0].item(), L.sum_scaled(x, L.SUM_WEIGHT))
    print(n, margin)
    assert margin <= 1.0 and out[1].item() == L.SUM_WEIGHT and out[2].item() == 0.0


# ------------------------------------------------------------------ 3. Adam
@pytest.mark.parametrize("gscale", L.ADAM_GSCALES)
def test_adam_steps(gscale):
    """m, v and p after each of K consecutive steps from non-zero moments."""
    from vst._lib import lib, ptr, stream

    p, m, v, grads, gmax = L.adam_case(gscale)
    ref = L.adam(p, m, v, grads, L.ADAM_FIRST, gscale=gscale, **L.ADAM_HYPER)
    h = L.ADAM_HYPER
    pg, mg, vg = G(p), G(m), G(v)
    for k, g in enumerate(grads):
        gd = G(g)
        lib.vst_adam(ptr(pg), ptr(gd), ptr(mg), ptr(vg), p.numel(), h["lr"], h["b1"], h["b2"], h["eps"],
                     L.ADAM_FIRST + k, gscale, stream())
        margins = L.adam_margins(C(pg), C(mg), C(vg), ref[k], gmax, L.ADAM_K)
        print(gscale, "step", L.ADAM_FIRST + k, "p / m / v margins", margins,
              "m / v errors", L.adam_moment_errors(C(mg), C(vg), ref[k], gmax))
        assert max(margins) <= 1.0, (k, margins)


def test_adam_first_step_flat_params():
    """n = 5, step 1 from zero moments, through FlatParams.adam."""
    from vst.reconet._flat import FlatParams

    p, m, v, grads, gmax = L.adam_first_case()
    ref = L.adam(p, m, v, grads, 1, **L.ADAM_HYPER)
    mod = torch.nn.Module()
    mod.w = torch.nn.Parameter(G(p))
    flat = FlatParams(mod)
    assert not flat.m.any() and not flat.v.any()
    flat.g.copy_(G(grads[0]))
    h = L.ADAM_HYPER
    flat.adam(1, h["lr"], (h["b1"], h["b2"]), h["eps"])
    margins = L.adam_margins(C(flat.p), C(flat.m), C(flat.v), ref[0], gmax, 1)
    print(margins)
    assert max(margins) <= 1.0 and torch.equal(mod.w.detach(), flat.p)


# ------------------------------------------------------------------ 4. / 5. warp
@pytest.mark.parametrize("kind,shape", L.WARP_FWD_CASES)
def test_warp_fwd(kind, shape):
    from vst import ops

    x, flo = L.warp_case(kind, shape)
    ref, A = L.warp_fwd(x, flo)
    out = C(ops.warp(G(x), G(flo)))
    margin = L.warp_margin(out, ref, A, 4)
    print(kind, shape, margin)
    assert margin <= 1.0
    if kind == "outside":  # all four taps out of bounds
        assert not out.any()
    if kind == "integer":  # a single-tap copy
        assert torch.equal(out.double(), ref)


@functools.lru_cache(maxsize=None)
def _warp_bwd_ref(kind, shape):
    g, flo = L.warp_case(kind, shape)
    return g, flo, L.warp_bwd(g, flo)


@pytest.mark.parametrize("kind,shape", L.WARP_BWD_CASES)
def test_warp_bwd_gather(kind, shape):
    """The deterministic gather form: within the bound, exact zeros where no tap lands, and two runs
    bitwise equal (the fill pass's atomics order the lists differently run to run; the sort undoes it)."""
    from vst import ops

    g, flo, (ref, A, n) = _warp_bwd_ref(kind, shape)
    runs = []
    for _ in range(2):
        xg = torch.zeros(shape, device=DEV).requires_grad_(True)
        ops.warp(xg, G(flo)).backward(G(g))
        runs.append(C(xg.grad))
    margin = L.warp_margin(runs[0], ref, A, n)
    print(kind, shape, "longest list", int(n.max()), "margin", margin)
    assert margin <= 1.0
    assert torch.equal(runs[0], runs[1])
    empty = (n == 0).view(shape[0], 1, *shape[2:]).expand(shape)
    assert not runs[0][empty].any()


@pytest.mark.parametrize("kind,shape", L.WARP_ATOMIC_CASES)
def test_warp_bwd_atomic(kind, shape):
    """vst_warp_bwd, the float-atomic scatter into a zero-filled gradient, under the same bound."""
    from vst._lib import lib, ptr, stream

    g, flo, (ref, A, n) = _warp_bwd_ref(kind, shape)
    B, Cc, H, W = shape
    gd, fd, gx = G(g), G(flo), torch.empty(shape, device=DEV)
    lib.vst_fill(ptr(gx), gx.numel(), 0.0, stream())
    lib.vst_warp_bwd(ptr(gd), ptr(fd), ptr(gx), B, Cc, H, W, stream())
    margin = L.warp_margin(C(gx), ref, A, n)
    print(kind, shape, margin)
    assert margin <= 1.0


# ------------------------------------------------------------------ 6. flow consistency mask
@pytest.mark.parametrize("shape", L.MASK_SHAPES)
def test_flow_warp_mask(shape):
    from vst import ops

    f01, f10 = L.mask_case(shape)
    err = L.flow_mask_err(f01, f10)
    mask = C(ops.flow_warp_mask(G(f01), G(f10), L.MASK_THR))
    assert mask.shape == shape and bool(((mask == 0) | (mask == 1)).all())
    wrong, share = L.mask_check(mask, err)
    print(shape, "wrong", wrong, "guard band share", share)
    assert wrong == 0 and share <= L.MASK_BAND_SHARE


# ------------------------------------------------------------------ 7. vgg_normalize
@pytest.mark.parametrize("shape", L.NORM_SHAPES)
def test_vgg_normalize(shape):
    from vst import ops

    x, gout, _ = L.norm_case(shape)
    out64, _ = L.vgg_normalize(x)
    xg = G(x).requires_grad_(True)
    out = ops.VggNormalizeFn.apply(xg)
    out.backward(G(gout))
    margins = (L.elem_margin(C(out), out64), L.elem_margin(C(xg.grad), L.vgg_normalize_bwd(gout)))
    print(shape, margins)
    assert torch.equal(C(xg), x) and max(margins) <= 1.0, margins


@pytest.mark.parametrize("shape", L.NORM_SHAPES)
def test_vgg_normalize_inplace(shape):
    """The in-place form leaves x / 255 in its argument; with the output and the mutated argument both
    consumed the gradient is (gout / std[c] + gscaled) / 255."""
    from vst import ops

    x, gout, gscaled = L.norm_case(shape)
    out64, scaled64 = L.vgg_normalize(x)
    x0 = G(x).requires_grad_(True)
    xs = x0 * 1.0  # (a non-leaf: autograd refuses an in-place op on a leaf)
    xm, out = ops.VggNormalizeInplaceFn.apply(xs)
    assert xm.data_ptr() == xs.data_ptr()
    torch.autograd.backward([out, xm], [G(gout), G(gscaled)])
    margins = (L.elem_margin(C(out), out64), L.elem_margin(C(xm), scaled64),
               L.elem_margin(C(x0.grad), L.vgg_normalize_bwd(gout, gscaled)))
    print(shape, margins)
    assert max(margins) <= 1.0, margins


# ------------------------------------------------------------------ 8. ConvTanh backward
@pytest.mark.parametrize("prenorm", [0, 1])
def test_tanh_out_bwd(prenorm):
    from vst._lib import lib, ptr, stream

    gy, t = L.tanh_case()
    gyd, td, gv = G(gy), G(t), torch.empty(gy.shape, device=DEV)  # (named: a temporary's memory is reused)
    lib.vst_tanh_out_bwd(ptr(gyd), ptr(td), ptr(gv), gy.numel(), gy[0, 0].numel(), prenorm, stream())
    margin = L.elem_margin(C(gv), L.tanh_out_bwd(gy, t, prenorm))
    print(prenorm, margin)
    assert margin <= 1.0
