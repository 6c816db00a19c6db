"""CPU checks of tests/losses_ref.py, the float64 yardstick of tests/test_gpu_losses.py (no GPU):

  * each reference agrees with the oracle's own float32 function (oracle/reconet_ref.py: `warp`,
    `flow_warp_mask`, the FTL / OTL / RL expressions, `adam_step`) within 1e-5 at small shapes, and
    `adam` with torch.optim.Adam run in float64;
  * on every input the GPU tests use, the float32 CPU rendition of the operation (the oracle function,
    or torch.optim.Adam in float32) meets the bound the GPU test applies -- a bound the plain float32
    form missed would be a wrong bound or a wrong input, not a wrong kernel;
  * the guard band of the mask test holds at most 1% of the pixels, from the reference alone;
  * the flows of the warp backward cases reach the list-length tiers they are there for.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import losses_ref as L
from oracle import reconet_ref as R


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------ float32 renditions (the oracle's expressions)
def ftl32(a, b, mask, weight):
    """oracle/reconet_ref.py:291-292 with autograd; (loss, d/da, d/db)."""
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    fm = (mask > 0).float().expand(-1, a.shape[1], -1, -1)
    loss = torch.sum(fm * (a - b) ** 2) * (1 / int(fm.count_nonzero())) * weight
    loss.backward()
    return loss.item(), a.grad, b.grad


def otl32(s2, ws1, i2, wi1, mask, weight):
    """oracle/reconet_ref.py:294-298 with autograd."""
    s2, ws1 = s2.clone().requires_grad_(True), ws1.clone().requires_grad_(True)
    ot = s2 - ws1
    it = i2 - wi1
    it = (0.2126 * it[:, 0] + 0.7152 * it[:, 1] + 0.0722 * it[:, 2]).unsqueeze(1).expand(-1, 3, -1, -1)
    m3 = mask.expand(-1, 3, -1, -1)
    loss = torch.sum(m3 * (ot - it) ** 2) * (1 / int(m3.count_nonzero())) * weight
    loss.backward()
    return loss.item(), s2.grad, ws1.grad


def temporal32(mode, a, b, c, d, mask, weight):
    return ftl32(a, b, mask, weight) if mode == 0 else otl32(a, b, c, d, mask, weight)


def tv32(s, weight):
    """oracle/reconet_ref.py:306-308 for one frame."""
    s = s.clone().requires_grad_(True)
    reg = (s[:, :, :-1, 1:] - s[:, :, :-1, :-1]) ** 2 + (s[:, :, 1:, :-1] - s[:, :, :-1, :-1]) ** 2
    loss = weight * torch.sum(reg)
    loss.backward()
    return loss.item(), s.grad


def tv_sqrt32(s, weight):
    s = s.clone().requires_grad_(True)
    r1 = (s[:, :, :-1, 1:] - s[:, :, :-1, :-1]) ** 2
    r2 = (s[:, :, 1:, :-1] - s[:, :, :-1, :-1]) ** 2
    loss = torch.sqrt((r1 + r2).clamp(min=1e-8)).mean() * weight
    loss.backward()
    return loss.item(), s.grad


def warp32(x, flo, gout=None):
    """R.warp and, with gout, its autograd backward."""
    x = x.clone().requires_grad_(True)
    y = R.warp(x, flo)
    if gout is None:
        return y.detach()
    y.backward(gout)
    return x.grad


def optim_adam(p, m, v, grads, first_step, dtype, gscale, lr, b1, b2, eps):
    """torch.optim.Adam in `dtype` from the given state; [(p, m, v) after each step]."""
    prm = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.Adam([prm], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[prm] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": m.to(dtype).clone(),
                      "exp_avg_sq": v.to(dtype).clone()}
    out = []
    for g in grads:
        prm.grad = g.to(dtype) * gscale
        opt.step()
        st = opt.state[prm]
        out.append((prm.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


# ------------------------------------------------------------------ the references against the oracle
def test_temporal_refs_match_oracle():
    for mode in (0, 1):
        shape = L.TEMPORAL_SHAPES[mode][0]
        for kind in ("binary", "signed"):
            args = L.temporal_case(mode, shape, kind)
            loss, count, ga, gb = L.temporal_ref(mode, *args)
            l32, ga32, gb32 = temporal32(mode, *args)
            assert _rel(loss, l32) < 1e-5 and _rel(ga, ga32) < 1e-5 and _rel(gb, gb32) < 1e-5, (mode, kind)
            mask = args[4]
            nnz = int((mask > 0).sum()) if mode == 0 else int((mask != 0).sum())
            assert count == shape[1] * nnz
    # the two modes differ on a signed mask exactly as the issue of their kernels says
    a, b, c, d, mask, w = L.temporal_case(1, (2, 3, 7, 9), "signed")
    assert (mask < 0).any() and (mask == 0).any() and ((mask > 0) & (mask < 1)).any()
    assert L.ftl(a, b, mask, w)[1] < L.otl(a, b, c, d, mask, w)[1]


def test_temporal_ref_zero_mask_is_defined_zero():
    for mode in (0, 1):
        for shape in L.TEMPORAL_SHAPES[mode]:
            loss, count, ga, gb = L.temporal_ref(mode, *L.temporal_case(mode, shape, "zero"))
            assert loss == 0.0 and count == 0 and not ga.any() and not gb.any()


def test_reduction_refs_match_oracle():
    a, b = L.mse_case("broadcast")
    loss, ga, _ = L.mse(a, b, 3.0)
    ar = a.clone().requires_grad_(True)
    ref = F.mse_loss(ar, b.expand_as(ar)) * 3.0
    ref.backward()
    assert _rel(loss, ref.item()) < 1e-5 and _rel(ga, ar.grad) < 1e-5
    s = L.tv_case((2, 3, 10, 13), True)
    for ref64, ref32 in ((L.tv, tv32), (L.tv_sqrt, tv_sqrt32)):
        l64, g64 = ref64(s, 0.5)
        l32, g32 = ref32(s, 0.5)
        assert _rel(l64, l32) < 1e-5 and _rel(g64, g32) < 1e-5
    assert not L.tv_sqrt(s, 0.5)[1][0, 0, :2, :2].any()  # the flat patch: the clamp's zero gradient
    x = L.sum_case(1003)
    assert _rel(L.sum_scaled(x, 0.25), float(x.sum()) * 0.25) < 1e-5


def test_adam_ref_matches_oracle_and_optim():
    p, m, v, grads, _ = L.adam_case(1.0)
    ref = L.adam(p, m, v, grads, L.ADAM_FIRST, **L.ADAM_HYPER)
    # the oracle's adam_step, float32, from the same state
    P = {"w": p.clone()}
    state = {"t": L.ADAM_FIRST - 1, "m_w": m.clone(), "v_w": v.clone()}
    for k, g in enumerate(grads):
        R.adam_step(P, {"w": g}, state)
        for got, want in zip((P["w"], state["m_w"], state["v_w"]), ref[k]):
            assert _rel(got, want) < 1e-5, k
    # torch.optim.Adam in float64: the same arithmetic up to float64 rounding
    for gscale in L.ADAM_GSCALES:
        p, m, v, grads, _ = L.adam_case(gscale)
        ref = L.adam(p, m, v, grads, L.ADAM_FIRST, gscale=gscale, **L.ADAM_HYPER)
        opt = optim_adam(p, m, v, grads, L.ADAM_FIRST, torch.float64, gscale, **L.ADAM_HYPER)
        for k in range(L.ADAM_K):
            for got, want in zip(opt[k], ref[k]):
                assert torch.allclose(got, want, rtol=1e-12, atol=1e-300), (gscale, k)


def test_warp_refs_match_oracle():
    for kind, shape in [("random", (2, 5, 12, 20)), ("random", (2, 3, 1, 7)), ("random", (1, 2, 9, 1)),
                        ("insertion", (1, 19, 10, 24))]:
        x, flo = L.warp_case(kind, shape)
        assert _rel(L.warp_fwd(x, flo)[0], warp32(x, flo)) < 1e-5, (kind, shape)
        assert _rel(L.warp_bwd(x, flo)[0], warp32(torch.zeros_like(x), flo, x)) < 1e-5, (kind, shape)
    idx, valid, w = L.warp_taps(L.warp_flow("random", (2, 5, 12, 20)), 12, 20)
    assert idx.shape == valid.shape == w.shape == (2, 4, 240) and w.dtype == torch.float64
    assert torch.allclose(w.sum(1), torch.ones(2, 240, dtype=torch.float64), atol=1e-12)  # the four weights sum to 1


def test_flow_mask_ref_matches_oracle():
    for shape in L.MASK_SHAPES:
        f01, f10 = L.mask_case(shape)
        err = L.flow_mask_err(f01, f10)
        assert err.shape == shape
        for b in range(shape[0]):
            wrong, _ = L.mask_check(R.flow_warp_mask(f01[b], f10[b], L.MASK_THR), err[b])
            assert wrong == 0, (shape, b)


def test_mask_guard_band_share():
    """The only GPU test that excludes elements: the share it excludes, from the reference alone."""
    for shape in L.MASK_SHAPES:
        err = L.flow_mask_err(*L.mask_case(shape))
        share = float((np.abs(err.numpy() - L.MASK_THR) <= L.MASK_BAND).mean())
        assert share <= L.MASK_BAND_SHARE, (shape, share)
        if err.numel() > 50:  # both outcomes occur
            assert 0 < int((err < L.MASK_THR).sum()) < err.numel(), shape


def test_norm_refs_match_oracle():
    for shape in L.NORM_SHAPES:
        x, gout, gscaled = L.norm_case(shape)
        out64, scaled64 = L.vgg_normalize(x)
        x0 = x.clone().requires_grad_(True)
        xs = x0 * 1.0
        out = R.vgg_normalize_(xs)
        assert _rel(out64, out.detach()) < 1e-5 and _rel(scaled64, xs.detach()) < 1e-5
        ((out * gout).sum() + (xs * gscaled).sum()).backward()
        assert _rel(L.vgg_normalize_bwd(gout, gscaled), x0.grad) < 1e-5
    gy, t = L.tanh_case()
    z = torch.atanh(t.double()).requires_grad_(True)  # ConvTanh, oracle/reconet_ref.py:64-66, from v = 255 z
    v = (255 * z)
    (torch.tanh(v / 255) * 150 + 255 / 2).backward(gy.double())
    assert _rel(L.tanh_out_bwd(gy, t, 0), z.grad / 255) < 1e-9


# ------------------------------------------------------------------ float32 renditions against the GPU tests' bounds
def _temporal_cases():
    for mode in (0, 1):
        for shape in L.TEMPORAL_SHAPES[mode]:
            for kind in L.TEMPORAL_MASKS:
                yield mode, shape, kind
        for kind in L.TEMPORAL_BIG_MASKS:
            yield mode, L.TEMPORAL_BIG[mode], kind


@pytest.mark.parametrize("mode,shape,kind", list(_temporal_cases()))
def test_temporal_float32_meets_bounds(mode, shape, kind):
    args = L.temporal_case(mode, shape, kind)
    loss, count, ga, gb = L.temporal_ref(mode, *args)
    if kind == "zero" or (mode == 0 and kind == "signed" and args[4].numel() == 1):  # (one negative pixel)
        assert count == 0
        return  # (the oracle's expression divides by zero here; the library's value is the reference's)
    assert count > 0
    l32, ga32, gb32 = temporal32(mode, *args)
    margins = (L.loss_margin(l32, loss), L.elem_margin(ga32, ga), L.elem_margin(gb32, gb))
    print(mode, shape, kind, "margins", margins)
    assert max(margins) <= 1.0, margins
    if kind == "tail":  # the whole result lies in the last 600 pixels
        assert count == shape[1] * 600 and not ga.reshape(shape[1], -1)[:, :-600].any()


@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse_float32_meets_bounds(name):
    a, b = L.mse_case(name)
    loss, ga, gb = L.mse(a, b, L.MSE_WEIGHT)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    l32 = F.mse_loss(ar, br.expand_as(ar)) * L.MSE_WEIGHT
    l32.backward()
    margins = (L.loss_margin(l32.item(), loss), L.elem_margin(ar.grad, ga), L.elem_margin(br.grad, gb))
    assert max(margins) <= 1.0, margins


@pytest.mark.parametrize("shape", L.TV_SHAPES)
def test_tv_float32_meets_bounds(shape):
    for ref64, ref32, flat in ((L.tv, tv32, False), (L.tv_sqrt, tv_sqrt32, True)):
        s = L.tv_case(shape, flat)
        l64, g64 = ref64(s, L.TV_WEIGHT)
        l32, g32 = ref32(s, L.TV_WEIGHT)
        margins = (L.loss_margin(l32, l64), L.elem_margin(g32, g64))
        print(shape, ref64.__name__, "margins", margins)
        assert max(margins) <= 1.0, (ref64.__name__, margins)
    n_terms = shape[0] * shape[1] * (shape[2] - 1) * (shape[3] - 1)
    assert (n_terms > 1024 * 256) == (shape == L.TV_SHAPES[-1])  # exactly the last shape is past one grid


@pytest.mark.parametrize("n", L.SUM_SIZES)
def test_sum_float32_meets_bounds(n):
    x = L.sum_case(n)
    assert L.loss_margin(float(x.sum() * L.SUM_WEIGHT), L.sum_scaled(x, L.SUM_WEIGHT)) <= 1.0


def test_adam_float32_meets_bounds_and_fixes_the_moment_bounds():
    """torch.optim.Adam in float32 against `adam`: meets the p bound; its normalised m / v errors are
    the measurement ADAM_M_BOUND / ADAM_V_BOUND are four times of."""
    worst_m = worst_v = 0.0
    for gscale in L.ADAM_GSCALES:
        p, m, v, grads, gmax = L.adam_case(gscale)
        ref = L.adam(p, m, v, grads, L.ADAM_FIRST, gscale=gscale, **L.ADAM_HYPER)
        got = optim_adam(p, m, v, grads, L.ADAM_FIRST, torch.float32, gscale, **L.ADAM_HYPER)
        for k in range(L.ADAM_K):
            mp, mm, mv = L.adam_margins(*got[k], ref[k], gmax, L.ADAM_K)
            assert max(mp, mm, mv) <= 1.0, (gscale, k, mp, mm, mv)
            em, ev = L.adam_moment_errors(got[k][1], got[k][2], ref[k], gmax)
            worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
    print(f"float32 torch.optim.Adam vs float64: m {worst_m:.3e}, v {worst_v:.3e}")
    assert L.ADAM_M_BOUND / 8 <= worst_m <= L.ADAM_M_BOUND / 4 * 1.05, worst_m
    assert L.ADAM_V_BOUND / 8 <= worst_v <= L.ADAM_V_BOUND / 4 * 1.05, worst_v
    p, m, v, grads, gmax = L.adam_first_case()
    ref = L.adam(p, m, v, grads, 1, **L.ADAM_HYPER)
    got = optim_adam(p, m, v, grads, 1, torch.float32, 1.0, **L.ADAM_HYPER)
    assert max(L.adam_margins(*got[0], ref[0], gmax, 1)) <= 1.0


@pytest.mark.parametrize("kind,shape", L.WARP_FWD_CASES)
def test_warp_fwd_float32_meets_bound(kind, shape):
    x, flo = L.warp_case(kind, shape)
    ref, A = L.warp_fwd(x, flo)
    assert L.warp_margin(warp32(x, flo), ref, A, 4) <= 1.0
    _, valid, w = L.warp_taps(flo, *shape[2:])
    if kind == "outside":  # all four taps out of bounds everywhere: the output is exactly 0
        assert not valid.any() and not ref.any()
    if kind == "integer":  # the sample sits exactly on an in-bounds pixel centre: a single-tap copy
        sx, sy = R._sample_coords(flo, *shape[2:])
        assert torch.equal(sx, sx.floor()) and torch.equal(sy, sy.floor())
        assert bool(valid[:, 0].all()) and torch.equal(w[:, 0], torch.ones_like(w[:, 0])) and not w[:, 1:].any()
        assert torch.equal(warp32(x, flo).double(), ref)


@pytest.mark.parametrize("kind,shape", L.WARP_BWD_CASES)
def test_warp_bwd_float32_meets_bound_and_reaches_its_tier(kind, shape):
    g, flo = L.warp_case(kind, shape)
    ref, A, n = L.warp_bwd(g, flo)
    assert L.warp_margin(warp32(torch.zeros_like(g), flo, g), ref, A, n) <= 1.0
    assert not ref.reshape(shape[0], shape[1], -1)[(n == 0).unsqueeze(1).expand(-1, shape[1], -1)].any()
    print(kind, shape, "longest list", int(n.max()), "lists of 9..16:", int(((n > L.WG_REG) & (n <= L.WG_NET)).sum()),
          "17..512:", int(((n > L.WG_NET) & (n <= L.WG_LONG)).sum()), "over 512:", int((n > L.WG_LONG).sum()))
    if kind == "mid":
        assert ((n > L.WG_REG) & (n <= L.WG_NET)).any() and ((n > L.WG_NET) & (n <= L.WG_LONG)).any()
    if kind == "insertion":
        assert (n > L.WG_LONG).any()
    if shape == L.WARP_TIER_CASES["scan"]:
        blocks = -(-n.numel() // L.WS_BLOCK)
        assert blocks > L.SCAN_CHUNK  # the totals scan takes a second chunk with a carry
        assert n.reshape(-1)[L.SCAN_CHUNK * L.WS_BLOCK:].any()  # ... and the pixels past it hold taps


def test_warp_atomic_cases_are_backward_cases():
    assert all(c in L.WARP_BWD_CASES for c in L.WARP_ATOMIC_CASES)


@pytest.mark.parametrize("shape", L.NORM_SHAPES)
def test_vgg_normalize_float32_meets_bounds(shape):
    x, gout, gscaled = L.norm_case(shape)
    out64, scaled64 = L.vgg_normalize(x)
    x0 = x.clone().requires_grad_(True)
    xs = x0 * 1.0
    out = R.vgg_normalize_(xs)
    ((out * gout).sum() + (xs * gscaled).sum()).backward()
    x1 = x.clone().requires_grad_(True)
    R.vgg_normalize_(x1 * 1.0).backward(gout)
    margins = (L.elem_margin(out.detach(), out64), L.elem_margin(xs.detach(), scaled64),
               L.elem_margin(x0.grad, L.vgg_normalize_bwd(gout, gscaled)),
               L.elem_margin(x1.grad, L.vgg_normalize_bwd(gout)))
    assert max(margins) <= 1.0, margins


@pytest.mark.parametrize("prenorm", [0, 1])
def test_tanh_out_bwd_float32_meets_bound(prenorm):
    gy, t = L.tanh_case()
    g = gy / torch.tensor(R.IMAGENET_STD).view(1, 3, 1, 1) / 255 if prenorm else gy
    assert L.elem_margin(g * 150 * (1 - t * t) / 255, L.tanh_out_bwd(gy, t, prenorm)) <= 1.0
    assert float(t.abs().max()) > 0.99
