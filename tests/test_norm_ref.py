"""CPU checks of tests/norm_ref.py, the float64 yardstick of tests/test_gpu_norm.py (no GPU):

  * `forward` / `backward` agree with float64 torch autograd of F.instance_norm + ReLU + residual, and
    `stats` with var(unbiased=False);
  * on every input the GPU tests use, the plain float32 form of each formula (fp64 moments, mean and
    rstd rounded to fp32, the rest fp32 torch) meets the bound the GPU test applies -- a bound the plain
    form missed would be a wrong bound or a wrong input, not a wrong kernel -- and the constants K_Y /
    K_G are 4x the worst ratio it reaches at K = 1, rounded up (the margins are printed);
  * the guard bands of the ReLU decision and of the tail's bytes hold at most 1 % of each case;
  * "const" planes have var == 0 exactly; `chunk_bounds` tiles a plane; every named shape lands on the
    kernel it is there for.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return R.case(shape, kind)


def _ids(cases):
    return [f"{s[2] * s[3]}-{k}" for s, k in cases]


# ------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 61, 68), (1, 2, 1, 4)])
@pytest.mark.parametrize("relu,with_res", R.RELU_RES)
def test_reference_vs_float64_autograd(shape, relu, with_res):
    c = _case(shape, "near")
    x, w, b, res = (c[k].double().requires_grad_(True) for k in ("x", "w", "b", "res"))
    y = F.instance_norm(x, weight=w, bias=b, eps=R.EPS)
    pre_t = y.detach().clone()
    if relu:
        y = torch.relu(y)
    if with_res:
        y = y + res
    y.backward(c["gy"].double())
    pre, y64 = R.forward(c["x"], c["w"], c["b"], relu, c["res"] if with_res else None)
    mask = (pre > 0) if relu else None
    assert bool((((pre_t > 0) == (pre > 0)) | (pre.abs() < 1e-12)).all())
    gx, gw, gb, gc = R.backward(c["gy"], c["x"], c["w"], mask)
    tol = 1e-12
    for name, a, r in (("y", y64, y.detach()), ("gx", gx, x.grad), ("gw", gw, w.grad), ("gb", gb, b.grad)):
        err = float((a - r).abs().max() / max(float(r.abs().max()), 1.0))
        assert err <= tol, (name, err)
    assert float(gc.abs().max()) <= 1e-9 * max(float(gx.abs().sum()), 1.0)
    if with_res:
        assert torch.equal(res.grad, c["gy"].double())


@pytest.mark.parametrize("shape", R.SHAPES[1:], ids=lambda s: str(s[2] * s[3]))
def test_stats_vs_var(shape):
    x = _case(shape, "near")["x"]
    mean, var, rstd = R.stats(x)
    v = x.double().flatten(2).var(2, unbiased=False).view(var.shape)
    assert float(((var - v).abs() / v).max()) <= 1e-11
    assert float((mean.flatten() - x.double().flatten(2).mean(2).flatten()).abs().max()) == 0.0
    assert torch.equal(rstd, 1.0 / torch.sqrt(var + R.EPS))


@pytest.mark.parametrize("hw", R.EDGE_HW)
def test_const_planes_have_zero_variance(hw):
    c = _case(R.BY_HW[hw], "const")
    mean, var, rstd = R.stats(c["x"])
    assert bool((var == 0).all()) and bool((mean == 1.5).all())
    assert bool((rstd == R.EPS ** -0.5).all())
    pre, y = R.forward(c["x"], c["w"], c["b"], relu=True)
    assert torch.equal(y, c["b"].double().clamp_min(0).view(1, -1, 1, 1).expand_as(y))
    mean32, rstd32 = R.plain_stats(c["x"])
    ppre, py = R.plain_forward(c["x"], c["w"], c["b"], relu=True)
    assert torch.equal(py, c["b"].clamp_min(0).view(1, -1, 1, 1).expand_as(py))


# ------------------------------------------------------------------ the plain float32 form meets every bound
def _plain_margins(shape, kind, K_y, K_g, K_gs):
    """{name: margin} of the plain float32 form over the four (relu, res) forwards and the two backward
    masks of one case, with its worst ReLU guard-band share."""
    c = _case(shape, kind)
    x, w, b, gy = c["x"], c["w"], c["b"], c["gy"]
    out = {"y": 0.0, "gx": 0.0, "gw": 0.0, "gb": 0.0, "gc_sum": 0.0, "gc_zero": 0.0, "band": 0.0, "wrong": 0}
    for relu, with_res in R.RELU_RES:
        res = c["res"] if with_res else None
        pre64, y64 = R.forward(x, w, b, relu, res)
        y_pre, Y = R.forward_bounds(x, w, b, relu, res, K=K_y)
        ppre, py = R.plain_forward(x, w, b, relu, res)
        out["y"] = max(out["y"], R.margin(py, y64, Y))
        if relu and not with_res:
            out["band"] = float(R.relu_band(pre64, y_pre).double().mean())
            out["wrong"] = R.relu_wrong(py, pre64, pre64.abs() > Y)
    _, py = R.plain_forward(x, w, b, True)
    for mask in (None, py > 0):
        gx64, gw64, gb64, _ = R.backward(gy, x, w, mask)
        GX, GW, GB = R.backward_bounds(gy, x, w, mask, K=K_g, K_shift=K_gs)
        gx, gw, gb, gc = R.plain_backward(gy, x, w, mask)
        out["gx"] = max(out["gx"], R.margin(gx, gx64, GX))
        out["gw"] = max(out["gw"], R.margin(gw, gw64, GW))
        out["gb"] = max(out["gb"], R.margin(gb, gb64, GB))
        out["gc_sum"] = max(out["gc_sum"], R.margin(gc, gx.double().sum((0, 2, 3)), R.gc_sum_bound(gx)))
        out["gc_zero"] = max(out["gc_zero"], R.margin(gc, torch.zeros_like(gw64), GX.sum((0, 2, 3))))
    return out


@functools.lru_cache(maxsize=None)
def _all_plain(K_y, K_g, K_gs):
    return {(s, k): _plain_margins(s, k, K_y, K_g, K_gs) for s, k in R.CASES}


@pytest.mark.parametrize("shape,kind", R.CASES, ids=_ids(R.CASES))
def test_plain_float32_form_meets_bounds(shape, kind):
    m = _all_plain(R.K_Y, R.K_G, R.K_GS)[(shape, kind)]
    print(shape, kind, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in m.items()})
    assert max(m[k] for k in ("y", "gx", "gw", "gb", "gc_sum", "gc_zero")) <= 1.0, m
    assert m["wrong"] == 0 and m["band"] <= R.BAND_SHARE, m


def test_constants_are_four_times_the_plain_forms_ratio():
    """K = 4 x (worst error / bound at K = 1), rounded up to one significant digit: asserted as
    K / 8 < ratio <= K / 4 (a rounding up never doubles).  Each form of GX is measured alone."""
    def worst(name, *Ks):
        return max((m[name], key) for key, m in _all_plain(*Ks).items())

    got = {"K_Y": worst("y", 1.0, 1.0, None), "K_G": worst("gx", 1.0, 1.0, None), "K_GS": worst("gx", 1.0, None, 1.0)}
    print("worst error / (bound at K = 1):", got, "-> K_Y", R.K_Y, "K_G", R.K_G, "K_GS", R.K_GS)
    for name, (ratio, _) in got.items():
        K = getattr(R, name)
        assert K / 8 < ratio <= K / 4, (name, got)


# ------------------------------------------------------------------ split-plane apply and the fused tail
@pytest.mark.parametrize("shape,S", R.APPLY_CASES)
def test_apply_inputs_meet_bound_and_band(shape, S):
    """The split-plane apply computes the same formula: its inputs under the same bound."""
    x, w, b, res = R.apply_case(shape)
    for relu, with_res in R.RELU_RES:
        r = res if with_res else None
        pre64, y64 = R.forward(x, w, b, relu, r)
        y_pre, Y = R.forward_bounds(x, w, b, relu, r)
        m = R.margin(R.plain_forward(x, w, b, relu, r)[1], y64, Y)
        assert m <= 1.0, (relu, with_res, m)
        assert float(R.relu_band(pre64, y_pre).double().mean()) <= R.BAND_SHARE


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("shape", sorted({s for s, _ in R.TAIL_CASES}))
def test_tail_bytes_band(shape, bgr):
    z, w, b = R.tail_case(shape)
    img, want = R.tanh_frames(z, w, b, bgr)
    wrong, band, differing = R.frames_check(R.plain_tanh_frames(z, w, b, bgr), img, R.frame_dimg(z, w, b, bgr))
    print(shape, bgr, "wrong", wrong, "band share", band, "differing", differing)
    assert wrong == 0 and band <= R.BAND_SHARE
    assert len(torch.unique(want)) >= 50  # not a trivial image
    # the layout: HWC, channel c of pixel p, reversed if bgr
    pre, _ = R.forward(z, w, b)
    c, n, p = 2, shape[0] - 1, shape[2] * shape[3] - 1
    v = float(((torch.tanh(pre[n, c].flatten()[p]) + 1) / 2 * 255).clamp(0, 255))
    assert int(want[n].view(-1, 3)[p, (2 - c) if bgr else c]) == int(v)


def test_chunk_bounds_tile_the_plane():
    cases = {(s[2] * s[3], S) for s, S in R.APPLY_CASES} | {(s[2] * s[3], S or 1) for s, S in R.TAIL_CASES}
    assert (8, 7) in cases
    for HW, S in sorted(cases):
        b = [R.chunk_bounds(HW, S, k) for k in range(S)]
        assert b[0][0] == 0 and b[-1][1] == HW
        assert all(lo <= hi for lo, hi in b) and all(b[k][1] == b[k + 1][0] for k in range(S - 1))
        if HW % 4 == 0:
            assert all(lo % 4 == 0 and hi % 4 == 0 for lo, hi in b)
    assert sum(lo == hi for lo, hi in (R.chunk_bounds(8, 7, k) for k in range(7))) == 5  # five empty chunks


# ------------------------------------------------------------------ channel_sum
@pytest.mark.parametrize("shape", R.CSUM_SHAPES)
def test_channel_sum_plain_form(shape):
    x, old = R.csum_case(shape)
    ref = R.channel_sum(x)
    m = (R.margin(x.double().sum((0, 2)).float(), ref, R.channel_sum_bound(x, ref)),
         R.margin(old + x.double().sum((0, 2)).float(), old.double() + ref, R.channel_sum_bound(x, ref, old)))
    print(shape, m)
    assert max(m) <= 1.0
    assert float((ref / (x.shape[0] * x.shape[2])).min()) > 1.0  # mean 3: a dropped element shows


# ------------------------------------------------------------------ routes
def test_named_shapes_land_on_their_routes():
    """The host conditions of vst_instnorm_fwd / vst_instnorm_bwd (norm_ref.FWD_ROUTES / BWD_ROUTES: the
    HW % 4 test, the 8192 and 32768 limits) put every named shape on the kernel it is there for.  If a
    limit moves, this says which shapes to move."""
    assert sorted(R.INTENDED) == sorted(R.BY_HW)
    for hw, (fwd, bwd, body) in R.INTENDED.items():
        assert R.route(R.FWD_ROUTES, hw) == (fwd, body), hw
        assert R.route(R.BWD_ROUTES, hw) == (bwd, body), hw
    lim = sorted({r[2] for r in R.FWD_ROUTES + R.BWD_ROUTES if r[2]})
    for L in lim:  # a shape exactly on each limit and on the first vector size past it
        assert L in R.BY_HW and L + 4 in R.BY_HW
    for hw in R.MISALIGNED_HW:  # off a 16-byte boundary every size takes the scalar two-pass body
        assert R.route(R.FWD_ROUTES, hw, aligned=False) == ("in_fwd_kernel<1024>", "scalar")
        assert R.route(R.BWD_ROUTES, hw, aligned=False) == ("in_bwd_kernel<1024>", "scalar")
    assert {R.route(R.BWD_ROUTES, hw)[0] for hw in R.ACC_HW} == {r[0] for r in R.BWD_ROUTES}
    assert max(s[0] * s[1] * s[2] * s[3] for s in R.SHAPES) <= 196608
