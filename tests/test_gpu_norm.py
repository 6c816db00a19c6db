"""The InstanceNorm and channel-sum kernels (csrc/norm.hip) against the float64 references of
tests/norm_ref.py, on a real MI355X.

Every comparison is with the float64 reference, never with another kernel, except three bitwise
identities the library promises: the two ReLU-mask modes of the backward give the same gx (what
`in_affine` exists for), a zero residual leaves the ReLU part unchanged, and VST_IN_YMASK's route gives
the default route's y and gx.  The inputs, the bounds and their derivations live in tests/norm_ref.py;
tests/test_norm_ref.py shows on the CPU that the plain float32 form of each formula meets every bound
applied here on these very inputs, that the guard bands hold at most 1 % of a case, and that each shape
lands on the kernel it is there for.  A margin is error / bound: <= 1 passes.

The C entries are called through vst._lib where that makes a route or a mask mode reachable without an
environment switch, and every output of such a call is filled with NaN first and must be finite after:
each element and each partial is written.

Shapes (norm_ref.SHAPES, by HW): 1 (var = 0), 4 (one float4), 35 (scalar two-pass, HW < threads),
4148 (third register slot partly filled), 8192 (register route full), 8196 (first size on the
<1024,8> forward and the LDS backward), 32768 (LDS route full), 32772 (float4 two-pass, thread 0 alone
takes the tail), 32761 (scalar two-pass, several strides), 36864 (float4 two-pass, the second load of
thread 0's last pair would be one float4 past the plane); N = 2, C = 3 where the size allows, so a
channel taken as plane / C, or a plane as n alone, reads another w and b.  "offset" planes (mean = 50
std) and "const" planes (var == 0 exactly) run at one shape per kernel body.

The recomputed ReLU mask: random inputs never reach the elements where the rounding order of the
pre-activation decides its sign (a backward kernel with a separate multiply and add in place of
`in_affine`'s fma passed every other test here), so test_recomputed_mask_has_the_forwards_sign plants them.

Misaligned tensors: `ops._check` and `.contiguous()` pass a contiguous view into a larger buffer on as
it is, so a tensor that starts one float past a 16-byte boundary does reach vst_instnorm_fwd / _bwd with
HW % 4 == 0.  The float4 forms there took the pointers as given; the routes and the two-pass kernels
now ask for 16-byte alignment like vst_channel_sum and vst_instnorm_apply, and such tensors take the
scalar two-pass body.  test_forward_misaligned / test_backward_misaligned run them at 35 and 32761 and,
with HW % 4 == 0, at one size per vector route (4148, 8196, 32772), and look at the floats around the
output for a store past its ends.
"""
import functools

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def G(t):
    return None if t is None else t.to(DEV)


def C(t):
    return t.detach().cpu()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _ids(cases):
    return [f"{s[2] * s[3]}-{k}" for s, k in cases]


def _p(t):
    from vst._lib import ptr

    return ptr(t)


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(CPU inputs, their device copies)."""
    c = R.case(shape, kind)
    return c, {k: G(v) for k, v in c.items()}


def _fwd(x, w, b, res, relu, y=None):
    """vst_instnorm_fwd into NaN-filled y and stats."""
    from vst._lib import lib, stream

    N, Cc, H, W = x.shape
    y = _nan(*x.shape) if y is None else y
    stats = _nan(N * Cc * 2)
    lib.vst_instnorm_fwd(_p(x), _p(w), _p(b), _p(res), _p(y), _p(stats), N, Cc, H * W, R.EPS, int(relu), stream())
    return y, stats


def _bwd(gy, x, y, b, stats, w, relu, gx=None, want_gc=True, accumulate=0, into=None):
    """vst_instnorm_bwd into NaN-filled gx, gw, gb, gc and partials (or accumulating into `into`)."""
    from vst._lib import lib, stream

    N, Cc, H, W = x.shape
    gx = _nan(*x.shape) if gx is None else gx
    gw, gb, gc = into if into is not None else (_nan(Cc), _nan(Cc), _nan(Cc) if want_gc else None)
    part = _nan(N * Cc * 3)
    lib.vst_instnorm_bwd(_p(gy), _p(x), _p(y), _p(b), _p(stats), _p(w), _p(gx), _p(gw), _p(gb), _p(gc), _p(part),
                         N, Cc, H * W, int(relu), accumulate, stream())
    assert _finite(part)
    return gx, gw, gb, gc


def _stats_margins(stats, x):
    mean, _, rstd = R.stats(x)
    dm, dr = R.stats_bounds(x)
    s = C(stats).view(*mean.shape[:2], 2)
    return (R.margin(s[..., 0], mean.view(s.shape[:2]), dm.view(s.shape[:2])),
            R.margin(s[..., 1], rstd.view(s.shape[:2]), dr.view(s.shape[:2])))


# ------------------------------------------------------------------ 1. forward
@functools.lru_cache(maxsize=None)
def _fwd_relu_plain(shape, kind):
    """The forward with ReLU and no residual of a case: (y, stats) on the device.  Its y > 0 is the mask
    the backward tests give the float64 reference."""
    _, d = _case(shape, kind)
    return _fwd(d["x"], d["w"], d["b"], None, True)


@pytest.mark.parametrize("relu,with_res", R.RELU_RES)
@pytest.mark.parametrize("shape,kind", R.CASES, ids=_ids(R.CASES))
def test_forward(shape, kind, relu, with_res):
    c, d = _case(shape, kind)
    res = c["res"] if with_res else None
    y, stats = _fwd(d["x"], d["w"], d["b"], d["res"] if with_res else None, relu)
    assert _finite(y, stats)
    pre64, y64 = R.forward(c["x"], c["w"], c["b"], relu, res)
    _, Y = R.forward_bounds(c["x"], c["w"], c["b"], relu, res)
    margins = dict(zip(("mean", "rstd"), _stats_margins(stats, c["x"])), y=R.margin(C(y), y64, Y))
    print("MARGIN forward", shape, kind, relu, with_res, margins)
    assert max(margins.values()) <= 1.0, margins
    if kind == "const" and not with_res:  # var == 0 exactly: xhat == 0 and y is b (or max(b, 0)) bit for bit
        want = c["b"].clamp_min(0) if relu else c["b"]
        assert torch.equal(C(y), want.view(1, -1, 1, 1).expand(shape))
    if relu:
        y_pre, Y0 = R.forward_bounds(c["x"], c["w"], c["b"], True, None)
        sure = pre64.abs() > Y0
        y0 = y if not with_res else _fwd_relu_plain(shape, kind)[0]
        assert R.relu_wrong(C(y0), pre64, sure) == 0
        assert float(R.relu_band(pre64, y_pre).double().mean()) <= R.BAND_SHARE
        if with_res:  # a zero residual leaves the ReLU part as it is, bit for bit
            yz, _ = _fwd(d["x"], d["w"], d["b"], torch.zeros_like(d["x"]), True)
            assert torch.equal(yz, y0)


@pytest.mark.parametrize("hw", R.MISALIGNED_HW)
def test_forward_misaligned(hw):
    """x, res and y each one float past a 16-byte boundary (see the module docstring)."""
    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    (x, _), (res, _) = R.misaligned(d["x"]), R.misaligned(d["res"])
    y, ybuf = R.misaligned(_nan(*shape))
    assert x.data_ptr() % 16 == 4 and res.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 4
    _, stats = _fwd(x, d["w"], d["b"], res, True, y=y)
    assert _finite(y, stats) and R.untouched_around(ybuf, y.numel())
    _, y64 = R.forward(c["x"], c["w"], c["b"], True, c["res"])
    _, Y = R.forward_bounds(c["x"], c["w"], c["b"], True, c["res"])
    margins = dict(zip(("mean", "rstd"), _stats_margins(stats, c["x"])), y=R.margin(C(y), y64, Y))
    print("MARGIN forward", shape, "misaligned", margins)
    assert max(margins.values()) <= 1.0, margins


# ------------------------------------------------------------------ 2. backward
def _bwd_margins(c, mask, gx, gw, gb, gc, old=None):
    """Margins of one backward against the float64 reference.  old: (gw, gb, gc) the call accumulated
    into -- the result is old + ref within the same bound plus one ulp of the sum."""
    gx64, gw64, gb64, _ = R.backward(c["gy"], c["x"], c["w"], mask)
    GX, GW, GB = R.backward_bounds(c["gy"], c["x"], c["w"], mask)
    m = {"gx": R.margin(C(gx), gx64, GX)}
    o = [torch.zeros(len(c["w"]), dtype=torch.float64)] * 3 if old is None else [t.double() for t in old]
    ulp = (lambda ref, k: R.ulp_sum(o[k], ref)) if old is not None else (lambda ref, k: 0.0)
    if gw is not None:
        m["gw"] = R.margin(C(gw), o[0] + gw64, GW + ulp(gw64, 0))
        m["gb"] = R.margin(C(gb), o[1] + gb64, GB + ulp(gb64, 1))
    if gc is not None:
        wrote = C(gx).double().sum((0, 2, 3))  # what the kernel wrote, summed in float64
        m["gc_sum"] = R.margin(C(gc), o[2] + wrote, R.gc_sum_bound(C(gx)) + ulp(wrote, 2))
        zero = torch.zeros_like(wrote)
        m["gc_zero"] = R.margin(C(gc), o[2] + zero, GX.sum((0, 2, 3)) + ulp(zero, 2))
    return m


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,kind", R.CASES, ids=_ids(R.CASES))
def test_backward(shape, kind, relu):
    """No ReLU; with ReLU both mask modes (from y, and recomputed from x and b through `in_affine`): each
    within the bounds, and the two bitwise equal.  The mask given to the reference is the GPU forward's own
    y > 0, so no comparison depends on a decision near zero."""
    c, d = _case(shape, kind)
    if relu:
        y, stats = _fwd_relu_plain(shape, kind)
        mask = C(y) > 0
    else:
        y, stats = _fwd(d["x"], d["w"], d["b"], None, False)
        mask = None
    outs = []
    for mode in (("ymask", "amask") if relu else ("none",)):
        gx, gw, gb, gc = _bwd(d["gy"], d["x"], y if mode == "ymask" else None, d["b"], stats, d["w"], relu)
        assert _finite(gx, gw, gb, gc), mode
        m = _bwd_margins(c, mask, gx, gw, gb, gc)
        print("MARGIN backward", shape, kind, mode, m)
        assert max(m.values()) <= 1.0, (mode, m)
        outs.append((gx, gw, gb, gc))
    if relu:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    # without gbias_prev the other two results are unchanged
    gx, gw, gb, _ = _bwd(d["gy"], d["x"], None, d["b"], stats, d["w"], relu, want_gc=False)
    m = _bwd_margins(c, mask, gx, gw, gb, None)
    assert _finite(gx, gw, gb) and max(m.values()) <= 1.0, m


@pytest.mark.parametrize("hw", R.MISALIGNED_HW)
def test_backward_misaligned(hw):
    """gy, x, y and gx each one float past a 16-byte boundary, mask from y."""
    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    y0, stats = _fwd_relu_plain(shape, "near")
    (gy, _), (x, _), (y, _) = (R.misaligned(t) for t in (d["gy"], d["x"], y0))
    gx, gxbuf = R.misaligned(_nan(*shape))
    _, gw, gb, gc = _bwd(gy, x, y, d["b"], stats, d["w"], True, gx=gx)
    assert _finite(gx, gw, gb, gc) and R.untouched_around(gxbuf, gx.numel())
    m = _bwd_margins(c, C(y0) > 0, gx, gw, gb, gc)
    print("MARGIN backward", shape, "misaligned", m)
    assert max(m.values()) <= 1.0, m


@pytest.mark.parametrize("hw", R.ACC_HW)
def test_recomputed_mask_has_the_forwards_sign(hw):
    """Elements planted where the rounding order of the pre-activation decides the ReLU: with t = fl(fl(x0 -
    mean) rstd) from the forward's own fp32 statistics and b = -fl(t w), `in_affine`'s fma gives the exact
    residual t w - fl(t w) (x0 is searched until that is positive: y > 0), a separate multiply and add give
    0 (no gradient).  Random inputs never land there; a backward that recomputed the mask in another
    rounding order than the forward would differ from the mask-from-y mode on every planted element."""
    import numpy as np

    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    N, Cc = shape[:2]
    idx = torch.arange(3, hw, 8)
    w32 = c["w"].numpy()
    centre = c["x"][0].flatten(1).mean(1)
    zero_b = torch.zeros(Cc, device=DEV)

    def planted(x0):
        x = c["x"].clone()
        x[0].flatten(1)[:, idx] = x0[:, None]
        return x

    chosen = {}
    for k in range(64):
        x0 = (centre + 0.25 + k / 64).float()
        _, stats = _fwd(G(planted(x0)), d["w"], zero_b, None, True)
        st = C(stats).view(N, Cc, 2)[0].numpy()
        t = (x0.numpy() - st[:, 0]) * st[:, 1]  # fp32, the order of in_affine
        p = t * w32
        r = t.astype(np.float64) * w32.astype(np.float64) - p.astype(np.float64)  # exact
        for ch in range(Cc):
            if ch not in chosen and r[ch] > 0:
                chosen[ch] = (float(x0[ch]), float(p[ch]), float(r[ch]))
        if len(chosen) == Cc:
            break
    assert len(chosen) == Cc, chosen
    x = planted(torch.tensor([chosen[ch][0] for ch in range(Cc)]))
    b = torch.tensor([-chosen[ch][1] for ch in range(Cc)])
    cc = dict(c, x=x, b=b)
    xd, bd = G(x), G(b)
    y, stats = _fwd(xd, d["w"], bd, None, True)
    got = C(y)[0].flatten(1)[:, idx].double()
    want = torch.tensor([chosen[ch][2] for ch in range(Cc)], dtype=torch.float64)[:, None].expand_as(got)
    assert torch.equal(got, want), "the forward is not fl(t w + b) in one rounding on the planted elements"
    mask = C(y) > 0
    outs = []
    for y_arg in (y, None):
        gx, gw, gb, gc = _bwd(d["gy"], xd, y_arg, bd, stats, d["w"], True)
        m = _bwd_margins(cc, mask, gx, gw, gb, gc)
        print("MARGIN backward", shape, "planted", "ymask" if y_arg is not None else "amask", m)
        assert _finite(gx, gw, gb, gc) and max(m.values()) <= 1.0, m
        outs.append((gx, gw, gb, gc))
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[0], outs[1]))


# ------------------------------------------------------------------ 3. accumulate
def _old(Cc, *key):
    g = R._gen("old", Cc, *key)
    return [5.0 * torch.randn(Cc, generator=g) for _ in range(3)]


@pytest.mark.parametrize("hw", R.ACC_HW)
def test_backward_accumulates(hw):
    """accumulate = 1 adds to gw, gb and gbias_prev (one shape per backward kernel)."""
    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    y, stats = _fwd_relu_plain(shape, "near")
    old = _old(shape[1], hw)
    into = [G(t) for t in old]
    gx, gw, gb, gc = _bwd(d["gy"], d["x"], None, d["b"], stats, d["w"], True, accumulate=1, into=into)
    m = _bwd_margins(c, C(y) > 0, gx, gw, gb, gc, old=old)
    print("MARGIN accumulate", shape, m)
    assert _finite(gx, gw, gb, gc) and max(m.values()) <= 1.0, m
    assert all(float((C(t) - o).abs().max()) > 0.01 for t, o in zip((gw, gb), old))  # something was added


@pytest.mark.parametrize("have", ["both", "weight_only"])
@pytest.mark.parametrize("hw", [35, 8192])
def test_autograd_grad_sinks(hw, have):
    """ops.instance_norm with leaf w, b: with both .grad buffers present the kernel accumulates into them
    (`grad_sink`), with one missing autograd adds the kernel's stored result; either way the gradients are
    old + ref, and a second backward adds again."""
    from vst import ops

    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    old = _old(shape[1], hw, have)
    w, b = d["w"].clone().requires_grad_(True), d["b"].clone().requires_grad_(True)
    w.grad = G(old[0])
    if have == "both":
        b.grad = G(old[1])
        assert ops.grad_sink(w) is w.grad and ops.grad_sink(b) is b.grad
    else:
        old[1] = torch.zeros_like(old[1])
        assert ops.grad_sink(b) is None
    x = d["x"].clone().requires_grad_(True)
    y = ops.instance_norm(x, w, b, relu=True)
    mask = C(y) > 0
    _, gw64, gb64, _ = R.backward(c["gy"], c["x"], c["w"], mask)
    _, GW, GB = R.backward_bounds(c["gy"], c["x"], c["w"], mask)
    for k in (1, 2):
        y.backward(d["gy"], retain_graph=True)
        m = {"gw": R.margin(C(w.grad), old[0].double() + k * gw64, k * (GW + R.ulp_sum(old[0], k * gw64))),
             "gb": R.margin(C(b.grad), old[1].double() + k * gb64, k * (GB + R.ulp_sum(old[1], k * gb64)))}
        print("MARGIN accumulate", shape, have, "backward", k, m)
        assert max(m.values()) <= 1.0, (k, m)
    assert _finite(x.grad)


@pytest.mark.parametrize("have", ["all", "no_conv_bias_grad"])
def test_conv_instance_norm_bias_gradient(have):
    """The conv bias feeding an InstanceNorm has gradient sum(gx) = 0: within the gc bound of 0, and an
    existing .grad of it is otherwise unchanged.  The conv's own output (read back from the GPU) is the
    norm's input here, for the bound only."""
    from vst import ops

    g = R._gen("convin", have)
    x = torch.randn(2, 3, 8, 10, generator=g)
    cw = torch.randn(4, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    cb = torch.randn(4, generator=g)
    gamma, beta = R.affine(4, "convin")
    gy = torch.randn(2, 4, 8, 10, generator=g)
    old = _old(4, "convin", have)
    xd, cwd = G(x), G(cw)
    cbd, gd, bd = (G(t).requires_grad_(True) for t in (cb, gamma, beta))
    gd.grad, bd.grad = G(old[0]), G(old[1])
    if have == "all":
        cbd.grad = G(old[2])
    else:
        old[2] = torch.zeros(4)
    with torch.no_grad():
        z = C(ops.Conv2dFn.apply(xd, cwd, None, 1, 1, "reflect", 1, None, cbd.detach()))
    y = ops.conv_instance_norm(xd, cwd, cbd, gd, bd, 1, 1, "reflect", 1, relu=True)
    y.backward(G(gy))
    mask = C(y) > 0
    _, gw64, gb64, _ = R.backward(gy, z, gamma, mask)
    GX, GW, GB = R.backward_bounds(gy, z, gamma, mask)
    zero = torch.zeros(4, dtype=torch.float64)
    m = {"gw": R.margin(C(gd.grad), old[0].double() + gw64, GW + R.ulp_sum(old[0], gw64)),
         "gb": R.margin(C(bd.grad), old[1].double() + gb64, GB + R.ulp_sum(old[1], gb64)),
         "gc_zero": R.margin(C(cbd.grad), old[2].double(), GX.sum((0, 2, 3)) + R.ulp_sum(old[2], zero))}
    print("MARGIN accumulate conv_instance_norm", have, m)
    assert max(m.values()) <= 1.0, m


# ------------------------------------------------------------------ 4. plain, and the mask from y, through Python
@pytest.mark.parametrize("hw", [35, 8196])
def test_instance_norm_plain(hw):
    """adaattn's instance_norm_plain: the affine kernels with the constants w = 1, b = 0."""
    from vst.adaattn.attention import instance_norm_plain

    shape = R.BY_HW[hw]
    c, d = _case(shape, "near")
    one, zero = torch.ones(shape[1]), torch.zeros(shape[1])
    x = d["x"].clone().requires_grad_(True)
    y = instance_norm_plain(x)
    y.backward(d["gy"])
    _, y64 = R.forward(c["x"], one, zero)
    _, Y = R.forward_bounds(c["x"], one, zero)
    gx64, *_ = R.backward(c["gy"], c["x"], one)
    GX, _, _ = R.backward_bounds(c["gy"], c["x"], one)
    m = {"y": R.margin(C(y), y64, Y), "gx": R.margin(C(x.grad), gx64, GX)}
    print("MARGIN forward plain", shape, m)
    assert max(m.values()) <= 1.0, m


@pytest.mark.parametrize("hw", [8192, 8196])
def test_ymask_route_is_bitwise_the_default(hw, monkeypatch):
    """ops._IN_YMASK (VST_IN_YMASK=1: the backward reads the ReLU mask from the saved y) gives the
    default route's y and gx bit for bit."""
    from vst import ops

    shape = R.BY_HW[hw]
    _, d = _case(shape, "near")
    runs = []
    for ymask in (False, True):
        monkeypatch.setattr(ops, "_IN_YMASK", ymask)
        x = d["x"].clone().requires_grad_(True)
        y = ops.instance_norm(x, d["w"], d["b"], relu=True)
        assert (y.grad_fn.saved_tensors[1] is not None) == ymask
        y.backward(d["gy"])
        runs.append((y.detach(), x.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert int((runs[0][0] > 0).sum()) > 0 and int((runs[0][0] == 0).sum()) > 0


# ------------------------------------------------------------------ 5. split-plane apply
def _apply(x, w, b, res, relu, S, y=None):
    """vst_instnorm_moments + vst_instnorm_apply into NaN-filled partials, y and stats."""
    from vst._lib import lib, stream

    N, Cc, H, W = x.shape
    part = _nan(N * Cc * S * 2, dtype=torch.float64)
    lib.vst_instnorm_moments(_p(x), part.data_ptr(), N * Cc, H * W, S, stream())
    y = _nan(*x.shape) if y is None else y
    stats = _nan(N * Cc * 2)
    lib.vst_instnorm_apply(_p(x), part.data_ptr(), _p(w), _p(b), _p(res), _p(y), _p(stats), N, Cc, H * W, S, R.EPS,
                           int(relu), stream())
    assert _finite(part)  # an empty chunk's partial is a written zero
    return y, stats


def _apply_check(tag, x, w, b, res, relu, y, stats):
    pre64, y64 = R.forward(x, w, b, relu, res)
    y_pre, Y = R.forward_bounds(x, w, b, relu, res)
    margins = {"y": R.margin(C(y), y64, Y)}
    if stats is not None:
        margins.update(zip(("mean", "rstd"), _stats_margins(stats, x)))
    print("MARGIN apply", *tag, margins)
    assert max(margins.values()) <= 1.0, margins
    if relu and res is None:
        assert R.relu_wrong(C(y), pre64, pre64.abs() > Y) == 0


@pytest.mark.parametrize("relu,with_res", R.RELU_RES)
@pytest.mark.parametrize("shape,S", R.APPLY_CASES)
def test_split_apply_vs_float64(shape, S, relu, with_res):
    """(1, 2, 1, 8) with S = 7: n4 = 2, five of the seven chunks are empty; S = 256: almost all are."""
    from vst import ops

    x, w, b, res = R.apply_case(shape)
    res = res if with_res else None
    xd, wd, bd, rd = G(x), G(w), G(b), G(res)
    y, stats = _apply(xd, wd, bd, rd, relu, S)
    assert _finite(y, stats)
    _apply_check((shape, S, relu, with_res), x, w, b, res, relu, y, stats)
    assert ops.IN_SPLIT
    y = ops.instance_norm_infer(xd, wd, bd, relu=relu, res=rd, chunks=S)
    _apply_check((shape, S, relu, with_res, "ops"), x, w, b, res, relu, y, None)


def test_split_apply_misaligned_residual():
    """A residual one float past a 16-byte boundary: the scalar body at HW % 4 == 0."""
    shape, S = R.APPLY_MISALIGNED
    x, w, b, res = R.apply_case(shape)
    rd, _ = R.misaligned(G(res))
    y, stats = _apply(G(x), G(w), G(b), rd, True, S)
    assert _finite(y, stats)
    _apply_check((shape, S, "misaligned res"), x, w, b, res, True, y, stats)


# ------------------------------------------------------------------ 6. fused tail
@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("shape,S", R.TAIL_CASES)
def test_fused_tail_vs_float64(shape, S, bgr):
    """Every byte is trunc of the float64 image value, except that a value within dimg of an integer (at
    most 1 % of a case) may give the neighbouring byte.  (1, 3, 33, 257): HW % 4 != 0, the byte path with
    several strides; S = None: the host rule keeps these sizes on vst_instnorm_fwd and two more kernels."""
    from vst import ops

    z, w, b = R.tail_case(shape)
    frames = torch.full((shape[0], shape[2], shape[3], 3), 77, dtype=torch.uint8, device=DEV)
    out = ops.instance_norm_tanh_frames(G(z), G(w), G(b), bgr=bgr, frames=frames, chunks=S)
    assert out is frames
    img, _ = R.tanh_frames(z, w, b, bgr)
    wrong, band, differing = R.frames_check(frames, img, R.frame_dimg(z, w, b, bgr))
    print("MARGIN bytes", shape, S, bgr, {"wrong": wrong, "band": band, "differing": differing})
    assert wrong == 0 and band <= R.BAND_SHARE


# ------------------------------------------------------------------ 7. channel_sum
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("shape", R.CSUM_SHAPES)
def test_channel_sum(shape, aligned):
    """vst_channel_sum storing into a NaN-filled out, and ops.channel_sum accumulating into a given one;
    off a 16-byte boundary the scalar kernel runs at HW % 4 == 0 too."""
    from vst import ops
    from vst._lib import lib, stream

    N, Cc, HW = shape
    x, old = R.csum_case(shape)
    ref = R.channel_sum(x)
    xd = G(x) if aligned else R.misaligned(G(x))[0]
    assert (xd.data_ptr() % 16 == 0) == aligned
    out, part = _nan(Cc), _nan(N * Cc, dtype=torch.float64)
    lib.vst_channel_sum(_p(xd), _p(out), part.data_ptr(), N, Cc, HW, 0, stream())
    assert _finite(out, part)
    acc = G(old).clone()
    assert ops.channel_sum(xd.view(N, Cc, 1, HW), out=acc) is acc
    m = {"store": R.margin(C(out), ref, R.channel_sum_bound(x, ref)),
         "accumulate": R.margin(C(acc), old.double() + ref, R.channel_sum_bound(x, ref, old)),
         "ops": R.margin(C(ops.channel_sum(xd.view(N, Cc, 1, HW))), ref, R.channel_sum_bound(x, ref))}
    print("MARGIN channel_sum", shape, aligned, m)
    assert max(m.values()) <= 1.0, m
