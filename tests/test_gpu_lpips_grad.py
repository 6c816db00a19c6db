"""The gradient of LPIPS on the GPU (`vst_lpips_head_bwd`, `vst.lpips.LPIPS.distance_to`, `PerceptualLoss`)
against the float64 references of tests/lpips_grad_ref.py.

Bars.  The fused head backward is held to the bar of tests/test_gpu_lpips.py (`_bar`): the worst element
at most max(4 x the fp32 torch-autograd gradient's distance from float64, 1e-6 x the scale), applied
separately to the ordinary pixels and to each adversarial pixel class of `lpips_ref.head_inputs`, so the
1e10-sized gradients of a half-zero pixel do not set the floor for the rest.  Where torch's gradient is
NaN (a zero norm) the comparison is with the closed form's finite limit and the bar is the 1e-6 floor
alone: there dA_c = (w_c gs) (b_c rb) ra is a product of rounded fp32 factors, each within 2^-24, times
rb's own error (a tree-summed sum of squares and a square root) -- under 16 x 2^-24 = 9.5e-7 together.
The whole metric is held to the golden bar (1e-3) for its value and to the project's per-tensor gradient
bar (conftest.py: 2e-3 of the exact norm, or 4 x the fp32 reference's own error) for the gradient's norm
and worst element against float64.
"""
import numpy as np
import pytest
import torch

import lpips_grad_ref as G
import lpips_ref as L
from conftest import TERM_REF_X, TERM_REL
from test_gpu_lpips import ALL_SHAPES, FLOOR, GOLDEN_REL, _bar, _close, _model

pytestmark = pytest.mark.gpu

_REF = {}


def _gl(N):
    g = torch.Generator().manual_seed(77)
    v = torch.randn(N, generator=g)
    v[0] = -abs(v[0])
    if N > 1:
        v[1] = abs(v[1])
    return v


def _refs(shape):
    """Host inputs, device copies and both CPU gradients (weighted and not), computed once per shape."""
    if shape not in _REF:
        f0, f1, w = L.head_inputs(shape)
        gl = _gl(shape[0])
        _REF[shape] = dict(host=(f0, f1, w, gl), dev=tuple(t.cuda() for t in (f0, f1, w, gl)),
                           g64={k: G.head_grad64(f0, f1, w if k else None, gl) for k in (True, False)},
                           g32={k: G.head_grad32(f0, f1, w if k else None, gl) for k in (True, False)})
    return _REF[shape]


def _head_bwd(f0, f1, w, gl, N, C, P, bs0=None, bs1=None, d0=None, bsd0=None, want_d1=False):
    """vst_lpips_head_bwd on device tensors (f0, f1, d0 may be views into larger batches) -> (d0, d1)."""
    from vst._lib import lib, ptr, stream

    dev = f0.device
    d0 = torch.full((N, C, P), float("nan"), device=dev) if d0 is None else d0
    d1 = torch.full((N, C, P), float("nan"), device=dev) if want_d1 else None
    lib.vst_lpips_head_bwd(f0.data_ptr(), bs0 or C * P, f1.data_ptr(), bs1 or C * P, ptr(w), ptr(gl), N, C, P,
                           d0.data_ptr(), bsd0 or C * P, ptr(d1), C * P if want_d1 else 0, stream())
    return d0, d1


def _classes(P):
    """{name: pixel indices} as `lpips_ref.head_inputs` places its adversarial pixels."""
    special = {"f0 zero": 0 if P > 1 else None, "both zero": 1 if P > 2 else None, "1e4": 2 if P > 3 else None,
               "eps norm": 3 if P > 4 else None}
    out = {k: [v] for k, v in special.items() if v is not None}
    out["ordinary"] = [p for p in range(P) if p not in [v[0] for v in out.values()]]
    return out


@pytest.mark.parametrize("want_d1", [False, True])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_head_backward_vs_float64(shape, weighted, want_d1):
    N, C, h, w_ = shape
    P = h * w_
    r = _refs(shape)
    f0, f1, w, gl = r["dev"]
    d0, d1 = _head_bwd(f0, f1, w if weighted else None, gl, N, C, P, want_d1=want_d1)
    assert torch.isfinite(d0).all() and (d1 is None or torch.isfinite(d1).all())
    for side, got in (("dA", d0), ("dB", d1)):
        if got is None:
            continue
        k = 0 if side == "dA" else 1
        got = got.cpu().numpy().reshape(N, C, P)
        e64 = r["g64"][weighted][k].numpy().reshape(N, C, P)
        e32 = r["g32"][weighted][k].numpy().reshape(N, C, P)
        for name, px in _classes(P).items():
            tag = f"head bwd {shape} {'w' if weighted else 'ones'} {side} [{name}]"
            a, ref32, exact = got[:, :, px], e32[:, :, px], e64[:, :, px]
            if np.isfinite(ref32).all():
                _bar(a, ref32, exact, tag)
            else:  # torch: NaN at a zero norm; the closed form's limit, at the floor
                err, scale = float(np.abs(a - exact).max()), float(np.abs(exact).max())
                print(f"{tag}: |hip - f64| {err:.3e} of scale {scale:.3e} (torch: NaN)")
                assert err <= FLOOR * scale, (tag, err, scale)
            if name == "both zero":
                assert float(np.abs(a).max()) == 0.0


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_head_backward_layout_and_reproducibility(shape):
    N, C, h, w_ = shape
    P = h * w_
    f0, f1, w, gl = _refs(shape)["dev"]
    d0, d1 = _head_bwd(f0, f1, w, gl, N, C, P, want_d1=True)
    again0, again1 = _head_bwd(f0, f1, w, gl, N, C, P, want_d1=True)
    assert torch.equal(again0, d0) and torch.equal(again1, d1)
    assert torch.equal(_head_bwd(f0, f1, w, gl, N, C, P)[0], d0)  # d1 = NULL changes nothing in d0
    # image n of the batch alone
    for n in range(N):
        one0, one1 = _head_bwd(f0[n:n + 1].contiguous(), f1[n:n + 1].contiguous(), w, gl[n:n + 1].contiguous(), 1, C, P,
                               want_d1=True)
        assert torch.equal(one0[0], d0[n]) and torch.equal(one1[0], d1[n])
    # f0, f1 and d0 as views into batches whose images lie 3 C P apart; the padding stays untouched
    wide = torch.full((N, 3, C, P), float("nan"), device=f0.device)
    wide[:, 0], wide[:, 2] = f0.view(N, C, P), f1.view(N, C, P)
    out = torch.full((N, 2, C, P), float("nan"), device=f0.device)
    _head_bwd(wide[:, 0], wide[:, 2], w, gl, N, C, P, bs0=3 * C * P, bs1=3 * C * P, d0=out[:, 1], bsd0=2 * C * P)
    assert torch.equal(out[:, 1], d0) and bool(torch.isnan(out[:, 0]).all())
    assert bool(torch.isnan(wide[:, 1]).all())
    # gl[n] = 0: exact zeros for image n
    gz = gl.clone()
    gz[N - 1] = 0.0
    z0, z1 = _head_bwd(f0, f1, w, gz, N, C, P, want_d1=True)
    assert float(z0[N - 1].abs().max()) == 0.0 and float(z1[N - 1].abs().max()) == 0.0
    if N > 1:
        assert torch.equal(z0[0], d0[0])


# ------------------------------------------------------------------------------------------------
# the whole metric
_METRIC = {}


def _metric_refs(g, key):
    """Both CPU gradients of sum_n total[n] with respect to in0, once per pair."""
    if key not in _METRIC:
        params = L.trunk_params(int(g["trunk_seed"]))
        lins = [torch.from_numpy(g[f"lin{k}"]) for k in range(5)]
        t0, t1 = L.im2tensor(g[key + "_img0"]), L.im2tensor(g[key + "_img1"])
        _METRIC[key] = dict(params=params, lins=lins, t0=t0, t1=t1, r64=G.metric_grad(params, lins, t0, t1, torch.float64),
                            r32=G.metric_grad(params, lins, t0, t1, torch.float32))
    return _METRIC[key]


def _grad_bar(got, r32, r64, what):
    """The per-tensor gradient bar of conftest.py (term_grad_margins), on the norm and the worst element."""
    got, r32, r64 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, r32, r64))
    assert np.isfinite(got).all(), what
    e, r, n = (float(np.linalg.norm(v)) for v in (r64, r32, got))
    bar_n = max(TERM_REL * e, TERM_REF_X * abs(r - e))
    bar_s = max(TERM_REL * e, TERM_REF_X * float(np.abs(r32 - r64).max()))
    worst = float(np.abs(got - r64).max())
    print(f"{what}: norm {n:.6e} vs exact {e:.6e} ({abs(n - e) / e:.2e} rel, bar {bar_n / e:.2e}); worst element "
          f"{worst:.3e} ({worst / e:.2e} of the norm, bar {bar_s / e:.2e}); ||hip - f64|| / ||f64|| "
          f"{float(np.linalg.norm(got - r64)) / e:.2e}")
    assert abs(n - e) <= bar_n and worst <= bar_s, (what, n, e, worst, bar_n, bar_s)


def _distance_and_grad(model, target, x, **kw):
    x = x.clone().requires_grad_(True)
    val = model.distance_to(target, x, **kw)
    val.sum().backward()
    return val.detach(), x.grad


@pytest.mark.parametrize("key", ["p16", "p32"])
def test_distance_to_value_and_gradient(golden, step_policy, key):
    from vst.lpips import PerceptualLoss

    g = golden("lpips_vgg")
    model = _model(g)
    m = _metric_refs(g, key)
    N = m["t0"].shape[0]
    t0, t1 = m["t0"].cuda(), m["t1"].cuda().requires_grad_(True)
    target = model.encode(t1)
    val, grad = _distance_and_grad(model, target, t0)
    assert val.shape == (N, 1, 1, 1) and grad.shape == t0.shape
    _close(val.reshape(-1).cpu().numpy(), g[key + "_total"], f"{key} {step_policy} distance_to")
    _grad_bar(grad.cpu().numpy(), m["r32"][1].numpy(), m["r64"][1].numpy(), f"{key} {step_policy} d/d in0")
    assert t1.grad is None and all(not f.requires_grad for f in target.feats)  # the target carries no gradient
    # nothing recorded: the same value bit for bit, per-layer values detached
    plain, layers = model.distance_to(target, t0, retPerLayer=True)
    assert not plain.requires_grad and torch.equal(plain, val)
    with torch.no_grad():
        assert torch.equal(model.distance_to(target, t0.clone().requires_grad_(True)), val)
    rec, rec_layers = model.distance_to(target, t0.clone().requires_grad_(True), retPerLayer=True)
    assert rec.requires_grad and all(not v.requires_grad and v.shape == (N, 1, 1, 1) for v in rec_layers)
    for k in range(5):
        assert torch.equal(rec_layers[k], layers[k])
        _close(layers[k].reshape(-1).cpu().numpy(), g[key + "_layers"][k], f"{key} {step_policy} level {k}")
    # the uint8 twin of encode builds the same target
    tu8 = model.encode_u8(torch.from_numpy(g[key + "_img1"]).cuda(), bgr=False)
    assert all(torch.equal(a, b) for a, b in zip(tu8.feats, target.feats))
    # normalize=True on [0,1] planes: d/dx of the same metric of 2 x - 1, i.e. twice the gradient; the
    # trunk input differs from im2tensor's by fp32 rounding, so the gradient bar applies to half of it
    u0, u1 = L.unit01(g[key + "_img0"]).cuda(), L.unit01(g[key + "_img1"]).cuda()
    nval, ngrad = _distance_and_grad(model, model.encode(u1, normalize=True), u0, normalize=True)
    _close(nval.reshape(-1).cpu().numpy(), g[key + "_norm01"], f"{key} {step_policy} normalize=True")
    _grad_bar(0.5 * ngrad.cpu().numpy(), m["r32"][1].numpy(), m["r64"][1].numpy(), f"{key} {step_policy} normalize=True")
    # PerceptualLoss on [0,255] planes: x / 255 is unit01's own division, so the trunk input is the
    # normalize=True form's bit for bit and the gradient is ngrad * weight / (255 N) up to the rounding
    # of that constant (2 / 255 in fp32, one product: 2^-23 relative); weight / N is a power of two, so
    # the upstream gradient scales every intermediate exactly
    f0, f1 = (torch.from_numpy(g[f"{key}_img{i}"].transpose(0, 3, 1, 2).copy()).float().cuda() for i in (0, 1))
    weight = 2.0 * N
    loss_mod = PerceptualLoss(model, weight=weight).set_target(f1)
    x = f0.clone().requires_grad_(True)
    loss = loss_mod(x)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    want = weight * float(nval.double().mean())
    assert abs(float(loss.detach()) - want) <= 1e-6 * want
    scaled = ngrad.double() * (weight / (255.0 * N))
    assert float((x.grad.double() - scaled).abs().max()) <= 2.0 ** -22 * float(scaled.abs().max())
    from vst import ops

    both = ops.sum_scalars(loss_mod(f0), loss_mod(f0))
    assert both.dim() == 0 and abs(float(both) - 2 * float(loss.detach())) <= 1e-6 * float(both)


def test_one_gradient_step_lowers_the_distance(golden, step_policy):
    g = golden("lpips_vgg")
    m = _metric_refs(g, "p32")
    total64, g64 = m["r64"]
    # a quarter of the step that would take the linearised distance to zero, from the float64 reference
    lr = 0.25 * float(total64.sum()) / float(g64.pow(2).sum())
    stepped, _ = G.metric_grad(m["params"], m["lins"], (m["t0"].double() - lr * g64).float(), m["t1"], torch.float64)
    assert float(stepped.sum()) < float(total64.sum())  # the reference's own step lowers it
    model = _model(g)
    t0 = m["t0"].cuda()
    target = model.encode(m["t1"].cuda())
    val, grad = _distance_and_grad(model, target, t0)
    after = model.distance_to(target, (t0 - lr * grad).contiguous())
    print(f"p32 {step_policy}: distance {float(val.sum()):.6f} -> {float(after.sum()):.6f} (float64 reference "
          f"{float(total64.sum()):.6f} -> {float(stepped.sum()):.6f}), lr {lr:.3e}")
    assert float(after.sum()) < float(val.sum())


def test_refusals(golden):
    from vst._lib import VstError, lib

    g = golden("lpips_vgg")
    model = _model(g)
    x = torch.zeros(1, 3, 16, 16, device="cuda")
    target = model.encode(x)
    with pytest.raises(VstError, match="spatial"):
        sp = _model(g, spatial=True)
        sp.distance_to(sp.encode(x), x)
    with pytest.raises(VstError):
        model.distance_to(target, torch.zeros(1, 3, 16, 16))  # a host tensor
    with pytest.raises(VstError):
        model.encode(torch.zeros(1, 3, 16, 16))
    with pytest.raises(VstError):
        model.distance_to(target, torch.zeros(1, 3, 16, 32, device="cuda"))  # not the target's shape
    with pytest.raises(VstError):
        model.encode(torch.zeros(1, 3, 8, 16, device="cuda"))
    f = torch.zeros(1, 24, 4, device="cuda")
    gl = torch.ones(1, device="cuda")
    rc = lib.load().vst_lpips_head_bwd(f.data_ptr(), 96, f.data_ptr(), 96, None, gl.data_ptr(), 1, 24, 4,
                                       torch.empty_like(f).data_ptr(), 96, None, 0, None)
    assert rc == -1  # VST_EINVAL: C is not a multiple of 16
    xg = torch.zeros(1, 3, 16, 16, device="cuda", requires_grad=True)
    with pytest.raises(VstError, match="grad"):
        model(xg, x)
