"""LPIPS on the GPU (vst.lpips, csrc/lpips.hip) against the float64 restatement of tests/lpips_ref.py and
the reference's own outputs in tests/golden/lpips_vgg.npz.

Bars.  The fused head may sit at most 4x as far from float64 as the reference's own fp32 op sequence
(torch-CPU) sits on the same inputs, with a floor of 1e-6 relative -- the bar of tests/test_gpu_metrics.py.
The input kernel is bit-exact.  The model is held to the project's model-versus-golden bar, 1e-3
relative, under the f32 and bf16x6 policies.  The measured distances are printed and recorded in
DESIGN.md 4.12.
"""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import lpips_ref as L
import metrics_ref as M
from conftest import PKG

pytestmark = pytest.mark.gpu

FLOOR, REF_X = 1e-6, 4.0
GOLDEN_REL = 1e-3


def _bar(hip, ref32, exact, what):
    """Distances from float64 (worst element), the bar, and the assertion."""
    hip, ref32, exact = (np.asarray(v, dtype=np.float64) for v in (hip, ref32, exact))
    assert np.isfinite(hip).all(), what
    d_hip, d_ref = float(np.abs(hip - exact).max()), float(np.abs(ref32 - exact).max())
    scale = float(np.abs(exact).max())
    bar = max(REF_X * d_ref, FLOOR * scale)
    print(f"{what}: |hip - f64| {d_hip:.3e} ({d_hip / max(scale, 1e-300):.2e} rel), |ref fp32 - f64| {d_ref:.3e} "
          f"({d_ref / max(scale, 1e-300):.2e} rel), bar {bar:.3e}")
    assert d_hip <= bar, (what, d_hip, d_ref, bar)


# ------------------------------------------------------------------------------------------------
# the head
# the issue's shapes (all on the 32-pixel blocks: 32 groups, C % 32 == 0), then: 16 groups of the
# 32-pixel form (C % 32 != 0), both sides of the 4096-pixel threshold, and the 64-pixel form with 4, 8 and
# 16 groups and a ragged last block
EXTRA_SHAPES = [(2, 80, 3, 5), (1, 16, 2, 2), (1, 64, 64, 64), (2, 64, 1, 4097), (1, 48, 65, 64), (1, 256, 1, 4100),
                (1, 512, 1, 4099)]
ALL_SHAPES = L.HEAD_SHAPES + EXTRA_SHAPES
_HEAD = {}


def _inputs(shape):
    """(f0, f1, w) on the host, their device copies and the two CPU references, computed once."""
    if shape not in _HEAD:
        f0, f1, w = L.head_inputs(shape)
        _HEAD[shape] = dict(host=(f0, f1, w), dev=tuple(t.cuda() for t in (f0, f1, w)),
                            r64={True: L.head64(f0, f1, w), False: L.head64(f0, f1, None)},
                            r32={True: L.head32(f0, f1, w), False: L.head32(f0, f1, None)})
    return _HEAD[shape]


def _head(f0, f1, w, N, C, P, bs0=None, bs1=None, total=None, accumulate=0, want_map=True):
    """vst_lpips_head on device tensors (f0, f1 may be views into a larger batch) -> (layer, total, map)."""
    from vst._lib import lib, ptr, stream

    dev = f0.device
    layer = torch.full((N,), float("nan"), device=dev)
    total = torch.full((N,), float("nan"), device=dev) if total is None else total
    dmap = torch.full((N, P), float("nan"), device=dev) if want_map else None
    nbytes = lib.vst_lpips_head_workspace(N, C, P)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    lib.vst_lpips_head(f0.data_ptr(), bs0 or C * P, f1.data_ptr(), bs1 or C * P, ptr(w), N, C, P, ptr(layer), ptr(total),
                       accumulate, ptr(dmap), ws.data_ptr(), stream())
    return layer, total, dmap


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_head_vs_float64(shape, weighted):
    N, C, h, w_ = shape
    P = h * w_
    d = _inputs(shape)
    f0, f1, w = d["dev"]
    layer, total, dmap = _head(f0, f1, w if weighted else None, N, C, P)
    l64, m64 = d["r64"][weighted]
    l32, m32 = d["r32"][weighted]
    tag = f"head {shape} {'w' if weighted else 'ones'}"
    _bar(layer.cpu().numpy(), l32.numpy(), l64.numpy(), tag + " layer")
    _bar(dmap.cpu().numpy().reshape(N, h, w_), m32.numpy(), m64.numpy(), tag + " map")
    assert torch.equal(total, layer)  # accumulate = 0 sets
    if P > 2:
        assert float(dmap[:, 1].abs().max()) == 0.0  # all-zero in both features: exactly 0, no NaN
        assert float(dmap[:, 0].min()) > 0.0  # all-zero in f0 only: the whole of normalised f1


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_head_sums_identity_reproducibility_batching_strides(shape):
    N, C, h, w_ = shape
    P = h * w_
    f0, f1, w = _inputs(shape)["dev"]
    layer, total, dmap = _head(f0, f1, w, N, C, P)
    # the accumulate flag: total += layer, so a chain of calls sums the `layer` outputs in call order
    layer2, total2, _ = _head(f0, f1, None, N, C, P, total=total.clone(), accumulate=1, want_map=False)
    assert torch.equal(total2, layer + layer2)
    layer3, total3, _ = _head(f1, f0, w, N, C, P, total=total2.clone(), accumulate=1, want_map=False)
    assert torch.equal(total3, (layer + layer2) + layer3)
    # f1 = f0: exactly 0.0
    same_l, _, same_m = _head(f0, f0.clone(), w, N, C, P)
    assert float(same_l.abs().max()) == 0.0 and float(same_m.abs().max()) == 0.0
    # run to run, and without the map
    again_l, _, again_m = _head(f0, f1, w, N, C, P)
    assert torch.equal(again_l, layer) and torch.equal(again_m, dmap)
    assert torch.equal(_head(f0, f1, w, N, C, P, want_map=False)[0], layer)
    # image n of the batch alone
    for n in range(N):
        one_l, _, one_m = _head(f0[n:n + 1].contiguous(), f1[n:n + 1].contiguous(), w, 1, C, P)
        assert torch.equal(one_l, layer[n:n + 1]) and torch.equal(one_m, dmap[n:n + 1])
    # the two halves of one 2N batch, and images 3 C P apart
    both = torch.cat([f0, f1]).contiguous()
    half_l, _, half_m = _head(both[:N], both[N:], w, N, C, P)
    assert torch.equal(half_l, layer) and torch.equal(half_m, dmap)
    wide = torch.full((N, 3, C, P), float("nan"), device=f0.device)
    wide[:, 0], wide[:, 2] = f0.view(N, C, P), f1.view(N, C, P)
    wide_l, _, wide_m = _head(wide[:, 0], wide[:, 2], w, N, C, P, bs0=3 * C * P, bs1=3 * C * P)
    assert torch.equal(wide_l, layer) and torch.equal(wide_m, dmap)


def test_package_functions_against_torch_cpu():
    from vst import lpips as VL

    g = torch.Generator().manual_seed(7)
    x = torch.relu(torch.randn(2, 64, 5, 7, generator=g))
    x.view(2, 64, 35)[:, :, 3] = 0.0
    xd = x.cuda()
    want = L._normalize32(x)
    got = VL.normalize_tensor(xd).cpu()
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert torch.allclose(VL.spatial_average(xd).cpu(), x.mean([2, 3], keepdim=True), rtol=1e-6, atol=1e-7)
    assert VL.spatial_average(xd[:, :, :1, :1].contiguous(), keepdim=False).shape == (2, 64)
    up = VL.upsample(xd[:, :1].contiguous(), (10, 21)).cpu()
    ref = torch.nn.functional.interpolate(x[:, :1], size=(10, 21), mode="bilinear", align_corners=False)
    assert torch.allclose(up, ref, rtol=1e-5, atol=1e-6)
    lin = VL.NetLinLayer(64, use_dropout=True).eval()
    with torch.no_grad():
        lin.weight.copy_(torch.rand(1, 64, 1, 1, generator=g))
        ref = lin.model(x)
    out = lin.cuda()(xd).cpu()
    assert out.shape == ref.shape and float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert torch.equal(VL.ScalingLayer().cuda()(xd[:, :3].contiguous()).cpu(), L.scaling(x[:, :3]))


# ------------------------------------------------------------------------------------------------
# the input kernel
def _lp_input(src, out, offset, N, H, W, u8, swap_rb=False, normalize=False, scaling=True):
    from vst.lpips import _input

    _input(src, out, offset, N, H, W, u8, swap_rb, normalize, scaling)
    return out


@pytest.mark.parametrize("swap_rb", [False, True])
def test_input_u8_table_bit_exact(golden, swap_rb):
    table = golden("lpips_vgg")["input_table"]  # (256,3): im2tensor then ScalingLayer, per value and channel
    # every value 0..255 in every channel of each frame, and the channels differ at every pixel (so a
    # wrong channel order shows): channel c holds (v + 85 c) mod 256, the second frame runs backwards
    v = np.arange(256).reshape(16, 16, 1) + 85 * np.arange(3).reshape(1, 1, 3)
    frames = np.stack([v % 256, (255 - v) % 256]).astype(np.uint8)
    for c in range(3):
        assert all(np.array_equal(np.sort(f[..., c].reshape(-1)), np.arange(256)) for f in frames)
    out = _lp_input(torch.from_numpy(frames).cuda(), torch.empty(2, 3, 16, 16, device="cuda"), 0, 2, 16, 16, True, swap_rb)
    src = frames[..., ::-1] if swap_rb else frames
    want = np.stack([table[src[..., c], c] for c in range(3)], axis=1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    raw = _lp_input(torch.from_numpy(frames).cuda(), torch.empty(2, 3, 16, 16, device="cuda"), 0, 2, 16, 16, True, swap_rb,
                    scaling=False)
    assert torch.equal(raw.cpu(), L.im2tensor(np.ascontiguousarray(src)))


@pytest.mark.parametrize("normalize", [False, True])
def test_input_fp32_bit_exact_and_batch_offset(normalize):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 5, 7, generator=g) if normalize else torch.rand(2, 3, 5, 7, generator=g) * 2 - 1
    buf = torch.full((4, 3, 5, 7), -7.0, device="cuda")
    _lp_input(x.cuda(), buf, 2, 2, 5, 7, False, normalize=normalize)
    want = L.scaling(2 * x - 1 if normalize else x)
    assert torch.equal(buf[2:].cpu(), want)
    assert float((buf[:2] + 7.0).abs().max()) == 0.0  # the other half untouched
    _lp_input(x.cuda(), buf, 0, 2, 5, 7, False, normalize=normalize, scaling=False)
    assert torch.equal(buf[:2].cpu(), 2 * x - 1 if normalize else x) and torch.equal(buf[2:].cpu(), want)


# ------------------------------------------------------------------------------------------------
# the model against the reference's outputs
def _model(g, **kw):
    from vst.lpips import LPIPS

    model = LPIPS(net="vgg", pretrained=False, verbose=False, **kw)
    model.net.load_state_dict(L.trunk_params(int(g["trunk_seed"])))
    if kw.get("lpips", True):
        model.load_state_dict({f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1)
                               for k in range(5)}, strict=False)
    return model.cuda()


def _close(got, want, what, rel=GOLDEN_REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{what}: {err:.2e} rel")
    assert got.shape == want.shape and err <= rel, (what, got, want)


@pytest.mark.parametrize("key", list(L.PAIRS))
def test_model_matches_the_reference(golden, step_policy, key):
    g = golden("lpips_vgg")
    model = _model(g)
    img0, img1 = g[key + "_img0"], g[key + "_img1"]
    N = img0.shape[0]
    t0, t1 = L.im2tensor(img0).cuda(), L.im2tensor(img1).cuda()
    val, res = model(t0, t1, retPerLayer=True)
    assert val.shape == (N, 1, 1, 1) and len(res) == 5 and all(r.shape == (N, 1, 1, 1) for r in res)
    _close(val.reshape(-1).cpu().numpy(), g[key + "_total"], f"{key} {step_policy} total")
    for k in range(5):
        _close(res[k].reshape(-1).cpu().numpy(), g[key + "_layers"][k], f"{key} {step_policy} level {k}")
    assert torch.equal(model(t0, t1), val)
    # the batch against its images run singly (the trunk's GEMMs may split differently: fp32 order)
    for n in range(N):
        one = model(t0[n:n + 1].contiguous(), t1[n:n + 1].contiguous())
        _close(one.reshape(-1).cpu().numpy(), val[n].reshape(-1).cpu().numpy(), f"{key} image {n} alone", rel=1e-5)
    assert float(model(t0, t0.clone()).abs().max()) == 0.0  # identical images
    norm = model(L.unit01(img0).cuda(), L.unit01(img1).cuda(), normalize=True)
    _close(norm.reshape(-1).cpu().numpy(), g[key + "_norm01"], f"{key} normalize=True")
    _close(_model(g, lpips=False)(t0, t1).reshape(-1).cpu().numpy(), g[key + "_baseline"], f"{key} lpips=False")
    _close(_model(g, version="0.0")(t0, t1).reshape(-1).cpu().numpy(), g[key + "_v00"], f"{key} version 0.0")
    u8 = model.forward_u8(torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda(), bgr=False)
    assert torch.equal(u8, val)  # the uint8 entry builds the same trunk input bit for bit


def test_spatial_map(golden, step_policy):
    g = golden("lpips_vgg")
    model = _model(g, spatial=True)
    t0, t1 = L.im2tensor(g["p32_img0"]).cuda(), L.im2tensor(g["p32_img1"]).cuda()
    val, res = model(t0, t1, retPerLayer=True)
    want = g["p32_spatial"]
    assert val.shape == (2, 1, 32, 48) and len(res) == 5
    err = float(np.abs(val.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"spatial map {step_policy}: {err:.2e} of the map's maximum")
    assert err <= GOLDEN_REL
    assert float((sum(r.cpu() for r in res) - val.cpu()).abs().max()) <= 1e-6 * float(np.abs(want).max())


def _shim(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_metrics_and_drop_ins(golden, step_policy, tmp_path):
    import vst.lpips
    from vst._lib import VstError
    from vst.metrics import LPIPSMean, lpips_distance

    g = golden("lpips_vgg")
    model = _model(g)
    mean = LPIPSMean(model, bgr=True)
    singles, wants = [], []
    for key in L.PAIRS:
        # cv2-order frames: the fixture's RGB reversed
        f0, f1 = (torch.from_numpy(np.ascontiguousarray(g[f"{key}_img{i}"][..., ::-1])).cuda() for i in (0, 1))
        d = lpips_distance(model, f0, f1, bgr=True)
        assert d.shape == (f0.shape[0],)
        _close(d.cpu().numpy(), g[key + "_total"], f"lpips_distance {key} {step_policy}")
        assert mean.update(f0, f1) is mean
        singles += d.cpu().tolist()
        wants += g[key + "_total"].tolist()
    acc, pairs = mean.state()
    assert pairs == 4 and acc.shape == (1,)
    with pytest.raises(VstError, match="spatial"):
        LPIPSMean(_model(g, spatial=True)).update(f0, f1)
    got = mean.result()
    assert abs(got - float(np.mean(singles))) <= 1e-6 * float(np.mean(singles))
    assert abs(got - float(np.mean(wants))) <= GOLDEN_REL * float(np.mean(wants))

    # AA/eval.py lpips_loss through the adaattn/ shims, over PNG files of the fixture's pixels
    ev = _shim("adaattn/eval.py", "adaattn_eval_shim_lpips")
    pkg = _shim("adaattn/lpips/__init__.py", "adaattn_lpips_shim")
    assert pkg.LPIPS is vst.lpips.LPIPS and pkg.im2tensor is vst.lpips.im2tensor
    paths = [str(tmp_path / f"p36_{i}.png") for i in (0, 1)]
    for i, p in enumerate(paths):
        M.write_png(p, g[f"p36_img{i}"][0][..., ::-1])
    assert np.array_equal(pkg.load_image(paths[0]), g["p36_img0"][0])
    assert torch.equal(pkg.im2tensor(pkg.load_image(paths[0])), L.im2tensor(g["p36_img0"]))
    ev.lpips_loss.loss_fn = model
    opt = argparse.Namespace(path0=paths[0], path1=paths[1], device="cuda")
    loss = ev.lpips_loss(opt, no_print=True)
    ref = float(g["p36_lpips_loss"])
    print(f"lpips_loss {step_policy}: {loss:.8f} vs the reference's {ref:.8f} ({abs(loss - ref) / ref:.2e} rel)")
    assert isinstance(loss, float) and abs(loss - ref) <= GOLDEN_REL * ref


def test_forward_refuses_host_tensors_and_gradients(golden):
    from vst._lib import VstError

    model = _model(golden("lpips_vgg"))
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(VstError):
        model(x, x)
    with pytest.raises(VstError):
        model.forward_u8(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    xg = torch.zeros(1, 3, 16, 16, device="cuda", requires_grad=True)
    with pytest.raises(VstError, match="grad"):
        model(xg, x.cuda())
    with pytest.raises(VstError):
        model(torch.zeros(1, 3, 8, 16, device="cuda"), torch.zeros(1, 3, 8, 16, device="cuda"))
