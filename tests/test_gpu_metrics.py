"""The evaluation metrics on the GPU (vst.metrics, csrc/metrics.hip) against the float64 restatement
of tests/metrics_ref.py and the reference's own outputs in tests/golden/eval_metrics.npz.

Bars.  A fused value may sit at most 4x as far from float64 as the reference's own fp32 form (torch-CPU
`grid_sample` + `mean`, five `conv2d`) sits on the same inputs -- the factor allows for a different but
fixed summation order -- with a floor of 1e-6 relative (a few fp32 roundings of the result itself).
The measured distances are printed and recorded in DESIGN.md 4.11.  Model-level drop-ins are held to
the project's model-versus-golden bar, 1e-3 relative (SSIM, no model in it: 1e-5).
"""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import metrics_ref as M
import oracle
from conftest import PKG
from oracle import shapes

pytestmark = pytest.mark.gpu

FLOOR, REF_X = 1e-6, 4.0


def _bar(hip, ref32, exact, what):
    """Distances from float64 (worst element), the bar, and the assertion."""
    hip, ref32, exact = (np.asarray(v, dtype=np.float64) for v in (hip, ref32, exact))
    d_hip, d_ref = float(np.abs(hip - exact).max()), float(np.abs(ref32 - exact).max())
    scale = float(np.abs(exact).max())
    bar = max(REF_X * d_ref, FLOOR * scale)
    print(f"{what}: |hip - f64| {d_hip:.3e} ({d_hip / max(scale, 1e-300):.2e} rel), |ref fp32 - f64| {d_ref:.3e} "
          f"({d_ref / max(scale, 1e-300):.2e} rel), bar {bar:.3e}")
    assert d_hip <= bar, (what, d_hip, d_ref, bar)


# ------------------------------------------------------------------------------------------------
# temporal error
TE_SHAPES = [(2, 3, 7, 9), (1, 3, 16, 64)]  # odd sizes: the per-pixel path; W % 4 == 0: four pixels per thread
_TE = {}


def _te_inputs(shape):
    """a, b in [-20, 280] (clamp_unit bites), a flow with: zero flow (row 0; its column 0 samples
    source x = -0.5 exactly, the zero-padding edge, since the grid is normalised by W - 1), a
    whole-pixel flow (row 1), targets far outside the frame (row 2), a few pixels elsewhere; a 0/1 mask."""
    if shape not in _TE:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(17 + H)
        a = torch.rand(shape, generator=g) * 300 - 20
        b = torch.rand(shape, generator=g) * 300 - 20
        flo = torch.randn(B, 2, H, W, generator=g) * 2.5
        flo[:, :, 0] = 0.0
        flo[:, 0, 1], flo[:, 1, 1] = 2.0, -1.0
        flo[:, 0, 2], flo[:, 1, 2] = 1e4, -3e3
        flo[:, 0, 3, : W // 2] = -float(W)  # just outside, along the left edge
        mask = (torch.rand(B, H, W, generator=g) > 0.3).float()
        _TE[shape] = (a, b, flo, mask)
    return _TE[shape]


def _te_state(a, b, flo, mask, power, clamp, hwc, updates=1):
    from vst.metrics import TemporalError

    te = TemporalError(power, clamp_unit=clamp)
    f = flo.permute(0, 2, 3, 1).contiguous() if hwc else flo
    dev = [t.cuda() if t is not None else None for t in (a, b, f, mask)]
    for _ in range(updates):
        te.update(dev[0], dev[1], dev[2], dev[3], flow_hwc=hwc)
    return te


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("shape", TE_SHAPES)
def test_temporal_error_vs_float64(shape, power, hwc, masked, clamp):
    a, b, flo, mask = _te_inputs(shape)
    mask = mask if masked else None
    total, pairs = _te_state(a, b, flo, mask, power, clamp, hwc).state().tolist()
    exact = M.temporal_pair_sum(a, b, flo, mask, power, clamp, torch.float64)
    ref32 = M.temporal_pair_sum(a, b, flo, mask, power, clamp, torch.float32, mean=True)
    assert pairs == shape[0] and exact > 0
    _bar(total, ref32, exact, f"temporal {shape} p{power} hwc{int(hwc)} mask{int(masked)} clamp{int(clamp)}")


@pytest.mark.parametrize("shape", TE_SHAPES)
def test_temporal_error_accumulates_and_reproduces(shape):
    from vst import ops

    a, b, flo, mask = _te_inputs(shape)
    B, C, H, W = shape
    single = _te_state(a, b, flo, mask, 2, False, False).state().tolist()
    again = _te_state(a, b, flo, mask, 2, False, False).state().tolist()
    assert single == again  # bitwise run to run
    three = _te_state(a, b, flo, mask, 2, False, False, updates=3)
    assert three.state().tolist() == [single[0] + single[0] + single[0], 3.0 * B]
    assert three.result() == float(np.sqrt(three.state()[0].item() / (3 * B)))
    aa = _te_state(a, b, flo, mask, 1, True, True, updates=2)
    s, n = aa.state().tolist()
    aa.convention = "aa"
    assert aa.result() == float(np.sqrt(s)) / n
    # an all-zero mask: exactly 0, and the pair count still advances
    zero = _te_state(a, b, flo, torch.zeros_like(mask), 2, False, False)
    assert zero.state().tolist() == [0.0, float(B)]
    # the fused pass against the composition it replaces, on the same device tensors
    ad, bd, fd, md = (t.cuda() for t in (a, b, flo, mask))
    comp = (md.unsqueeze(1) * (ad - ops.warp(bd, fd)) ** 2).double().sum().item() / (C * H * W)
    assert abs(single[0] - comp) <= 1e-6 * comp, (single[0], comp)


# ------------------------------------------------------------------------------------------------
# SSIM
@pytest.mark.parametrize("tile", ["32x32", "64x16"])
@pytest.mark.parametrize("key,shape,kind,seed", M.ssim_cases())
def test_ssim_vs_float64(golden, key, shape, kind, seed, tile):
    from vst.metrics import SSIMMetric

    x, y = M.ssim_inputs(shape, kind, seed)
    metric = SSIMMetric(11, shape[1], 1.5, reduction="none").cuda()
    score, smap = metric(x.cuda(), y.cuda(), return_map=True, tile=tile)
    assert score.shape == (shape[0],) and smap.shape == shape
    m64, m32 = M.ssim_map(x, y, dtype=torch.float64), M.ssim_map(x, y, dtype=torch.float32)
    per = lambda m: m.mean(dim=[2, 3]).mean(dim=1).numpy()  # noqa: E731
    _bar(score.cpu().numpy(), per(m32), per(m64), f"{key} {tile} score")
    _bar(smap.cpu().numpy(), m32.numpy(), m64.numpy(), f"{key} {tile} map")
    g = golden("eval_metrics")
    assert np.abs(score.cpu().numpy() - g[key + "_none"]).max() <= 1e-5 * np.abs(g[key + "_none"]).max()
    mean = SSIMMetric(11, shape[1], 1.5, reduction="mean").cuda()(x.cuda(), y.cuda(), tile=tile)
    assert mean.dim() == 0 and abs(mean.item() - float(g[key + "_mean"])) <= 1e-5 * float(g[key + "_mean"])


@pytest.mark.parametrize("win", [1, 3, 7, 11])
def test_ssim_identity_and_windows(win):
    from vst.metrics import ssim

    x, y = M.ssim_inputs((2, 3, 13, 37), "u255", 5)
    same = ssim(x.cuda(), x.cuda(), window_size=win, reduction="none")
    assert same.shape == (2,) and float((same - 1).abs().max()) <= 1e-6
    score = ssim(x.cuda(), y.cuda(), window_size=win, reduction="none").cpu().numpy()
    exact = M.ssim(x, y, window_size=win, dtype=torch.float64).numpy()
    _bar(score, M.ssim(x, y, window_size=win).numpy(), exact, f"window {win}")


# ------------------------------------------------------------------------------------------------
# histogram / KL
@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 64, 48, 3), (1, 32, 32, 3), (3, 9, 11, 1), (1, 16, 24, 1)])
def test_histogram_equals_bincount(shape):
    from vst.metrics import histogram_u8

    img = np.random.default_rng(shape[1]).integers(0, 256, size=shape, dtype=np.uint8)
    if shape == (1, 32, 32, 3):
        img[:] = 200  # every thread hits one bin
    hist = histogram_u8(torch.from_numpy(img).cuda())
    assert hist.dtype == torch.int32 and hist.shape == (shape[0], shape[3], 256)
    want = np.stack([M.histograms(i) for i in img])
    assert np.array_equal(hist.cpu().numpy(), want)
    assert np.array_equal(histogram_u8(torch.from_numpy(img).cuda()).cpu().numpy(), want)  # overwritten, not added


def test_kl_divergence_golden(golden):
    from vst.metrics import kl_divergence

    g = golden("eval_metrics")
    kl = kl_divergence(torch.from_numpy(g["kl_img0"]).cuda(), torch.from_numpy(g["kl_img1"]).cuda())
    assert abs(kl - float(g["kl_loss"])) <= 1e-9


# ------------------------------------------------------------------------------------------------
# drop-ins
def _shim(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_temporal_errors_sintel_drop_in(golden, step_policy, tmp_path):
    util = _shim("rtnstv/utilities.py", "rtnstv_utilities_shim")
    from vst.rtnstv.network import StylizingNetwork

    g = golden("eval_metrics")
    root = str(tmp_path / "MPI-Sintel-complete")
    ckpt = str(tmp_path / "rt.pth")
    torch.save(oracle.seeded_params(shapes.rtnstv(), int(g["te_seed"])), ckpt)
    for scene in M.SCENES:
        M.write_sintel_scene(root, scene, g[f"te_{scene}_frames"], g[f"te_{scene}_occ"], g[f"te_{scene}_flows"])
        err = util.temporal_errors_sintel(StylizingNetwork, ckpt, scene, device="cuda", root=root)
        ref = float(g[f"te_{scene}_error"])
        print(f"{scene} {step_policy}: {err:.8f} vs the reference's {ref:.8f} ({abs(err - ref) / ref:.2e} rel)")
        assert abs(err - ref) <= 1e-3 * ref
    flow = util.read_sintel_flow(os.path.join(root, "training", "flow", "scene_b", "frame_0001.flo"))
    assert np.array_equal(flow, g["te_scene_b_flows"][0])


def test_adaattn_eval_drop_in(golden, tmp_path):
    ev = _shim("adaattn/eval.py", "adaattn_eval_shim")
    from vst.adaattn.inference import load_vgg

    g = golden("eval_metrics")
    paths = {}
    for k in ("gram_img0", "gram_img1", "kl_img0", "kl_img1"):
        paths[k] = str(tmp_path / (k + ".png"))
        M.write_png(paths[k], g[k])
    opt = argparse.Namespace(path0=paths["gram_img0"], path1=paths["gram_img1"], device="cuda")
    s = ev.ssim_loss(opt, no_print=True)
    assert abs(s - float(g["gram_ssim"])) <= 1e-5 * float(g["gram_ssim"])
    assert isinstance(ev.ssim_loss.metric, ev.SSIMMetric)
    ev.gram_loss.vgg19 = load_vgg(oracle.seeded_params(shapes.vgg19(), int(g["vgg_seed"])))
    gl = ev.gram_loss(opt, no_print=True)
    print(f"gram_loss {gl:.8f} vs {float(g['gram_loss']):.8f}, ssim_loss {s:.8f} vs {float(g['gram_ssim']):.8f}")
    assert abs(gl - float(g["gram_loss"])) <= 1e-3 * float(g["gram_loss"])
    x = torch.randn(2, 5, 3, 4, device="cuda")
    gm = ev.gram_matrix(x).cpu()
    f = x.cpu().reshape(2, 5, 12)
    assert torch.allclose(gm, f.bmm(f.transpose(1, 2)) / 12, rtol=1e-5, atol=1e-6)
    opt = argparse.Namespace(path0=paths["kl_img0"], path1=paths["kl_img1"], device="cuda")
    assert abs(ev.kl_loss(opt, no_print=True) - float(g["kl_loss"])) <= 1e-3 * float(g["kl_loss"])


def test_sintel_temporal_error_isolates_the_metric(golden):
    from vst import ops
    from vst.adaattn import inference
    from vst.adaattn.evaluate import sintel_temporal_error
    from vst.synthetic import video_frames

    a = golden("aa_infer")
    sm, sv = int(a["a_meta"][0]), int(a["a_meta"][1])
    P = {k: v.detach() for k, v in oracle.seeded_params(shapes.stylizing_network(), sm).items()}
    scale, shift = (float(v) for v in a["a_conv8"])  # the inference fixture's last-conv change: outputs leave [0, 255]
    P["decoder.conv8.conv.weight"] = P["decoder.conv8.conv.weight"] * scale
    P["decoder.conv8.conv.bias"] = P["decoder.conv8.conv.bias"] + shift
    model = inference.load_model(P, "cosine")
    vgg = inference.load_vgg(oracle.seeded_params(shapes.vgg19(), sv))
    H, W = 64, 128
    clip = ops.frames_to_tensor(torch.from_numpy(video_frames(91, 3, H, W)).cuda())
    style = ops.frames_to_tensor(torch.from_numpy(video_frames(92, 1, H, W)).cuda())
    g = torch.Generator().manual_seed(93)
    pairs = []
    for i in range(2):
        flow = torch.randn(1, 2, H, W, generator=g) * 3
        mask = (torch.rand(1, H, W, generator=g) > 0.3).float()
        pairs.append((clip[i:i + 1], clip[i + 1:i + 2], flow.cuda(), mask.cuda()))
    got = sintel_temporal_error(model, vgg, style, pairs)
    assert got == sintel_temporal_error(model, vgg, style, iter(pairs))
    assert got == sintel_temporal_error(model, vgg, style, (p for p in pairs))
    # the restatement on the frames inference.stylize itself produced (a = cs2, warped = cs1)
    state = inference.encode_style(vgg, model, style)
    cpu = []
    for c1, c2, flow, mask in pairs:
        cs1, cs2 = (inference.stylize(vgg, model, state, c).cpu() for c in (c1, c2))
        assert float(cs1.min()) < 0 and float(cs1.max()) > 255
        cpu.append((cs2, cs1, flow.cpu(), mask.cpu()))
    exact = M.temporal_error(cpu, 1, True, "aa", torch.float64)
    ref32 = M.temporal_error(cpu, 1, True, "aa", torch.float32)
    _bar(got, ref32, exact, "sintel_temporal_error")
