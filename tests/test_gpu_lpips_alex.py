"""LPIPS over the AlexNet trunk on the GPU (vst.lpips net="alex", csrc/alex.hip): the stem and the pool
kernel on their own, and the model against the reference's own outputs in tests/golden/lpips_alex.npz.

Bars.  The stem is held to the suite's single-kernel bar (tests/test_gpu_lpips.py `_bar`, REF_X = 4, FLOOR =
1e-6): at most 4x as far from float64 `F.conv2d` as torch-CPU's fp32 `F.conv2d` on the same inputs, floored
at 1e-6 of the largest exact value.  The pool is bit-exact.  The model is held to the project's
model-versus-golden bar, 1e-3 relative, under the f32 and bf16x6 policies.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_alex_ref as A
import lpips_ref as L
from conftest import PKG
from test_gpu_lpips import GOLDEN_REL, _bar, _close

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# the stem
# (N, H, W, Cout).  The kernel's block tile is 8 x 32 outputs: 31 x 31 is a 7 x 7 grid where every output
# touches padding; 47 x 70 has W % 4 != 0 and an unread trailing column; 11 x 7 is the minimum width (Ho = 2,
# Wo = 1); 139 x 263 gives 34 x 65 outputs, 5 x 3 block tiles that end in partial ones in both directions
# (34 = 4 * 8 + 2, 65 = 2 * 32 + 1) -- the tile is not larger than 32 x 64, so the issue's shape stands.
STEM_SHAPES = [(1, 31, 31, 64), (2, 35, 67, 64), (1, 47, 70, 16), (1, 11, 7, 16), (3, 139, 263, 64)]
_STEM = {}


def _stem_case(shape):
    """Inputs on the host and the device and the two CPU references (without bias / ReLU), computed once."""
    if shape not in _STEM:
        N, H, W, Cout = shape
        x, w, b = A.stem_inputs(N, H, W, Cout)
        assert float(x.min()) < -2.0 and float(x.max()) > 2.5
        _STEM[shape] = dict(host=(x, w, b), dev=tuple(t.cuda() for t in (x, w, b)),
                            r64=F.conv2d(x.double(), w.double(), None, stride=4, padding=2),
                            r32=F.conv2d(x, w, None, stride=4, padding=2))
    return _STEM[shape]


def _stem(x, w, b, relu):
    from vst._lib import lib, ptr, stream

    N, _, H, W = x.shape
    Cout = w.shape[0]
    out = torch.full((N, Cout, (H - 7) // 4 + 1, (W - 7) // 4 + 1), float("nan"), device=x.device)
    lib.vst_conv_cin3_k11s4(ptr(x), ptr(w), ptr(b), ptr(out), N, H, W, Cout, int(relu), stream())
    return out


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_vs_float64(shape, bias, relu):
    d = _stem_case(shape)
    x, w, b = d["dev"]
    got = _stem(x, w, b if bias else None, relu)
    r64, r32 = d["r64"], d["r32"]
    if bias:
        r64, r32 = r64 + d["host"][2].double().view(1, -1, 1, 1), r32 + d["host"][2].view(1, -1, 1, 1)
    if relu:
        r64, r32 = torch.relu(r64), torch.relu(r32)
    assert got.shape == r64.shape
    _bar(got.cpu().numpy(), r32.numpy(), r64.numpy(), f"stem {shape} bias={bias} relu={relu}")
    if relu:
        assert float(got.min()) == 0.0  # both signs before the ReLU


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_image_of_a_batch_is_bitwise_the_image_alone(shape):
    x, w, b = _stem_case(shape)["dev"]
    full = _stem(x, w, b, True)
    assert torch.equal(_stem(x, w, b, True), full)  # run to run
    for n in range(shape[0]):
        assert torch.equal(_stem(x[n:n + 1].contiguous(), w, b, True), full[n:n + 1]), n
    # the ops wrapper, and the channel groups on their own: 16 channels of 64 are the same chains
    from vst import ops

    assert torch.equal(ops.conv_cin3_k11s4(x, w, b, relu=True), full)
    if shape[3] == 64:
        assert torch.equal(_stem(x, w[16:32].contiguous(), b[16:32].contiguous(), True), full[:, 16:32])


def test_stem_never_reads_past_the_last_window():
    """50 x 70 gives 11 x 16 outputs: the last window ends at row 4 * 10 - 2 + 10 = 48 and at column 4 * 15 - 2 +
    10 = 68, so row 49 and column 69 are unread.  NaN there reaches no output, and the result is that of the
    49 x 69 crop."""
    x, w, b = A.stem_inputs(1, 50, 70, 16)
    x[:, :, 49, :] = float("nan")
    x[:, :, :, 69] = float("nan")
    got = _stem(x.cuda(), w.cuda(), b.cuda(), False)
    assert got.shape == (1, 16, 11, 16) and torch.isfinite(got).all()
    assert torch.equal(got, _stem(x[:, :, :49, :69].contiguous().cuda(), w.cuda(), b.cuda(), False))


# ------------------------------------------------------------------------------------------------
# the pool
POOL_SHAPES = [(3, 3, 3), (5, 7, 7), (192, 8, 16), (2, 15, 23), (1, 4, 70), (64, 34, 65)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_is_torch_bit_for_bit(shape):
    from vst import ops
    from vst._lib import lib, ptr, stream

    NC, H, W = shape
    g = torch.Generator().manual_seed(100 + NC + H * W)
    x = torch.randn(NC, H, W, generator=g)
    assert float(x.min()) < 0 < float(x.max())
    # a plane of ties (few distinct values of both signs, signed zeros among them) and an all-negative plane
    x[0] = torch.randint(-2, 3, (H, W), generator=g).float() * 0.5
    x[0, 0, 0] = -0.0
    if NC > 1:
        x[1] = -x[1].abs() - 1.0
    want = F.max_pool2d(x.unsqueeze(0), 3, 2)[0]
    xd = x.cuda()
    out = torch.full(want.shape, float("nan"), device="cuda")
    lib.vst_maxpool3x3s2_fwd(ptr(xd), ptr(out), NC, H, W, stream())
    assert out.shape == (NC, (H - 3) // 2 + 1, (W - 3) // 2 + 1)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(ops.maxpool3x3s2(xd.view(1, NC, H, W)).cpu()[0], want)


# ------------------------------------------------------------------------------------------------
# the model against the reference's outputs
def _model(g, cls=None, **kw):
    from vst.lpips import LPIPS

    model = (cls or LPIPS)(net="alex", pretrained=False, verbose=False, **kw)
    model.net.load_state_dict(A.trunk_params(int(g["trunk_seed"])))
    if kw.get("lpips", True):
        model.load_state_dict({f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1)
                               for k in range(5)}, strict=False)
    return model.cuda()


@pytest.mark.parametrize("key", list(A.PAIRS))
def test_model_matches_the_reference(golden, step_policy, key):
    g = golden("lpips_alex")
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
    for n in range(N):  # the batch against its images run singly (the trunk's GEMMs may split differently)
        one = model(t0[n:n + 1].contiguous(), t1[n:n + 1].contiguous())
        _close(one.reshape(-1).cpu().numpy(), val[n].reshape(-1).cpu().numpy(), f"{key} image {n} alone", rel=1e-5)
    assert float(model(t0, t0.clone()).abs().max()) == 0.0  # identical images
    norm = model(L.unit01(img0).cuda(), L.unit01(img1).cuda(), normalize=True)
    _close(norm.reshape(-1).cpu().numpy(), g[key + "_norm01"], f"{key} normalize=True")
    _close(_model(g, lpips=False)(t0, t1).reshape(-1).cpu().numpy(), g[key + "_baseline"], f"{key} lpips=False")
    _close(_model(g, version="0.0")(t0, t1).reshape(-1).cpu().numpy(), g[key + "_v00"], f"{key} version 0.0")
    u8 = model.forward_u8(torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda(), bgr=False)
    assert torch.equal(u8, val)  # the uint8 entry builds the same trunk input bit for bit
    feats = model.net(model.scaling_layer(t0))
    assert tuple(tuple(f.shape[2:]) for f in feats) == A.GRIDS[key] and type(feats).__name__ == "AlexnetOutputs"


def test_spatial_map(golden, step_policy):
    g = golden("lpips_alex")
    model = _model(g, spatial=True)
    t0, t1 = L.im2tensor(g["a35_img0"]).cuda(), L.im2tensor(g["a35_img1"]).cuda()
    val, res = model(t0, t1, retPerLayer=True)
    want = g["a35_spatial"]
    assert val.shape == (2, 1, 35, 67) and len(res) == 5
    err = float(np.abs(val.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"alex spatial map {step_policy}: {err:.2e} of the map's maximum")
    assert err <= GOLDEN_REL
    assert float((sum(r.cpu() for r in res) - val.cpu()).abs().max()) <= 1e-6 * float(np.abs(want).max())


def test_metrics_and_drop_in(golden, step_policy, tmp_path):
    import vst.lpips
    from vst.metrics import LPIPSMean, lpips_distance

    g = golden("lpips_alex")
    model = _model(g)
    mean = LPIPSMean(model, bgr=True)
    singles, wants = [], []
    for key in A.PAIRS:
        # cv2-order frames: the fixture's RGB reversed
        f0, f1 = (torch.from_numpy(np.ascontiguousarray(g[f"{key}_img{i}"][..., ::-1])).cuda() for i in (0, 1))
        d = lpips_distance(model, f0, f1, bgr=True)
        assert d.shape == (f0.shape[0],)
        fwd = model(L.im2tensor(g[key + "_img0"]).cuda(), L.im2tensor(g[key + "_img1"]).cuda())
        assert torch.equal(d, fwd.reshape(-1))
        _close(d.cpu().numpy(), g[key + "_total"], f"lpips_distance {key} {step_policy}")
        assert mean.update(f0, f1) is mean
        singles += d.cpu().tolist()
        wants += g[key + "_total"].tolist()
    acc, pairs = mean.state()
    assert pairs == 4 and acc.shape == (1,)
    got = mean.result()
    assert abs(got - float(np.mean(singles))) <= 1e-6 * float(np.mean(singles))
    assert abs(got - float(np.mean(wants))) <= GOLDEN_REL * float(np.mean(wants))

    # the drop-in package's default constructor: lpips.LPIPS(...) is the alex model, its linear layers from a file
    spec = importlib.util.spec_from_file_location("adaattn_lpips_shim_alex", os.path.join(PKG, "adaattn/lpips/__init__.py"))
    pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    assert pkg.LPIPS is vst.lpips.LPIPS and pkg.alexnet is vst.lpips.alexnet
    path = str(tmp_path / "alex.pth")
    torch.save({f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1) for k in range(5)}, path)
    drop = pkg.LPIPS(model_path=path, verbose=False)
    assert drop.pnet_type == "alex"
    drop.net.load_state_dict(A.trunk_params(int(g["trunk_seed"])))
    drop = drop.cuda()
    t0, t1 = pkg.im2tensor(g["a64_img0"][0]).cuda(), pkg.im2tensor(g["a64_img1"][0]).cuda()
    assert torch.equal(drop(t0, t1), model(t0, t1))
    _close(drop(t0, t1).reshape(-1).cpu().numpy(), g["a64_total"], f"drop-in a64 {step_policy}")


def test_what_raises_on_the_gpu(golden):
    from vst._lib import VstError
    from vst.lpips import LPIPS, PerceptualLoss

    model = _model(golden("lpips_alex"))
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    for call in (lambda: model.encode(x), lambda: model.distance_to(None, x), lambda: PerceptualLoss(model),
                 lambda: model.encode_u8(torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(VstError, match="forward only"):
            call()
    small = torch.zeros(1, 3, 30, 40, device="cuda")
    with pytest.raises(VstError, match="31"):
        model(small, small)
    with pytest.raises(VstError, match="31"):
        model(small.transpose(2, 3).contiguous(), small.transpose(2, 3).contiguous())
    with pytest.raises(VstError, match="31"):
        model.forward_u8(torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device="cuda"),
                         torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device="cuda"))
    xg = torch.zeros(1, 3, 32, 32, device="cuda", requires_grad=True)
    with pytest.raises(VstError, match="grad"):
        model(xg, x)
    # the VGG model keeps its own minimum
    # (seeded trunk and the plain channel sum: a sum of squares, positive for two different images, whereas
    # the randomly initialised linear layers of pretrained=False may have either sign)
    vgg = LPIPS(net="vgg", pretrained=False, lpips=False, verbose=False)
    vgg.net.load_state_dict(L.trunk_params())
    vgg = vgg.cuda()
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(1, 3, 16, 16, generator=g).cuda() * 2 - 1, torch.rand(1, 3, 16, 16, generator=g).cuda() * 2 - 1
    v = vgg(a, b)
    assert v.shape == (1, 1, 1, 1) and torch.isfinite(v).all() and float(v) > 0.0
    with pytest.raises(VstError, match="16"):
        vgg(a[:, :, :15].contiguous(), b[:, :, :15].contiguous())
