"""RTNSTV video inference on the GPU: the split-plane InstanceNorm forward (vst_instnorm_moments /
_apply / _tanh_frames), the uint8 stem (vst_conv_stem_u8), `forward_frames` and `Inference` against
tests/golden/rt_infer.npz (made by the reference's own Inference, tests/golden/gen_golden_rt_infer.py).

Tolerances (each computed in the test from float64 statistics of the test's own inputs):
  * chunk partials: fp64 sums of n terms in any order, |err| <= n * 2^-53 * sum |term|;
  * mean / rstd: 2^-22 relative to float64 numpy (inputs with |mean| <= 4 std, so the variance's
    cancellation costs fp64 bits only);
  * split apply vs ops.instance_norm: |dy| <= 2^-22 * (|xhat| + |mean| * rstd) * |w| per element -- one
    ulp of mean and one of rstd through in_affine -- and no ReLU decision flipped where the
    pre-activation is farther from 0 than that; chunks=1 is bitwise ops.instance_norm;
  * fused tail vs the three-kernel chain with the same chunks (for S > 1 the same partial sums, hence the
    same statistics; S = 1 is that chain): byte for byte;
  * stem vs float64: |err| <= 28 * 2^-24 * (|W| (*) |X| + |b|), 27 FMAs and one add; a frame in a batch
    bitwise the frame alone;
  * stylised uint8 frames: |diff| <= 1 and <= 1 % of the bytes differing (the project's bar for
    inference frames; the restatement and the reference alone differ in <= 0.25 %, asserted by the
    generator), between batch sizes too (the GEMM convs' split over channel blocks depends on the
    launch size, so batch 2 is not bitwise batch 1).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rt_infer_ref as ref

pytestmark = pytest.mark.gpu

PROD = (1, 3, 360, 640)  # conv4's output at the reference's frame size


def _planes(shape, seed):
    """Planes with per-plane mean in [-4, 4] std and std in [0.5, 2]."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    std = 0.5 + 1.5 * torch.rand(N, C, 1, 1, generator=g)
    mean = (8 * torch.rand(N, C, 1, 1, generator=g) - 4) * std
    return torch.randn(N, C, H, W, generator=g) * std + mean


def _chunk_bounds(HW, S, k):
    if HW % 4 == 0:
        n4 = HW // 4
        return n4 * k // S * 4, n4 * (k + 1) // S * 4
    return HW * k // S, HW * (k + 1) // S


def _stats64(x, eps=1e-5):
    x64 = x.double().flatten(2)
    mean = x64.mean(2)
    var = (x64 * x64).mean(2) - mean * mean
    return mean, 1.0 / torch.sqrt(var.clamp_min(0) + eps)


def _split_cases():
    from vst import ops

    return [((1, 3, 36, 52), 1), ((1, 3, 36, 52), 2), ((1, 3, 36, 52), 7), ((2, 2, 5, 7), 1), ((2, 2, 5, 7), 3),
            (PROD, ops.instnorm_chunks(3, 360 * 640))]


@pytest.mark.parametrize("case", range(6))
def test_moments_and_stats_vs_float64(case):
    from vst import _lib

    shape, S = _split_cases()[case]
    N, C, H, W = shape
    HW, planes = H * W, N * C
    if shape == PROD:
        assert S > 1, "the production geometry of the tail is split"
    x = _planes(shape, 11 + case)
    xd = x.cuda()
    part = torch.full((planes * S * 2,), float("nan"), dtype=torch.float64, device="cuda")
    lib, st = _lib.lib, _lib.stream()
    lib.vst_instnorm_moments(xd.data_ptr(), part.data_ptr(), planes, HW, S, st)
    got = part.cpu().view(planes, S, 2)
    x64 = x.double().view(planes, HW)
    for k in range(S):
        lo, hi = _chunk_bounds(HW, S, k)
        c = x64[:, lo:hi]
        n = max(hi - lo, 1)
        assert bool(((got[:, k, 0] - c.sum(1)).abs() <= n * 2.0 ** -53 * c.abs().sum(1) + 1e-300).all()), k
        assert bool(((got[:, k, 1] - (c * c).sum(1)).abs() <= n * 2.0 ** -53 * (c * c).sum(1) + 1e-300).all()), k
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    y = torch.empty_like(xd)
    stats = torch.full((planes * 2,), float("nan"), device="cuda")
    lib.vst_instnorm_apply(xd.data_ptr(), part.data_ptr(), w.data_ptr(), b.data_ptr(), None, y.data_ptr(),
                           stats.data_ptr(), N, C, HW, S, 1e-5, 0, st)
    mean, rstd = _stats64(x)
    s = stats.cpu().double().view(N, C, 2)
    em = float(((s[..., 0] - mean).abs() / mean.abs()).max())
    er = float(((s[..., 1] - rstd).abs() / rstd).max())
    print(f"{shape} S={S}: mean rel err {em:.2e}, rstd rel err {er:.2e} (bar {2.0 ** -22:.2e})")
    assert em <= 2.0 ** -22 and er <= 2.0 ** -22
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("relu,with_res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("case", [1, 2, 4, 5])
def test_split_apply_vs_instance_norm(case, relu, with_res):
    from vst import ops

    shape, S = _split_cases()[case]
    N, C, H, W = shape
    g = torch.Generator().manual_seed(23 + case)
    x = _planes(shape, 17 + case)
    w = 1.0 + 0.3 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    res = torch.randn(shape, generator=g) if with_res else None
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    rd = res.cuda() if with_res else None
    with torch.no_grad():
        want = ops.instance_norm(xd, wd, bd, relu=relu, res=rd)
    got = ops.instance_norm_infer(xd, wd, bd, relu=relu, res=rd, chunks=S)
    assert not got.requires_grad and got.shape == want.shape
    assert torch.equal(ops.instance_norm_infer(xd, wd, bd, relu=relu, res=rd, chunks=1), want)
    mean, rstd = _stats64(x)
    mean, rstd = mean.view(N, C, 1, 1), rstd.view(N, C, 1, 1)
    xhat = (x.double() - mean) * rstd
    w64 = w.double().view(1, C, 1, 1)
    bound = 2.0 ** -22 * (xhat.abs() + mean.abs() * rstd) * w64.abs()
    err = (got.cpu().double() - want.cpu().double()).abs()
    print(f"{shape} S={S} relu={relu} res={with_res}: max |dy| / bound {float((err / bound).max()):.3f}, "
          f"bitwise equal {bool(torch.equal(got, want))}")
    assert bool((err <= bound).all()), float((err / bound).max())
    if relu and not with_res:
        pre = xhat * w64 + b.double().view(1, C, 1, 1)
        sure = pre.abs() > bound
        assert bool(((got.cpu() > 0) == (want.cpu() > 0))[sure].all())
        assert bool(((got.cpu() > 0) == (pre > 0))[sure].all())


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("shape,chunks", [((2, 3, 36, 52), 2), ((2, 3, 36, 52), 7), ((2, 3, 36, 52), None),
                                          ((2, 3, 5, 7), 3), (PROD, None), (PROD, 24)])  # 5x7: the byte-wise path
def test_fused_tail_equals_three_kernels(shape, chunks, bgr):
    from vst import ops

    g = torch.Generator().manual_seed(31)
    z = (_planes(shape, 29) * 3).cuda()
    w = (1.0 + 0.3 * torch.randn(3, generator=g)).cuda()
    b = (0.3 * torch.randn(3, generator=g)).cuda()
    if chunks is None:  # the rule: the production frame is split, the small one stays on vst_instnorm_fwd
        assert (ops.instnorm_chunks(3, shape[2] * shape[3]) > 1) == (shape == PROD)
    frames = ops.instance_norm_tanh_frames(z, w, b, bgr=bgr, chunks=chunks)
    with torch.no_grad():
        img = ops.tanh_image(ops.instance_norm_infer(z, w, b, chunks=chunks), image=True)
    want = ops.tensor_to_frames(img, bgr=bgr)
    assert frames.dtype == torch.uint8 and frames.shape == (shape[0], shape[2], shape[3], 3)
    assert torch.equal(frames, want)
    lv = len(torch.unique(frames))
    assert lv >= (150 if frames.numel() > 10000 else 50), lv  # not a trivial image
    # and the bytes are what numpy makes of the fp32 image
    u8 = img.permute(0, 2, 3, 1).cpu().numpy().astype(np.uint8)
    assert np.array_equal(frames.cpu().numpy(), u8[..., ::-1] if bgr else u8)
    out = torch.zeros_like(frames)
    assert ops.instance_norm_tanh_frames(z, w, b, bgr=bgr, frames=out, chunks=chunks) is out
    assert torch.equal(out, want)


def _stem_inputs(N, H, W, Cout, seed):
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8))
    g = torch.Generator().manual_seed(seed)
    return frames, torch.randn(Cout, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5, torch.randn(Cout, generator=g)


def _stem_ref(frames, w, b, bgr):
    rgb = frames.flip(-1) if bgr else frames
    x = rgb.permute(0, 3, 1, 2).float().div(255).mul(255).double()  # toTensor255
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    ref64 = F.conv2d(xp, w.double(), b.double())
    mag = F.conv2d(xp.abs(), w.double().abs()) + b.double().abs().view(1, -1, 1, 1)
    return ref64, 28 * 2.0 ** -24 * mag


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("Cout", [4, 16])
@pytest.mark.parametrize("NHW", [(2, 6, 8), (1, 36, 52), (1, 6, 10)])
def test_stem_vs_float64(NHW, Cout, bgr):
    """(1, 6, 10): W % 4 != 0, the frames_to_tensor + conv2d fallback, under the same bound."""
    from vst import ops

    N, H, W = NHW
    assert ops.conv_stem_u8_ok(Cout, H, W, N) == (W % 4 == 0)
    frames, w, b = _stem_inputs(N, H, W, Cout, 41)
    out = ops.conv_stem_u8(frames.cuda(), w.cuda(), b.cuda(), bgr=bgr)
    assert out.shape == (N, Cout, H, W) and out.dtype == torch.float32 and not out.requires_grad
    ref64, bound = _stem_ref(frames, w, b, bgr)
    err = (out.cpu().double() - ref64).abs()
    print(f"{NHW} Cout={Cout} bgr={bgr}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    if N == 2:
        alone = ops.conv_stem_u8(frames[1:2].contiguous().cuda(), w.cuda(), b.cuda(), bgr=bgr)
        assert torch.equal(out[1:2], alone)


def test_stem_is_the_frame_kernel_plus_conv_in_one_order():
    """out= is honoured, no bias is no add, and the kernel's X is vst_frames_to_tensor's (the table in LDS
    holds the same (v / 255) * 255): the float64 conv of those planes bounds it as above."""
    from vst import ops

    frames, w, b = _stem_inputs(1, 36, 52, 8, 43)
    fd, wd = frames.cuda(), w.cuda()
    out = torch.zeros((1, 8, 36, 52), device="cuda")
    assert ops.conv_stem_u8(fd, wd, None, out=out) is out
    x = ops.frames_to_tensor(fd, bgr=True).cpu().double()
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    bound = 27 * 2.0 ** -24 * F.conv2d(xp.abs(), w.double().abs())
    assert bool(((out.cpu().double() - F.conv2d(xp, w.double())).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------
# end to end
_RUNS = {}


def _run(golden, tag, batch):
    from vst.rtnstv.inference import Inference
    from vst.rtnstv.network import StylizingNetwork

    if (tag, batch) not in _RUNS:
        g = golden("rt_infer")
        clip = ref.case_clip(tag, g[f"{tag}_meta"])
        inf = Inference(StylizingNetwork, ref.case_params(g, tag), clip, "cuda", batch_frames=batch,
                        resize=(640, 360) if tag == "a" else None)
        _RUNS[(tag, batch)] = (clip, list(inf))
    return _RUNS[(tag, batch)]


@pytest.mark.parametrize("tag,batch", [("a", 1), ("a", 2), ("b", 1), ("b", 2)])
def test_inference_golden(golden, tag, batch):
    g = golden("rt_infer")
    clip, outs = _run(golden, tag, batch)
    assert len(outs) == int(g[f"{tag}_n_out"]) == len(clip)
    assert all(o.shape == clip.shape[1:] and o.dtype == np.uint8 for o in outs)
    dmax, share = ref.case_bars(g, tag, np.stack(outs), f"Inference {tag} batch {batch}")
    assert dmax <= 1 and share <= 0.01, (dmax, share)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_inference_batch_sizes_agree(golden, tag):
    _, one = _run(golden, tag, 1)
    _, two = _run(golden, tag, 2)
    dmax, share = ref.frame_bars(np.stack(two), np.stack(one), f"Inference {tag} batch 2 vs 1")
    assert dmax <= 1 and share <= 0.01, (dmax, share)


def test_cvframe_to_tensor_and_wrong_sizes(golden):
    from vst._lib import VstError
    from vst.rtnstv.inference import Inference, cvframe_to_tensor
    from vst.rtnstv.network import StylizingNetwork

    g = golden("rt_infer")
    clip = ref.case_clip("b", g["b_meta"])
    t = cvframe_to_tensor(clip[0])
    assert t.is_cuda and t.shape == (3, 36, 52)
    assert torch.equal(t.cpu(), ref.to255(clip[0][..., ::-1])[0])
    assert torch.equal(cvframe_to_tensor(clip[0], resize=(52, 36)), t)
    with pytest.raises(VstError):  # 38 rows do not come back from the two stride-2 stages
        list(Inference(StylizingNetwork, ref.case_params(g, "b"), np.zeros((1, 38, 52, 3), np.uint8), resize=None))
    try:
        import cv2  # noqa: F401
    except ImportError:  # a frame of another size needs cv2.resize like the reference: absent -> ImportError
        with pytest.raises(ImportError):
            list(Inference(StylizingNetwork, ref.case_params(g, "b"), clip))


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np, torch
import rt_infer_ref as ref
from vst import ops
from vst.rtnstv.inference import forward_frames
from vst.rtnstv.network import StylizingNetwork
assert not ops.IN_SPLIT and ops.instnorm_chunks(3, 230400) == 1
g = dict(np.load({npz!r}))
model = StylizingNetwork().cuda()
model.load_state_dict(ref.case_params(g, "b"))
clip = ref.case_clip("b", g["b_meta"])
out = forward_frames(model, torch.from_numpy(clip).cuda(), bgr=True)
np.save({out!r}, out.cpu().numpy())
"""


def test_fallback_without_split_in_child(golden, tmp_path):
    """VST_IN_SPLIT=0 (read at import, so in a fresh child): every norm on vst_instnorm_fwd, the tail as
    three kernels -- the same bar on case b."""
    tests = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests)
    out = str(tmp_path / "frames.npy")
    code = _CHILD.format(paths=[tests, repo, os.path.join(repo, "video-style-transfer_amd")],
                         npz=os.path.join(tests, "golden", "rt_infer.npz"), out=out)
    env = dict(os.environ, VST_IN_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    g = golden("rt_infer")
    dmax, share = ref.case_bars(g, "b", np.load(out), "forward_frames VST_IN_SPLIT=0")
    assert dmax <= 1 and share <= 0.01, (dmax, share)
