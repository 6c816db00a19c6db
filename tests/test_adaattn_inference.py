"""AdaAttN inference (AA/infer_video.py, AA/infer_image.py): the thin-output forward conv
(`vst_conv_thin_fwd`), the cached style state and `VideoInference` / `stylize_image`, against
tests/golden/aa_infer.npz made by running the reference's own per-frame chain
(tests/golden/gen_golden_aa_infer.py: seeded VGG19 + StylizingNetwork whose last conv is rescaled so
the uint8 frames are not trivial; case a cosine 3 x 32x64, case b softmax 2 x 48x80 over a 32x64 style).

Tolerances:
  * thin forward vs float64: the fp32 bound of ANY summation order of a 9*Cin-term dot product plus
    the partial sums' adds and the bias, |err| <= (9*Cin + 2) * 2^-24 * (|x| (*) |w| + |b|), per element;
  * fused frames, batch invariance, cached attention vs the module: bitwise;
  * stylised uint8 frames: |diff| <= 1 and <= 1 % of the bytes differing (the project's bar for
    inference frames, tests/test_inference.py; the reference and the fp32 oracle alone differ in
    <= 0.25 %, asserted by the generator and below), pre-clamp fp32 output within 1e-3 relative
    (the fp32 contract).  The measured shares are recorded in DESIGN.md (AdaAttN inference).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from conftest import rel_err
from oracle import adaattn_ref as A
from oracle import shapes
from vst import _lib
from vst.synthetic import video_frames


# ---------------------------------------------------------------------------------------------
# the fixture's cases
def _case(golden, tag):
    g = golden("aa_infer")
    sm, sv, svid, ssty, T, H, W, Hs, Ws = (int(v) for v in g[f"{tag}_meta"])
    clip = video_frames(svid, T, H, W)
    pic = np.random.default_rng(ssty).integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8)
    return g, str(g[f"{tag}_activation"]), (sm, sv), clip, pic


_PARAMS = {}


def _params(golden, tag):
    """(stylizer parameters with the fixture's last-conv change, VGG19 parameters), CPU, shared."""
    if tag not in _PARAMS:
        g, _, (sm, sv), _, _ = _case(golden, tag)
        P = {k: v.detach() for k, v in oracle.seeded_params(shapes.stylizing_network(), sm).items()}
        scale, shift = (float(v) for v in g[f"{tag}_conv8"])
        P["decoder.conv8.conv.weight"] = P["decoder.conv8.conv.weight"] * scale
        P["decoder.conv8.conv.bias"] = P["decoder.conv8.conv.bias"] + shift
        _PARAMS[tag] = (P, oracle.seeded_params(shapes.vgg19(), sv))
    return _PARAMS[tag]


def _to255(u8_hwc):
    """toTensor255 of an HxWx3 uint8 RGB array: ToTensor (x / 255) then mul(255), (1,3,H,W)."""
    return torch.from_numpy(np.ascontiguousarray(u8_hwc.transpose(2, 0, 1))).float().div(255).mul(255).unsqueeze(0)


def _frame_bars(frames, ref, what):
    d = np.abs(np.asarray(frames).astype(int) - ref.astype(int))
    share = float((d > 0).mean())
    print(f"{what}: max |diff| {d.max()}, differing share {share:.5f}")
    return int(d.max()), share


# ---------------------------------------------------------------------------------------------
# CPU
@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_matches_reference_frames(golden, tag):
    """Pins the oracle's restatement of the per-frame chain against the reference's own frames."""
    g, act, _, clip, pic = _case(golden, tag)
    P, VP = _params(golden, tag)
    with torch.no_grad():
        fs = A.vgg19(VP, _to255(pic))
        outs = [A.stylize(P, A.vgg19(VP, _to255(f[..., ::-1])), fs, act) for f in clip]
    frames = np.stack([y.clamp(0, 255)[0].permute(1, 2, 0).numpy().astype(np.uint8) for y in outs])
    dmax, share = _frame_bars(frames, g[f"{tag}_frames"], f"oracle {tag}")
    assert dmax <= 1 and share <= 0.0025
    assert rel_err(outs[0][0].numpy(), g[f"{tag}_pre0"]) < 1e-4


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built")
def test_thin_fwd_host_side_validation():
    """vst_conv_thin_fwd refuses unsupported shapes and output combinations before any launch."""
    lib = _lib.lib.load()
    x, w, b, out, fr = 4096, 8192, 12288, 16384, 20480  # never dereferenced: every call below is refused

    def call(N=1, Cin=4, H=8, W=16, Cout=3, out=out, frames=fr):
        return lib.vst_conv_thin_fwd(x, w, b, out, frames, N, Cin, H, W, Cout, 1, 0, None)

    assert call(Cout=0, frames=None) == -1
    assert call(Cout=5, frames=None) == -1
    assert call(W=6) == -1
    assert call(W=10) == -1
    assert call(H=1) == -1
    assert call(out=None, frames=None) == -1
    assert call(Cout=2) == -1  # frames need three channels
    assert call(Cin=0) == -1
    assert lib.vst_conv_thin_fwd(None, w, b, out, fr, 1, 4, 8, 16, 3, 1, 0, None) == -1
    assert lib.vst_conv_thin_fwd(x, None, b, out, fr, 1, 4, 8, 16, 3, 1, 0, None) == -1


def test_thin_fwd_in_header():
    protos = _lib.parse_header()
    assert "vst_conv_thin_fwd" in protos
    rt, args = protos["vst_conv_thin_fwd"]
    assert rt == "int" and args[-1] == "void*" and len(args) == 13


# ---------------------------------------------------------------------------------------------
# GPU: the thin forward kernel
# the issue's shapes, then one whose launch takes the 4-rows-per-lane tiling (>= 512 blocks of them)
THIN_SHAPES = [(2, 64, 9, 8, 3), (1, 6, 5, 44, 1), (1, 16, 18, 260, 4), (3, 2, 2, 12, 2), (1, 5, 7, 16, 3),
               (1, 3, 512, 1024, 3)]


def _thin_inputs(shape, seed, target_std=None):
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g)
    b = torch.randn(Cout, generator=g)
    if target_std is not None:  # outputs of about 130 +- 2 * 85: spans -40 .. 300
        w = w * (target_std / (9 * Cin) ** 0.5)
        b = b + 130.0
    return x, w, b


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("reflect", [True, False])
@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_thin_fwd_vs_float64(shape, reflect, bias):
    from vst import ops

    N, Cin, H, W, Cout = shape
    x, w, b = _thin_inputs(shape, 3)
    b = b if bias else None
    out = ops.conv_thin_fwd(x.cuda(), w.cuda(), None if b is None else b.cuda(), reflect=reflect).cpu().double()
    xp = F.pad(x.double(), (1, 1, 1, 1), mode="reflect" if reflect else "constant")
    ref = F.conv2d(xp, w.double(), None if b is None else b.double())
    mag = F.conv2d(xp.abs(), w.double().abs())
    if b is not None:
        mag = mag + b.double().abs().view(1, -1, 1, 1)
    bound = (9 * Cin + 2) * 2.0 ** -24 * mag
    err = (out - ref).abs()
    print(f"{shape} reflect={reflect} bias={bias}: max err / bound {float((err / bound).max()):.3f}")
    assert out.shape == ref.shape
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("shape", [(2, 64, 9, 8, 3), (1, 5, 7, 16, 3), (1, 3, 512, 1024, 3)])
def test_thin_fwd_fused_frames(shape, bgr):
    from vst import ops

    N, Cin, H, W, Cout = shape
    x, w, b = (t.cuda() for t in _thin_inputs(shape, 5, target_std=85.0))
    alone = ops.conv_thin_fwd(x, w, b)
    assert float(alone.min()) < -20 and float(alone.max()) > 275
    out = torch.empty_like(alone)
    frames = torch.zeros((N, H, W, 3), dtype=torch.uint8, device="cuda")
    ret = ops.conv_thin_fwd(x, w, b, out=out, frames=frames, bgr=bgr)
    assert ret is frames
    assert torch.equal(out, alone)
    assert torch.equal(frames, ops.tensor_to_frames(out, bgr=bgr))
    only = torch.zeros_like(frames)
    ops.conv_thin_fwd(x, w, b, frames=only, bgr=bgr)
    assert torch.equal(only, frames)
    # and the bytes are what numpy makes of the fp32 image
    ref = out.clamp(0, 255).permute(0, 2, 3, 1).cpu().numpy().astype(np.uint8)
    assert np.array_equal(frames.cpu().numpy(), ref[..., ::-1] if bgr else ref)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 6, 9, 24, 3), (3, 5, 688, 256, 3)])
def test_thin_fwd_batch_invariance(shape):
    """Image 1 of a batch of 3 is bitwise the image alone (the second shape runs 4 rows per lane as a
    batch and 2 rows per lane alone)."""
    from vst import ops

    x, w, b = (t.cuda() for t in _thin_inputs(shape, 9))
    batch = ops.conv_thin_fwd(x, w, b)
    alone = ops.conv_thin_fwd(x[1:2].contiguous(), w, b)
    assert torch.equal(batch[1:2], alone)


# ---------------------------------------------------------------------------------------------
# GPU: the cached style state
ATT_DIMS = [(2, 2, 40, 24, (5, 7), (6, 5)), (1, 1, 64, 32, (8, 16), (8, 16)), (2, 2, 16, 8, (1, 3), (2, 2)),
            (3, 1, 40, 24, (5, 7), (6, 5))]  # tests/test_gpu_adaattn.py's, then 3 contents over 1 style


@pytest.mark.gpu
@pytest.mark.parametrize("activation", ["cosine", "softmax"])
@pytest.mark.parametrize("dims", ATT_DIMS)
def test_cached_attention_equals_module(activation, dims):
    from vst.adaattn.attention import adaattn
    from vst.adaattn.inference import attend, style_level

    Nq, Nk, d, dv, (h, w), (hs, ws) = dims
    g = torch.Generator().manual_seed(7)
    Q = torch.randn(Nq, d, h, w, generator=g)
    K = torch.randn(Nk, d, hs, ws, generator=g)
    V = torch.rand(Nk, dv, hs, ws, generator=g) * 3
    cn = torch.randn(Nq, dv, h, w, generator=g)
    r = Nq // Nk
    Kf, Vf = K.repeat(r, 1, 1, 1), V.repeat(r, 1, 1, 1)
    with torch.no_grad():
        if activation == "cosine":
            mod = adaattn(Q.cuda(), K.cuda(), V.cuda(), cn.cuda(), activation)
        else:
            mod = adaattn(Q.cuda(), Kf.cuda(), Vf.cuda(), cn.cuda(), activation)
        level = style_level(K.cuda(), V.cuda(), activation)
        out = attend(level, activation, Q.cuda(), cn.cuda())
    assert not out.requires_grad
    assert torch.equal(out, mod)
    M, S = A.attention_moments(Q.double(), Kf.double(), Vf.double(), activation)
    ref = S * cn.double() + M
    assert rel_err(out.cpu().numpy(), ref.numpy()) < (1e-4 if activation == "cosine" else 5e-4)
    # the state holds what the issue lists and nothing of the style's size beyond it
    if activation == "cosine":
        G, ksum, us, Ns = level
        assert G.shape == (Nk, d, 2 * dv) and ksum.shape == (Nk, d) and us.shape == (Nk, 2 * dv) and Ns == hs * ws
    else:
        Kc, VV2 = level
        assert Kc.shape == (Nk, d, hs * ws) and VV2.shape == (Nk, 2 * dv, hs * ws)


# ---------------------------------------------------------------------------------------------
# GPU: end to end
def _style_arg(tag, pic):
    # case a's picture already has the frame size (a uint8 array: resized Pillow-exactly, here the
    # identity); case b's style keeps its own 32x64 (a ready tensor is taken as it is)
    return pic if tag == "a" else _to255(pic)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,batch", [("a", 1), ("a", 2), ("b", 1), ("b", 2)])
def test_video_inference_golden(golden, step_policy, tag, batch):
    from vst import ops
    from vst.adaattn.inference import VideoInference, stylize

    g, act, _, clip, pic = _case(golden, tag)
    P, VP = _params(golden, tag)
    H, W = clip.shape[1:3]
    vi = VideoInference(P, _style_arg(tag, pic), clip, activation=act, size=(H, W), batch_frames=batch, vgg=VP)
    outs = list(vi)
    ref = g[f"{tag}_frames"]
    assert len(outs) == len(ref)
    assert all(o.shape == (H, W, 3) and o.dtype == np.uint8 for o in outs)
    dmax, share = _frame_bars(np.stack(outs), ref, f"{tag} batch {batch} {step_policy}")
    assert dmax <= 1 and share <= 0.01, (dmax, share)
    c0 = ops.frames_to_tensor(torch.from_numpy(clip[:1].copy()).cuda())
    pre = stylize(vi.vgg, vi.model, vi.state, c0)
    e = rel_err(pre[0].cpu().numpy(), g[f"{tag}_pre0"])
    print(f"{tag} {step_policy}: pre-clamp rel err {e:.2e}")
    assert not pre.requires_grad and e < 1e-3
    if batch == 1:  # BGR frames are the RGB ones reversed
        bgr = list(VideoInference(P, _style_arg(tag, pic), clip[:1], activation=act, size=(H, W), bgr=True, vgg=VP))
        assert np.array_equal(bgr[0], outs[0][..., ::-1])


@pytest.mark.gpu
def test_stylize_image_golden(golden, step_policy):
    from vst.adaattn.inference import stylize_image

    g, act, _, clip, pic = _case(golden, "b")
    P, VP = _params(golden, "b")
    H, W = clip.shape[1:3]
    content = np.ascontiguousarray(clip[0][..., ::-1])  # cv2 BGR frame -> the RGB picture
    cs, u8 = stylize_image(P, VP, content, _to255(pic), activation=act, size=(H, W))
    assert cs.shape == (1, 3, H, W) and cs.dtype == torch.float32 and not cs.requires_grad
    assert u8.shape == (H, W, 3) and u8.dtype == np.uint8
    dmax, share = _frame_bars(u8, g["b_frames"][0], f"stylize_image {step_policy}")
    assert dmax <= 1 and share <= 0.01, (dmax, share)
    assert rel_err(cs[0].cpu().numpy(), np.clip(g["b_pre0"], 0, 255)) < 1e-3
    assert np.array_equal(u8, cs[0].permute(1, 2, 0).cpu().numpy().astype(np.uint8))


@pytest.mark.gpu
def test_style_input_forms(golden, tmp_path):
    from vst.adaattn.inference import encode_style, image_tensor, load_model, load_vgg

    P, VP = _params(golden, "a")
    model, vgg = load_model(P, "cosine"), load_vgg(VP)
    pic = np.random.default_rng(5).integers(0, 256, size=(40, 72, 3), dtype=np.uint8)
    size = (32, 64)
    forms = [pic]
    try:
        from PIL import Image
    except ImportError:  # (then only the array form exists to compare)
        pass
    else:
        img = Image.fromarray(pic)
        img.save(tmp_path / "style.png")
        forms += [img, str(tmp_path / "style.png"), tmp_path / "style.png"]
        want = _to255(np.asarray(img.resize((size[1], size[0]), Image.BILINEAR)))
        assert torch.equal(image_tensor(pic, size).cpu(), want)
    states = [encode_style(vgg, model, image_tensor(f, size)) for f in forms]
    for st in states[1:]:
        assert len(st.tensors()) == len(states[0].tensors()) == 9
        assert all(torch.equal(a, b) for a, b in zip(st.tensors(), states[0].tensors()))
    ready = image_tensor(pic, size)
    assert image_tensor(ready, (1, 1)).data_ptr() == ready.data_ptr()  # a ready tensor is taken as it is


@pytest.mark.gpu
def test_no_autograd_state_and_wrong_size(golden):
    from vst.adaattn.inference import VideoInference, encode_style, load_model, load_vgg, stylize
    from vst.adaattn.utilities import cv2_to_tensor

    g, act, _, clip, pic = _case(golden, "a")
    P, VP = _params(golden, "a")
    model, vgg = load_model(P, act), load_vgg(VP)
    assert all(p.requires_grad for p in model.parameters())
    state = encode_style(vgg, model, _to255(pic).cuda())
    assert not any(t.requires_grad for t in state.tensors())
    c = cv2_to_tensor(clip[0]).unsqueeze(0)
    assert c.is_cuda and torch.equal(c.cpu(), _to255(clip[0][..., ::-1]))
    y = stylize(vgg, model, state, c)
    assert not y.requires_grad and y.grad_fn is None
    frames = torch.empty((1, 32, 64, 3), dtype=torch.uint8, device="cuda")
    assert stylize(vgg, model, state, c, frames=frames) is frames
    assert np.array_equal(frames[0].cpu().numpy(), y.clamp(0, 255)[0].permute(1, 2, 0).cpu().numpy().astype(np.uint8))
    # a frame of another size needs cv2.resize (INTER_AREA) like the reference: absent -> ImportError
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            list(VideoInference(P, pic, video_frames(3, 1, 40, 72), activation=act, size=(32, 64), vgg=VP))
        with pytest.raises(ImportError):
            cv2_to_tensor(clip[0], resize=(72, 40))
