"""CPU checks of the evaluation metrics' test yardstick and host-side pieces (no GPU):

  * tests/metrics_ref.py, the restatement the GPU tests measure against, reproduces every value of
    tests/golden/eval_metrics.npz (the reference's own outputs, tests/golden/gen_golden_eval.py): in
    float32, its own arithmetic, to 1e-6 relative; in float64 to 1e-5 (the golden values are fp32
    results: an fp32 mean of ~6000 terms or a 121-tap fp32 window sits up to a few 1e-7 from exact;
    the Gram distance, a VGG19 forward deep, to 1e-4); KL, float64 on integers in both, to 1e-12;
  * `read_sintel_flow` round-trips a file and raises the reference's four errors;
  * the header declares the three new entries, stream last; bad arguments fail before any launch.
"""
import os
import struct

import numpy as np
import pytest
import torch

import metrics_ref as M
import oracle
from oracle import shapes
from vst import _lib
from vst.metrics import read_sintel_flow


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def scene_pairs(g, scene):
    """The fixture's scene as (a, b, flow planar, mask) CPU tensors: the reference's styled frames,
    its 1/255 mask (ToTensor of a uint8 array)."""
    styled = torch.from_numpy(g[f"te_{scene}_styled"])
    flows, occ = g[f"te_{scene}_flows"], g[f"te_{scene}_occ"]
    out = []
    for i in range(len(flows)):
        flow = torch.from_numpy(flows[i].transpose(2, 0, 1).copy()).unsqueeze(0)
        mask = torch.from_numpy((occ[i] == 0).astype(np.float32) / np.float32(255)).unsqueeze(0)
        out.append((styled[i:i + 1], styled[i + 1:i + 2], flow, mask))
    return out


@pytest.mark.parametrize("scene", list(M.SCENES))
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-5)])
def test_temporal_restatement_matches_reference(golden, scene, dtype, tol):
    g = golden("eval_metrics")
    pairs = scene_pairs(g, scene)
    means = [M.temporal_pair_sum(*p, power=2, clamp_unit=False, dtype=dtype, mean=True) for p in pairs]
    assert _rel(means, g[f"te_{scene}_pair_means"]) < tol
    err = M.temporal_error(pairs, 2, False, "rt", dtype)
    assert abs(err - float(g[f"te_{scene}_error"])) < tol * err
    # the synthetic scene is what the generator wrote
    frames, occ, flows = M.sintel_scene(scene)
    assert np.array_equal(frames, g[f"te_{scene}_frames"]) and np.array_equal(occ, g[f"te_{scene}_occ"])
    assert np.array_equal(flows, g[f"te_{scene}_flows"])
    assert 0.25 < (occ == 255).mean() < 0.35


def test_temporal_conventions():
    """"aa" is the root of the SUM over pairs divided by the count, "rt" the root of the mean."""
    gen = torch.Generator().manual_seed(1)
    pairs = []
    for _ in range(3):
        a, b = torch.rand(1, 3, 6, 8, generator=gen) * 300 - 20, torch.rand(1, 3, 6, 8, generator=gen) * 300 - 20
        pairs.append((a, b, torch.randn(1, 2, 6, 8, generator=gen), (torch.rand(1, 6, 8, generator=gen) > 0.3).float()))
    sums = [M.temporal_pair_sum(*p, power=1, clamp_unit=True, dtype=torch.float64) for p in pairs]
    assert abs(M.temporal_error(pairs, 1, True, "aa", torch.float64) - np.sqrt(sum(sums)) / 3) < 1e-15
    assert abs(M.temporal_error(pairs, 1, True, "rt", torch.float64) - np.sqrt(sum(sums) / 3)) < 1e-12
    assert all(0 < s < 1 for s in sums)  # clamp_unit: differences of values in [0, 1]


@pytest.mark.parametrize("key,shape,kind,seed", M.ssim_cases())
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-5)])
def test_ssim_restatement_matches_reference(golden, key, shape, kind, seed, dtype, tol):
    g = golden("eval_metrics")
    x, y = M.ssim_inputs(shape, kind, seed)
    assert _rel(M.ssim(x, y, dtype=dtype).numpy(), g[key + "_none"]) < tol
    assert _rel(M.ssim(x, y, dtype=dtype, reduction="mean").item(), g[key + "_mean"]) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-4)])
def test_gram_restatement_matches_reference(golden, dtype, tol):
    g = golden("eval_metrics")
    VP = oracle.seeded_params(shapes.vgg19(), int(g["vgg_seed"]))
    img, style = (M.to255(g[k][..., ::-1]) for k in ("gram_img0", "gram_img1"))  # BGR file bytes -> RGB planes
    assert _rel(M.gram_distance(VP, img, style, dtype), g["gram_loss"]) < tol


def test_ssim_loss_restatement_matches_reference(golden):
    g = golden("eval_metrics")
    img, style = (M.to255(g[k]) for k in ("gram_img0", "gram_img1"))
    assert _rel(M.ssim(img, style, reduction="mean").item(), g["gram_ssim"]) < 1e-6


def test_kl_restatement_matches_reference(golden):
    g = golden("eval_metrics")
    assert abs(M.kl(g["kl_img0"], g["kl_img1"]) - float(g["kl_loss"])) < 1e-12
    from vst.metrics import _entropy

    h0, h1 = M.histograms(g["kl_img0"]) + 1, M.histograms(g["kl_img1"]) + 1
    assert abs(sum(_entropy(h0[c], h1[c]) for c in range(3)) / 3 - float(g["kl_loss"])) < 1e-12


# ------------------------------------------------------------------------------------------------
def test_read_sintel_flow_round_trip_and_errors(tmp_path):
    flow = np.random.default_rng(0).standard_normal((5, 7, 2)).astype(np.float32)
    p = tmp_path / "a.flo"
    M.write_flo(p, flow)
    got = read_sintel_flow(p)
    assert got.dtype == np.float32 and got.shape == (5, 7, 2) and np.array_equal(got, flow)
    assert got.flags["C_CONTIGUOUS"] and got.flags["WRITEABLE"]
    raw = p.read_bytes()

    def bad(name, data, msg):
        q = tmp_path / name
        q.write_bytes(data)
        with pytest.raises(ValueError) as e:
            read_sintel_flow(str(q))
        assert str(e.value) == f"ReadFlowFile({q}): {msg}"

    bad("tag.flo", struct.pack("<f", 1.0) + raw[4:], "wrong tag (possibly due to big-endian machine?)")
    bad("w.flo", raw[:4] + struct.pack("<ii", 0, 5) + raw[12:], "illegal width 0")
    bad("w2.flo", raw[:4] + struct.pack("<ii", 100000, 5) + raw[12:], "illegal width 100000")
    bad("h.flo", raw[:4] + struct.pack("<ii", 7, -3) + raw[12:], "illegal height -3")
    bad("short.flo", raw[:-4], "file is too short")
    bad("long.flo", raw + b"\0", "file is too long")


def test_header_declares_metric_entries():
    protos = _lib.parse_header()
    want = {"vst_temporal_error": 15, "vst_ssim": 13, "vst_hist_u8": 7}
    for name, nargs in want.items():
        assert name in protos, name
        rt, args = protos[name]
        assert rt == "int" and args[-1] == "void*" and len(args) == nargs, (name, args)
    assert protos["vst_temporal_error_workspace"] == ("long", ["int", "int", "int"])
    assert protos["vst_ssim_workspace"] == ("long", ["int", "int", "int", "int"])


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built")
def test_metric_entries_validate_on_the_host():
    """Bad arguments are refused with VST_EINVAL before any launch (the pointers are never read)."""
    lib = _lib.lib.load()
    a, b, f, m, ws, acc, out = 4096, 8192, 12288, 16384, 20480, 24576, 28672

    def te(a=a, flo=f, B=1, C=3, H=8, W=8, power=2, hwc=0, clamp=0, scale=1.0, ws=ws, acc=acc):
        return lib.vst_temporal_error(a, b, flo, m, B, C, H, W, power, hwc, clamp, scale, ws, acc, None)

    for kw in (dict(a=None), dict(flo=None), dict(ws=None), dict(acc=None), dict(B=0), dict(C=0), dict(H=0),
               dict(W=-1), dict(power=0), dict(power=3), dict(hwc=2), dict(clamp=-1), dict(scale=float("nan")),
               dict(ws=ws + 4), dict(acc=acc + 4), dict(H=1 << 16, W=1 << 16)):
        assert te(**kw) == -1, kw
    assert lib.vst_temporal_error_workspace(8, 436, 1024) >= 8 * 2048
    assert lib.vst_temporal_error_workspace(0, 4, 4) == 0

    taps = (np.ones(11, dtype=np.float32) / 11).ctypes.data

    def ss(img1=a, taps=taps, win=11, B=1, C=3, H=16, W=16, out=out, ws=ws, tile=0):
        return lib.vst_ssim(img1, b, taps, win, B, C, H, W, out, None, ws, tile, None)

    for kw in (dict(img1=None), dict(taps=None), dict(out=None), dict(ws=None), dict(win=0), dict(win=4),
               dict(win=13), dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(tile=3), dict(tile=-1),
               dict(B=300, C=300), dict(ws=ws + 4)):
        assert ss(**kw) == -1, kw
    assert lib.vst_ssim_workspace(1, 3, 33, 65) == 8 * 3 * max(2 * 3, 3 * 2)

    def hi(img=a, hist=out, N=1, H=4, W=4, C=3):
        return lib.vst_hist_u8(img, hist, N, H, W, C, None)

    for kw in (dict(img=None), dict(hist=None), dict(N=0), dict(H=0), dict(W=0), dict(C=2), dict(C=4),
               dict(hist=out + 2), dict(N=70000)):
        assert hi(**kw) == -1, kw


def test_metrics_fail_loudly_without_hip_tensors():
    from vst.metrics import SSIMMetric, TemporalError, histogram_u8, ssim

    x = torch.zeros(1, 3, 12, 12)
    with pytest.raises(_lib.VstError):
        ssim(x, x)
    with pytest.raises(_lib.VstError):
        SSIMMetric()(x, x)
    with pytest.raises(_lib.VstError):
        TemporalError(2).update(x, x, torch.zeros(1, 2, 12, 12))
    with pytest.raises(_lib.VstError):
        histogram_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(_lib.VstError):
        SSIMMetric(window_size=13)
    m = SSIMMetric(window_size=11, channel=3, sigma=1.5)
    assert m.kernel.shape == (3, 1, 11, 11) and m.kernel.dtype == torch.float32
    assert torch.equal(m.kernel[0, 0], M.gauss_window(11, 1.5)[1]) and "kernel" in m.state_dict()
