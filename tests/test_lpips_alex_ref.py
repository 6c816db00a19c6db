"""LPIPS over the AlexNet trunk without a GPU: the restatement of tests/lpips_alex_ref.py against the
reference's own outputs (tests/golden/lpips_alex.npz), the module structure of `vst.lpips.LPIPS(net="alex")`,
and the host-side argument validation of the two entries of csrc/alex.hip."""
import os

import numpy as np
import pytest
import torch

import lpips_alex_ref as A
import lpips_ref as L
from vst import _lib

REL = 1e-5  # the bar tests/test_lpips_ref.py holds the VGG restatement to
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("lpips_alex")
    assert int(g["trunk_seed"]) == A.TRUNK_SEED
    return g, A.trunk_params(), [torch.from_numpy(g[f"lin{k}"]) for k in range(5)]


@pytest.mark.parametrize("key", list(A.PAIRS))
def test_restatement_reproduces_the_reference(fx, key):
    g, params, lins = fx
    img0, img1 = g[key + "_img0"], g[key + "_img1"]
    assert np.array_equal(img0, A.image_pair(key)[0]) and np.array_equal(img1, A.image_pair(key)[1])
    assert img0.shape == A.PAIRS[key][:3] + (3,)
    t0, t1 = L.im2tensor(img0), L.im2tensor(img1)
    assert tuple(tuple(f.shape[2:]) for f in A.trunk(params, t0)) == A.GRIDS[key]
    total, layers, maps = A.lpips64(params, lins, t0, t1)
    for name, got, want in (("layers", layers.numpy(), g[key + "_layers"]), ("total", total.numpy(), g[key + "_total"])):
        rel = np.abs(got - want) / np.abs(want)
        print(f"{key} {name}: worst {rel.max():.2e} rel")
        assert rel.max() <= REL, (key, name, got, want)
    assert (g[key + "_layers"] / g[key + "_total"][None]).min() >= 0.02  # every level counts in the fixture
    for name, got in (("norm01", A.lpips64(params, lins, 2 * L.unit01(img0) - 1, 2 * L.unit01(img1) - 1)[0]),
                      ("baseline", A.lpips64(params, None, t0, t1)[0]),
                      ("v00", A.lpips64(params, lins, t0, t1, scale=False)[0])):
        want = g[f"{key}_{name}"]
        assert np.abs(got.numpy() - want).max() <= REL * np.abs(want).max(), (key, name, got, want)
    assert float(A.lpips64(params, lins, t0, t0)[0].abs().max()) == 0.0
    if key == "a35":
        up = sum(torch.nn.functional.interpolate(m.unsqueeze(1), size=t0.shape[2:], mode="bilinear", align_corners=False)
                 for m in maps)
        want = g["a35_spatial"]
        assert up.shape == want.shape and np.abs(up.numpy() - want).max() <= REL * np.abs(want).max()


def test_float64_trunk_sits_beside_the_fp32_one(fx):
    """The float64 form of the restatement (the GPU tests' yardstick for single kernels) agrees with the fp32
    one on the fixture's pairs to fp32 rounding of a 5-layer trunk."""
    g, params, lins = fx
    t0, t1 = L.im2tensor(g["a64_img0"]), L.im2tensor(g["a64_img1"])
    t32, t64 = A.lpips64(params, lins, t0, t1)[0], A.lpips64(params, lins, t0, t1, dtype=torch.float64)[0]
    assert float((t32 - t64).abs().max()) <= 1e-4 * float(t64.abs().max())


def test_module_structure_matches_the_reference(fx):
    from oracle.seeding import seed_module
    from vst.lpips import LPIPS, alexnet

    g = fx[0]
    ref_keys = [str(k) for k in g["state_dict_keys"]]
    assert len(ref_keys) == 22
    assert ref_keys == (["scaling_layer.shift", "scaling_layer.scale"] + ["net." + n for n, _ in A.trunk_shapes()]
                        + [f"lin{k}.model.1.weight" for k in range(5)] + [f"lins.{k}.model.1.weight" for k in range(5)])
    model = LPIPS(net="alex", pretrained=False, verbose=False)
    sd = model.state_dict()
    assert list(sd) == ref_keys
    assert isinstance(model.net, alexnet) and model.chns == [64, 192, 384, 256, 256]
    for name, shape in A.trunk_shapes():
        assert tuple(sd["net." + name].shape) == tuple(shape)
    for k, c in enumerate(A.CHNS):
        assert tuple(sd[f"lin{k}.model.1.weight"].shape) == (1, c, 1, 1)
    assert not model.training and not any(p.requires_grad for p in model.net.parameters())
    lins = {f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1) for k in range(5)}
    missing, unexpected = model.load_state_dict(lins, strict=False)
    assert not unexpected
    for k in range(5):
        assert np.array_equal(model.state_dict()[f"lins.{k}.model.1.weight"].numpy().reshape(-1), g[f"lin{k}"])
    seed_module(model.net, A.TRUNK_SEED)
    for name, v in fx[1].items():
        assert torch.equal(model.state_dict()["net." + name], v)
    assert list(LPIPS(net="alex", pretrained=False, lpips=False, verbose=False).state_dict()) == ref_keys[:12]


def test_default_constructor_builds_the_alex_trunk():
    from vst.lpips import LPIPS, alexnet

    model = LPIPS(pretrained=False, verbose=False)  # the reference's default: net="alex"
    assert model.pnet_type == "alex" and isinstance(model.net, alexnet) and model.L == 5


def test_weights_paths_and_what_keeps_raising(fx, tmp_path):
    from vst.lpips import LPIPS, PerceptualLoss, default_model_path

    g = fx[0]
    assert default_model_path("0.1", "alex").endswith(os.path.join("adaattn", "lpips", "weights", "v0.1", "alex.pth"))
    assert default_model_path("0.0", "alex").endswith(os.path.join("weights", "v0.0", "alex.pth"))
    missing = str(tmp_path / "nowhere" / "alex.pth")
    with pytest.raises(_lib.VstError) as e:
        LPIPS(net="alex", model_path=missing, verbose=False)
    assert missing in str(e.value) and "lpips/weights/v0.1/alex.pth" in str(e.value)  # names the reference's file
    path = str(tmp_path / "alex.pth")
    torch.save({f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1) for k in range(5)}, path)
    model = LPIPS(model_path=path, verbose=False)
    assert np.array_equal(model.lin1.weight.detach().numpy().reshape(-1), g["lin1"])
    # a local torchvision-format trunk state dict, as vgg16 takes one
    tv = {f"features.{n.split('.')[1]}.{n.split('.')[2]}": v for n, v in fx[1].items()}
    wpath = str(tmp_path / "alexnet_tv.pth")
    torch.save(tv, wpath)
    loaded = LPIPS(pretrained=False, verbose=False, weights=wpath)
    for name, v in fx[1].items():
        assert torch.equal(loaded.state_dict()["net." + name], v)

    with pytest.raises(_lib.VstError, match="squeeze"):
        LPIPS(net="squeeze", pretrained=False, verbose=False)
    with pytest.raises(_lib.VstError):
        LPIPS(net="resnet", pretrained=False, verbose=False)
    with pytest.raises(_lib.VstError, match="pnet_tune"):
        LPIPS(net="alex", pnet_tune=True, pretrained=False, verbose=False)
    x = torch.zeros(1, 3, 32, 32)
    for call in (lambda: model.encode(x), lambda: model.encode_u8(torch.zeros(1, 32, 32, 3, dtype=torch.uint8)),
                 lambda: model.distance_to(None, x), lambda: PerceptualLoss(model)):
        with pytest.raises(_lib.VstError, match="forward only"):
            call()
    with pytest.raises(_lib.VstError):
        model(x, x)  # host tensors: there is no CPU path


def test_header_declares_the_alex_entries():
    protos = _lib.parse_header()
    assert protos["vst_conv_cin3_k11s4"] == ("int", ["float*"] * 4 + ["int"] * 5 + ["void*"])
    assert protos["vst_maxpool3x3s2_fwd"] == ("int", ["float*", "float*", "long", "int", "int", "void*"])


@built
def test_alex_host_side_validation_without_gpu():
    """Bad calls fail with VST_EINVAL before anything touches the device."""
    lib = _lib.lib.load()
    assert lib.vst_version() == 400

    def stem(x=4, w=4, b=None, out=4, N=1, H=31, W=31, Cout=64):
        return lib.vst_conv_cin3_k11s4(x, w, b, out, N, H, W, Cout, 1, None)

    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(H=6), dict(W=6), dict(Cout=20), dict(Cout=0),
                dict(Cout=80), dict(N=0), dict(N=65536), dict(x=2), dict(out=6)):
        assert stem(**bad) == -1, bad

    def pool(x=4, out=4, NC=1, H=3, W=3):
        return lib.vst_maxpool3x3s2_fwd(x, out, NC, H, W, None)

    for bad in (dict(x=None), dict(out=None), dict(H=2), dict(W=2), dict(NC=0)):
        assert pool(**bad) == -1, bad
