"""LPIPS without a GPU: the float64 restatement of tests/lpips_ref.py against the reference's own outputs
(tests/golden/lpips_vgg.npz), the C ABI's new entries (header, host-side validation), and the module
structure of vst.lpips."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as L
from vst import _lib

REL = 1e-5
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built (run __graft_entry__.build())")

# the reference's 38 state_dict keys (AA/lpips/lpips.py with net="vgg", use_dropout=True)
REF_KEYS = (["scaling_layer.shift", "scaling_layer.scale"]
            + ["net." + n for n, _ in L.trunk_shapes()]
            + [f"lin{k}.model.1.weight" for k in range(5)]
            + [f"lins.{k}.model.1.weight" for k in range(5)])


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("lpips_vgg")
    assert int(g["trunk_seed"]) == L.TRUNK_SEED
    return g, L.trunk_params(), [torch.from_numpy(g[f"lin{k}"]) for k in range(5)]


@pytest.mark.parametrize("key", list(L.PAIRS))
def test_float64_head_reproduces_the_reference(fx, key):
    g, params, lins = fx
    img0, img1 = g[key + "_img0"], g[key + "_img1"]
    assert np.array_equal(img0, L.image_pair(key)[0]) and np.array_equal(img1, L.image_pair(key)[1])
    t0, t1 = L.im2tensor(img0), L.im2tensor(img1)
    total, layers, maps = L.lpips64(params, lins, t0, t1)
    for name, got, want in (("layers", layers.numpy(), g[key + "_layers"]), ("total", total.numpy(), g[key + "_total"])):
        rel = np.abs(got - want) / np.abs(want)
        print(f"{key} {name}: worst {rel.max():.2e} rel")
        assert rel.max() <= REL, (key, name, got, want)
    assert (g[key + "_layers"] / g[key + "_total"][None]).min() >= 0.005  # every level counts in the fixture
    for name, got in (("norm01", L.lpips64(params, lins, 2 * L.unit01(img0) - 1, 2 * L.unit01(img1) - 1)[0]),
                      ("baseline", L.lpips64(params, None, t0, t1)[0]),
                      ("v00", L.lpips64(params, lins, t0, t1, scale=False)[0])):
        want = g[f"{key}_{name}"]
        assert np.abs(got.numpy() - want).max() <= REL * np.abs(want).max(), (key, name, got, want)
    assert float(L.lpips64(params, lins, t0, t0)[0].abs().max()) == 0.0
    if key == "p32":
        up = sum(torch.nn.functional.interpolate(m.unsqueeze(1), size=t0.shape[2:], mode="bilinear", align_corners=False)
                 for m in maps)
        want = g["p32_spatial"]
        assert up.shape == want.shape and np.abs(up.numpy() - want).max() <= REL * np.abs(want).max()
    if key == "p36":
        assert abs(float(total[0]) - float(g["p36_lpips_loss"])) <= REL * float(g["p36_lpips_loss"])


def test_input_table_restated(fx):
    g = fx[0]
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    assert np.array_equal(L.scaling(L.im2tensor(ramp))[0, :, :, 0].numpy().T, g["input_table"])


def test_fp32_form_against_float64_on_the_head_inputs():
    """The reference's fp32 sequence sits near float64 on the GPU test's inputs (so its distance is a
    meaningful bar there), NaN-free with all-zero pixels."""
    for shape in L.HEAD_SHAPES:
        f0, f1, w = L.head_inputs(shape)
        l64, m64 = L.head64(f0, f1, w)
        l32, m32 = L.head32(f0, f1, w)
        assert torch.isfinite(m32).all() and torch.isfinite(m64).all()
        assert float((l32.double() - l64).abs().max()) <= 1e-5 * float(l64.abs().max())
        if shape[2] * shape[3] > 2:
            assert float(m64.reshape(shape[0], -1)[:, 1].abs().max()) == 0.0  # all-zero in both


def test_header_declares_lpips_entries():
    protos = _lib.parse_header()
    for name in ("vst_lpips_head", "vst_lpips_head_workspace", "vst_lpips_input"):
        assert name in protos, name
    for name in ("vst_lpips_head", "vst_lpips_input"):
        assert protos[name][0] == "int" and protos[name][1][-1] == "void*", name
    assert protos["vst_lpips_head_workspace"] == ("long", ["int", "int", "long"])


@built
def test_lpips_host_side_validation_without_gpu():
    lib = _lib.lib.load()
    assert lib.vst_version() == 400

    def head(f0=1, f1=1, N=1, C=64, P=63, ws=8):
        return lib.vst_lpips_head(f0, C * P, f1, C * P, None, N, C, P, 1, 1, 0, None, ws, None)

    for bad in (dict(C=24), dict(C=1024), dict(N=0), dict(f0=None), dict(f1=None), dict(P=0), dict(ws=None), dict(ws=4)):
        assert head(**bad) == -1, bad
    assert lib.vst_lpips_head(1, 10, 1, 64 * 63, None, 1, 64, 63, 1, 1, 0, None, 8, None) == -1  # stride below C P
    assert lib.vst_lpips_head(1, 64 * 63, 1, 64 * 63, None, 1, 64, 63, 1, None, 1, None, 8, None) == -1  # accumulate, no total
    sizes = [lib.vst_lpips_head_workspace(n, 64, p) for n, p in ((1, 63), (1, 5000), (2, 5000), (2, 100000))]
    assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes
    assert lib.vst_lpips_head_workspace(1, 24, 63) == 0
    assert lib.vst_lpips_input(None, 1, 1, 0, 1, 16, 16, 0, 0, 1, None) == -1
    assert lib.vst_lpips_input(1, 1, 1, -1, 1, 16, 16, 0, 0, 1, None) == -1
    assert lib.vst_lpips_input(1, 2, 1, 0, 1, 16, 16, 0, 0, 1, None) == -1


def test_module_structure_matches_the_reference(fx):
    from vst.lpips import LPIPS

    g = fx[0]
    model = LPIPS(net="vgg", pretrained=False, verbose=False)
    sd = model.state_dict()
    assert list(sd) == REF_KEYS and len(sd) == 38
    for (name, shape) in L.trunk_shapes():
        assert tuple(sd["net." + name].shape) == tuple(shape)
    assert not model.training and not any(p.requires_grad for p in model.net.parameters())
    # the reference's weights file is a dict of lin{k}.model.1.weight: strict=False loads it
    lins = {f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1) for k in range(5)}
    missing, unexpected = model.load_state_dict(lins, strict=False)
    assert not unexpected
    for k in range(5):
        assert np.array_equal(model.state_dict()[f"lins.{k}.model.1.weight"].numpy().reshape(-1), g[f"lin{k}"])
    # seed_module behaves as on the reference: the trunk's arrays are those of lpips_ref.trunk_params
    from oracle.seeding import seed_module

    seed_module(model.net, L.TRUNK_SEED)
    for name, v in fx[1].items():
        assert torch.equal(model.state_dict()["net." + name], v)
    assert list(LPIPS(net="vgg16", pretrained=False, lpips=False, verbose=False).state_dict()) == REF_KEYS[:28]


def test_unsupported_configurations_raise(tmp_path):
    from vst.lpips import LPIPS, default_model_path

    for net in ("alex", "squeeze"):
        with pytest.raises(_lib.VstError, match="11x11"):
            LPIPS(net=net, verbose=False)
    with pytest.raises(_lib.VstError):
        LPIPS(verbose=False)  # the reference's default trunk is AlexNet
    with pytest.raises(_lib.VstError, match="pnet_tune"):
        LPIPS(net="vgg", pnet_tune=True, pretrained=False, verbose=False)
    missing = str(tmp_path / "nowhere" / "vgg.pth")
    with pytest.raises(_lib.VstError) as e:
        LPIPS(net="vgg", model_path=missing, verbose=False)
    assert missing in str(e.value)
    assert default_model_path().endswith(os.path.join("adaattn", "lpips", "weights", "v0.1", "vgg.pth"))
    if not os.path.exists(default_model_path()):
        with pytest.raises(_lib.VstError) as e:
            LPIPS(net="vgg", verbose=False)
        assert default_model_path() in str(e.value)
    model = LPIPS(net="vgg", pretrained=False, verbose=False)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(_lib.VstError):
        model(x, x)  # host tensors: there is no CPU path


def test_weights_file_loads_from_model_path(fx, tmp_path):
    from vst.lpips import LPIPS

    g = fx[0]
    path = str(tmp_path / "vgg.pth")
    torch.save({f"lin{k}.model.1.weight": torch.from_numpy(g[f"lin{k}"]).view(1, -1, 1, 1) for k in range(5)}, path)
    model = LPIPS(net="vgg", model_path=path, verbose=False)
    assert np.array_equal(model.lin3.weight.detach().numpy().reshape(-1), g["lin3"])
