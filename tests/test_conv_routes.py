"""Which kernel form every benchmark conv takes, decided by vst.ops' three pure route functions (no
tensors, no launches: only the built host library, for the exact-grid workspace query).  A slip in a
route predicate sends a layer to a slower but still correct kernel, which no numeric test sees: the
expected names below were taken from the chains the route functions replaced, layer by layer."""
import contextlib
import os

import pytest

from vst import _lib, ops

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built")

POLICIES = ("f32", "bf16x6", "parity", "f16")
VGG16 = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512))
VGG19 = ((64, 64), (128, 128), (256, 256, 256, 256), (512, 512, 512, 512), (512,))
# AA/vgg19.py:39-63: slice k ends at relu{k}_1, so these convs open a slice: their input is a loss feature
# (FeatureSplitFn masks it), not a ReLU output they alone consume
VGG19_HEADS = ("conv1_1", "conv1_2", "conv2_2", "conv3_2", "conv4_2")
# the AdaAttN decoder (vst/adaattn/network.py trunk): name, Cin, Cout, downscale of its plane, mask_dx
DECODER = (("conv1", 512, 512, 8, False), ("conv2", 512, 256, 8, True), ("conv3_0", 512, 256, 4, False),
           ("conv3_1", 256, 256, 4, True), ("conv3_2", 256, 256, 4, True), ("conv4", 256, 128, 4, True),
           ("conv5", 128, 128, 2, False), ("conv6", 128, 64, 2, True), ("conv7", 64, 64, 1, False),
           ("conv8", 64, 3, 1, True))


def _vgg(tag, scope, N, H, W, widths, heads=()):
    """(name, scope, N, Cin, Cout, ks, H, W, stride, pad, pad_mode, up, act, masked) per conv; masked: the
    conv follows another conv of its slice (run_vgg_slice's fuse_next)."""
    out, cin = [], 3
    for i, block in enumerate(widths):
        for j, cout in enumerate(block):
            name = f"conv{i + 1}_{j + 1}"
            sc = scope and f"{scope}.s{i + 1 if j == 0 else i + 2}"
            out.append((f"{tag}.{name}", sc, N, cin, cout, 3, H >> i, W >> i, 1, 1, "zero", 1, "relu",
                        j > 0 and name not in heads))
            cin = cout
    return out


def _layers():
    N, H, W = 16, 256, 512  # config 3: ReCoNet on 8 frame pairs of 256 x 512 under VGG16 (no scope)
    layers = [("rc.conv1", "stylizer", N, 3, 48, 9, H, W, 1, 4, "reflect", 1, None, False),
              ("rc.conv2", "stylizer", N, 48, 96, 3, H, W, 2, 1, "reflect", 1, None, False),
              ("rc.conv3", "stylizer", N, 96, 192, 3, H // 2, W // 2, 2, 1, "reflect", 1, None, False),
              ("rc.res", "stylizer.res", N, 192, 192, 3, H // 4, W // 4, 1, 1, "reflect", 1, None, False),
              ("rc.deconv1", "stylizer", N, 192, 96, 3, H // 4, W // 4, 1, 1, "reflect", 2, None, False),
              ("rc.deconv2", "stylizer", N, 96, 48, 3, H // 2, W // 2, 1, 1, "reflect", 2, None, False),
              ("rc.deconv3", "stylizer", N, 48, 3, 9, H, W, 1, 4, "reflect", 1, "tanh", False)]
    layers += _vgg("vgg16", None, N, H, W, VGG16)
    for cfg, B, H, W in (("aa4", 4, 256, 512), ("aa5", 4, 512, 1024)):  # configs 4 and 5
        layers += _vgg(cfg + ".enc", "encode", 3 * B, H, W, VGG19, VGG19_HEADS)
        layers += _vgg(cfg + ".loss", "lossnet", 2 * B, H, W, VGG19, VGG19_HEADS)
        layers += [(f"{cfg}.dec.{n}", "stylizer.dec", 2 * B, cin, cout, 3, H // ds, W // ds, 1, 1, "reflect", 1,
                    None if n == "conv8" else "relu", m) for n, cin, cout, ds, m in DECODER]
    return layers


LAYERS = {layer[0]: layer for layer in _layers()}

# "forward data-gradient weight-gradient" per layer: one string where the four policies agree, else one per
# policy.  Weight gradient: "gemm" = vst_conv_wgrad, "gemm+pertap" with the PERTAP flag, "gemm/thin" where
# its launch is recorded in the "thin" family.
_VGG = {"conv1_1": "cin3 tapsum gemm"}
_DEC = {"f32": "gemm padout gemm", "bf16x6": "gemm reflect3 gemm", "parity": "gemm reflect3 gemm",
        "f16": "gemm padout gemm"}
_DEC64 = {"f32": "gemm padout rowsplit", "bf16x6": "gemm reflect3 gemm", "parity": "gemm reflect3 rowsplit",
          "f16": "gemm padout gemm"}
EXPECTED = {
    "rc.conv1": "kwu padout gemm",
    "rc.conv2": "gemm phase2 gemm",
    "rc.conv3": {"f32": "gemm phase2 gemm", "bf16x6": "gemm phase2 gemm+pertap", "parity": "gemm phase2 gemm",
                 "f16": "gemm phase2 gemm"},
    "rc.res": {"f32": "gemm padout gemm", "bf16x6": "gemm reflect3 gemm+pertap", "parity": "gemm reflect3 gemm",
               "f16": "gemm padout gemm"},
    "rc.deconv1": "up2 ring up2",
    "rc.deconv2": "up2 ring up2",
    "rc.deconv3": "rowsplit padout_kwu rowsplit",
}
for _tag, _widths in (("vgg16", VGG16), ("aa4.enc", VGG19), ("aa4.loss", VGG19), ("aa5.enc", VGG19),
                      ("aa5.loss", VGG19)):
    for _i, _block in enumerate(_widths):
        for _j in range(len(_block)):
            _n = f"conv{_i + 1}_{_j + 1}"
            EXPECTED[f"{_tag}.{_n}"] = _VGG.get(_n, "gemm zero gemm")
for _cfg in ("aa4", "aa5"):
    for _n in ("conv1", "conv2", "conv3_0", "conv3_1", "conv3_2", "conv4", "conv5"):
        EXPECTED[f"{_cfg}.dec.{_n}"] = _DEC
    EXPECTED[f"{_cfg}.dec.conv6"] = _DEC64
    EXPECTED[f"{_cfg}.dec.conv7"] = _DEC64
    EXPECTED[f"{_cfg}.dec.conv8"] = "rowsplit thin gemm/thin"


@pytest.fixture
def policy(request):
    ops.gemm_role("fwd")  # (applies the environment's policy first, so it is the one restored)
    old = ops.POLICY_NAME[0]
    ops.use_policy(request.param)
    yield request.param
    ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)


def routes(layer):
    """The three routes of one layer as Conv2dFn takes them: the forward's mode looked up inside the
    layer's scope, the backward's outside it under policy_scope (Conv2dFn.backward)."""
    _, scope, N, Cin, Cout, ks, H, W, stride, pad, pad_mode, up, act, masked = layer
    fwd = ops.conv_fwd_route(Cin, Cout, H, W, ks, stride, pad, pad_mode, up, act)
    Ho, Wo = ops.conv_out_hw(H, W, ks, stride, pad, up)
    with ops.policy_scope(scope):
        dgrad, nws = ops.conv_dgrad_route(N, Cin, Cout, H, W, Ho, Wo, ks, (ks, ks), stride, pad, pad_mode, up, masked,
                                          ops.gemm_role("dgrad"))
        wgrad, flags, family = ops.conv_wgrad_route(Cin, Cout, W, ks, stride, pad, pad_mode, up, ops.gemm_role("wgrad"),
                                                    H=H)
    assert (nws >= 0) if dgrad == "reflect3" else nws == 0
    assert flags in (0, ops.PERTAP) and (wgrad == "gemm" or flags == 0)
    assert family is None if wgrad == "rowsplit" else family in ("wgrad", "thin")
    return f"{fwd} {dgrad} {wgrad}" + ("+pertap" if flags else "") + ("/thin" if family == "thin" else "")


@pytest.mark.parametrize("policy", POLICIES, indirect=True)
def test_benchmark_layers(policy):
    assert sorted(EXPECTED) == sorted(LAYERS)
    got = {name: routes(layer) for name, layer in LAYERS.items()}
    want = {name: e if isinstance(e, str) else e[policy] for name, e in EXPECTED.items()}
    assert got == want


def test_forward_mode_follows_scope_and_policy():
    """The mode handed to the forward's pack and launch: the role's under the layer's scope, the
    channel-blocked bit outside the stylizer, in its residual blocks and in the AdaAttN decoder."""
    ops.gemm_role("fwd")
    old = ops.POLICY_NAME[0]
    try:
        ops.use_policy("parity")
        got = {}
        for scope in (None, "stylizer", "stylizer.res", "stylizer.dec", "lossnet.s1"):
            with contextlib.ExitStack() as st:
                for part in (scope.split(".") if scope else ()):
                    st.enter_context(ops.gemm_scope(part))
                got[scope] = (ops.gemm_role("fwd"), ops.gemm_role("fwd_img"), ops.gemm_role("dgrad"))
        x3, x6, kb = ops.GEMM_MODES["bf16x3"], ops.GEMM_MODES["bf16x6"], ops.KBLOCK if ops.KBLOCK_ON else 0
        res = kb if ops.KBLOCK_RES else 0
        sty = kb if ops.KBLOCK_STYLIZER else 0
        assert got == {None: (x3 | kb,) * 3, "stylizer": (x6 | sty, x6 | sty, x3 | sty),
                       "stylizer.res": (x6 | res, x6 | res, x3 | res), "stylizer.dec": (x6 | res, x6 | res, x3 | res),
                       "lossnet.s1": (x3 | kb,) * 3}
        # a lookup, not a setter: another role's lookup in between changes nothing
        assert (ops.gemm_role("fwd"), ops.gemm_role("wgrad"), ops.gemm_role("fwd"))[::2] == (x3 | kb,) * 2
    finally:
        ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)


def test_routes_outside_the_benchmark_layers():
    """The route names no benchmark layer reaches, at the smallest geometry that does, and the two
    geometries without a route."""
    m = ops.GEMM_MODES["f32"]
    # a reflect conv that is neither stride-1 pad-in-plane, stride-2 nor odd-kernel "same": 1 x 1, no padding
    assert ops.conv_dgrad_route(1, 16, 16, 8, 16, 8, 16, 1, (1, 1), 1, 0, "reflect", 1, False, m) == ("fold", 0)
    # nearest-x2 upsampled 3 x 3 (UpsampleConvLayer) ...
    assert ops.conv_dgrad_route(1, 16, 16, 8, 16, 16, 32, 3, (3, 3), 1, 1, "reflect", 2, False, m) == ("ring", 0)
    # ... down to the plane where the ring would overlap itself (min(H, W) * up <= ks + 1)
    assert ops.conv_dgrad_route(1, 16, 16, 2, 16, 4, 32, 3, (3, 3), 1, 1, "reflect", 2, False, m) == ("fold", 0)
    assert ops.conv_dgrad_route(1, 3, 16, 8, 16, 8, 16, 3, (3, 3), 1, 1, "zero", 1, False, m) == ("tapsum", 0)
    assert ops.conv_dgrad_route(1, 3, 16, 8, 16, 8, 16, 3, (3, 3), 1, 1, "zero", 1, True, m) == ("zero", 0)
    with pytest.raises(ops.VstError, match="fused ReLU mask only on the zero-pad and stride-1 reflect-pad paths"):
        ops.conv_dgrad_route(1, 16, 16, 8, 16, 4, 8, 3, (3, 3), 2, 1, "reflect", 1, True, m)
    with pytest.raises(ops.VstError, match="zero padding with upsampling is not on the reference path"):
        ops.conv_dgrad_route(1, 16, 16, 8, 16, 16, 32, 3, (3, 3), 1, 1, "zero", 2, False, m)
    # a zero-pad thin-output conv: no row-split form, so VST_THIN_WGRAD=0 puts it on the row-tiled GEMM
    assert ops.conv_wgrad_route(64, 3, 64, 3, 1, 1, "zero", 1, m) == ("gemm", 0, "thin")
    # a one-row plane: the library's VALU kernels need two rows, and the routes follow its answer
    assert ops.conv_dgrad_route(1, 16, 3, 1, 16, 1, 16, 3, (3, 3), 1, 1, "zero", 1, False, m) == ("zero", 0)
    assert ops.conv_wgrad_route(16, 3, 16, 3, 1, 1, "zero", 1, m, H=1) == ("gemm", 0, "wgrad")
    assert ops.conv_dgrad_route(1, 16, 3, 2, 16, 2, 16, 3, (3, 3), 1, 1, "zero", 1, False, m) == ("thin", 0)
    assert ops.conv_wgrad_route(16, 3, 16, 3, 1, 1, "zero", 1, m, H=2) == ("gemm", 0, "thin")


# switch, its default, the layer it routes, the policy, which of the three routes, default-state and
# flipped-state answer
SWITCHES = [
    ("DGRAD_EXACT", True, "rc.res", "bf16x6", 1, "reflect3", "padout"),
    ("THIN_DGRAD", True, "aa4.dec.conv8", "f32", 1, "thin", "padout_kwu"),
    ("THIN_WGRAD", True, "aa4.dec.conv8", "f32", 2, "gemm/thin", "rowsplit"),
    ("RS_WGRAD", True, "aa4.dec.conv6", "f32", 2, "rowsplit", "gemm"),
    ("WGRAD_HALO_RES", False, "rc.res", "bf16x6", 2, "gemm+pertap", "gemm"),
    ("_WGRAD_UP2", True, "rc.deconv1", "f32", 2, "up2", "gemm"),
    ("UP2_FWD", True, "rc.deconv1", "f32", 0, "up2", "gemm"),
    ("CIN3_DIRECT", True, "vgg16.conv1_1", "f32", 0, "cin3", "kwu"),
]


@pytest.mark.parametrize("switch,default,layer,policy,which,at_default,flipped", SWITCHES, indirect=["policy"])
def test_ab_switches(monkeypatch, switch, default, layer, policy, which, at_default, flipped):
    monkeypatch.setattr(ops, switch, default)
    assert routes(LAYERS[layer]).split()[which] == at_default
    monkeypatch.setattr(ops, switch, not default)
    assert routes(LAYERS[layer]).split()[which] == flipped
    if switch == "THIN_WGRAD":
        assert ops.conv_wgrad_route(64, 3, 64, 3, 1, 1, "zero", 1, 0) == ("gemm", ops.PERTAP, "wgrad")


def test_every_route_name_is_exercised():
    seen = {r.replace("+pertap", "").replace("/thin", "") for e in EXPECTED.values()
            for r in ((e,) if isinstance(e, str) else e.values())}
    fwd, dgrad, wgrad = ({s.split()[i] for s in seen} for i in range(3))
    assert fwd == set(ops._FWD) == {"rowsplit", "cin3", "up2", "kwu", "gemm"}
    assert dgrad | {"fold"} == set(ops._DGRAD)  # ("fold": test_routes_outside_the_benchmark_layers)
    assert wgrad == {"up2", "rowsplit", "gemm"}
