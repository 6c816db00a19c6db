"""RTNSTV video inference, CPU side: the restatement of the per-frame chain against the frames the
reference's own `Inference` made (tests/golden/rt_infer.npz, tests/golden/gen_golden_rt_infer.py), the
loud failure without a device, the drop-in's exports, and the argument checks of the new C entries.
The GPU tests are in tests/test_gpu_rtnstv_inference.py.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import rt_infer_ref as ref
from vst import _lib


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_reference_frames(golden, tag):
    """|diff| <= 1 and at most 1 % of the bytes (the generator asserted 0.25 % where it ran)."""
    g = golden("rt_infer")
    clip = ref.case_clip(tag, g[f"{tag}_meta"])
    frames = ref.stylise(ref.case_params(g, tag), clip)
    assert len(frames) == int(g[f"{tag}_n_out"])
    dmax, share = ref.case_bars(g, tag, frames, f"restatement {tag}")
    assert dmax <= 1 and share <= 0.01, (dmax, share)
    assert float(g[f"{tag}_oracle_share"]) <= 0.0025


def test_inference_fails_loudly_on_host():
    from vst.rtnstv.inference import Inference, cvframe_to_tensor, forward_frames
    from vst.rtnstv.network import StylizingNetwork

    frame = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(_lib.VstError):
        cvframe_to_tensor(frame, device="cpu")
    with pytest.raises(_lib.VstError):
        Inference(StylizingNetwork, StylizingNetwork().state_dict(), frame[None], device="cpu")
    with pytest.raises(_lib.VstError):
        forward_frames(StylizingNetwork(), torch.zeros((1, 8, 8, 3), dtype=torch.uint8))


def test_forward_ops_fail_loudly_on_host():
    from vst import ops

    x, w = torch.zeros(1, 3, 8, 8), torch.ones(3)
    with pytest.raises(_lib.VstError):
        ops.instance_norm_infer(x, w, w)
    with pytest.raises(_lib.VstError):
        ops.instance_norm_tanh_frames(x, w, w)
    with pytest.raises(_lib.VstError):
        ops.conv_stem_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros(4, 3, 3, 3))


def test_chunk_rule_depends_on_plane_only():
    """S comes from (C, HW) alone, stays within the library's limit, and is 1 for planes the
    register-resident one-read kernels of vst_instnorm_fwd take."""
    from vst import ops

    for C, HW in ((16, 230400), (32, 57600), (48, 14400), (3, 230400), (3, 36 * 52), (1, 1 << 24)):
        s = ops.instnorm_chunks(C, HW)
        assert 1 <= s <= ops.IN_MAX_CHUNKS
        assert s == 1 or HW // s >= 4
    assert ops.instnorm_chunks(48, 14400) == 1


def test_dropin_exports_inference():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd")
    spec = importlib.util.spec_from_file_location("rt_dropin_utilities", os.path.join(pkg, "rtnstv", "utilities.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
    from vst.rtnstv import inference, utilities

    assert mod.Inference is inference.Inference and mod.cvframe_to_tensor is inference.cvframe_to_tensor
    assert utilities.Inference is inference.Inference
    assert not hasattr(mod, "calculate_mse")  # nothing to be faithful to (vst.rtnstv.inference docstring)


def test_new_entries_in_header():
    protos = _lib.parse_header()
    want = {"vst_instnorm_moments": 6, "vst_instnorm_apply": 14, "vst_instnorm_tanh_frames": 11,
            "vst_conv_stem_u8": 10}
    for name, nargs in want.items():
        assert name in protos, name
        rt, args = protos[name]
        assert rt == "int" and args[-1] == "void*" and len(args) == nargs, (name, args)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built")
def test_new_entries_validate_arguments_without_gpu():
    """Every call below is refused with VST_EINVAL before any launch (the pointers are never read)."""
    lib = _lib.lib.load()
    x, p, w, b, y, st, fr = 4096, 8192, 12288, 16384, 20480, 24576, 28672

    def moments(x=x, p=p, planes=3, HW=64, S=2):
        return lib.vst_instnorm_moments(x, p, planes, HW, S, None)

    assert moments(x=None) == -1 and moments(p=None) == -1
    assert moments(planes=0) == -1 and moments(HW=0) == -1
    assert moments(S=0) == -1 and moments(S=257) == -1
    assert moments(p=p + 4) == -1  # doubles
    assert moments(planes=1 << 30, S=256) == -1  # the grid does not fit

    def apply(x=x, p=p, w=w, b=b, y=y, st=st, N=1, C=3, HW=64, S=2):
        return lib.vst_instnorm_apply(x, p, w, b, None, y, st, N, C, HW, S, 1e-5, 0, None)

    for k in ("x", "p", "w", "b", "y", "st"):
        assert apply(**{k: None}) == -1, k
    assert apply(N=0) == -1 and apply(C=0) == -1 and apply(HW=0) == -1
    assert apply(S=0) == -1 and apply(S=257) == -1

    def head(x=x, p=p, w=w, b=b, fr=fr, N=1, HW=64, S=2):
        return lib.vst_instnorm_tanh_frames(x, p, w, b, fr, N, HW, S, 1e-5, 1, None)

    for k in ("x", "p", "w", "b", "fr"):
        assert head(**{k: None}) == -1, k
    assert head(N=0) == -1 and head(HW=0) == -1 and head(S=0) == -1 and head(S=257) == -1

    def stem(fr=fr, w=w, out=y, N=1, H=8, W=8, Cout=16):
        return lib.vst_conv_stem_u8(fr, w, b, out, N, H, W, Cout, 1, None)

    assert stem(fr=None) == -1 and stem(w=None) == -1 and stem(out=None) == -1
    assert stem(N=0) == -1 and stem(N=65536) == -1
    assert stem(H=1) == -1 and stem(W=10) == -1 and stem(W=0) == -1
    for cout in (0, 3, 6, 20):
        assert stem(Cout=cout) == -1, cout
    assert stem(fr=fr + 2) == -1 and stem(out=y + 4) == -1  # dword frame loads, 16-byte stores
