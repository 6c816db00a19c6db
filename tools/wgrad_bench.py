import os
"""Microbenchmark of the split-K weight-gradient kernel (vst_conv_wgrad) on the step's layer
shapes, optionally across library builds.  Interleaved rounds, HIP-event timing.

    python tools/wgrad_bench.py [lib.so ...]
"""
import ctypes
import statistics
import sys

import torch

# GEMM arithmetic passed to every call (vst_hip.h VST_GEMM_*): 0 f32, 1 bf16x3, 2 bf16, 3 bf16x6, 4 f16;
# BENCH_MODES: several modes as columns (e.g. "3,35": bf16x6 halo / row-tiled via VST_GEMM_PERTAP = 32)
MODES = [int(m) for m in os.environ.get("BENCH_MODES", os.environ.get("BENCH_GEMM_MODE", "3")).split(",")]

sys.path.insert(0, "video-style-transfer_amd")
from vst._lib import LIB_PATH, _CTYPES, parse_header  # noqa: E402

# name, N, Cin, H, W, Cout, k, stride, gmode(0 reflect / 1 zero), pad, up
SHAPES = [
    ("res", 16, 192, 64, 128, 192, 3, 1, 0, 1, 1),
    ("deconv1", 16, 192, 64, 128, 96, 3, 1, 0, 1, 2),
    ("deconv2", 16, 96, 128, 256, 48, 3, 1, 0, 1, 2),
    ("conv2", 16, 48, 256, 512, 96, 3, 2, 0, 1, 1),
    ("conv3", 16, 96, 128, 256, 192, 3, 2, 0, 1, 1),
    ("conv1", 16, 3, 256, 512, 48, 9, 1, 0, 4, 1),
    # the nearest-x2 layers through the phase-stacked source-grid GEMM (vst_conv_wgrad_up2)
    ("deconv1_p", 16, 192, 64, 128, 96, 3, 1, 0, 1, 2),
    ("deconv2_p", 16, 96, 128, 256, 48, 3, 1, 0, 1, 2),
    # AdaAttN decoder at config 5 (B = 8 pairs -> 16 images, 512x1024 input; AA/network.py:63-99)
    ("aadec1", 16, 512, 64, 128, 512, 3, 1, 0, 1, 1),
    ("aadec3", 16, 256, 128, 256, 256, 3, 1, 0, 1, 1),
    ("aadec5", 16, 128, 256, 512, 128, 3, 1, 0, 1, 1),
    ("aadec7", 16, 64, 512, 1024, 64, 3, 1, 0, 1, 1),
    # the same 64-output decoder convs as row-split GEMMs (vst_conv_wgrad_rowsplit, ops.rowsplit_wgrad_ok)
    ("aadec6_rs", 16, 128, 256, 512, 64, 3, 1, 0, 1, 1),
    ("aadec6", 16, 128, 256, 512, 64, 3, 1, 0, 1, 1),
    ("aadec7_rs", 16, 64, 512, 1024, 64, 3, 1, 0, 1, 1),
]
ONLY = os.environ.get("BENCH_ONLY")


def load(path):
    lib = ctypes.CDLL(path)
    for name, (rt, argts) in parse_header().items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = _CTYPES[rt] if rt != "char*" else ctypes.c_char_p
            fn.argtypes = [_CTYPES[a] for a in argts]
    return lib


def main():
    global SHAPES
    if ONLY:
        SHAPES = [s for s in SHAPES if any(o in s[0] for o in ONLY.split(","))]
    paths = sys.argv[1:] or [LIB_PATH]
    libs = [load(p) for p in paths]
    st = torch.cuda.current_stream().cuda_stream
    cols = [(p, lib, m) for p, lib in zip(paths, libs) for m in MODES]
    res = {(p, m, s[0]): [] for p, _, m in cols for s in SHAPES}
    bufs = {}
    for s in SHAPES:
        name, N, Cin, H, W, Cout, k, stride, gm, pad, up = s
        Ho = (H * up + 2 * pad - k) // stride + 1
        Wo = (W * up + 2 * pad - k) // stride + 1
        x = torch.randn(N, Cin, H, W, device="cuda")
        dy = torch.randn(N, Cout, Ho, Wo, device="cuda")
        dw = torch.empty(Cout, Cin, k, k, device="cuda")
        if name.endswith("_p"):
            ws = torch.empty(libs[0].vst_conv_wgrad_up2_workspace(N, Cin, H, W, Cout), device="cuda")
        elif name.endswith("_rs"):
            ws = torch.empty(libs[0].vst_wgrad_workspace(N, Cout * k, k * Cin, (H + k - 1) * W), device="cuda")
        else:
            # (each build plans its own split: the largest workspace any of them asks for)
            ws = torch.empty(max(lb.vst_conv_wgrad_workspace(N, Cin, H, W, Cout, Ho, Wo, k, k, gm, stride, pad, up, m)
                                 for lb in libs for m in MODES), device="cuda")
        bufs[name] = (x, dy, dw, ws, Ho, Wo, 2.0 * N * Cout * Ho * Wo * Cin * k * k)
    for _ in range(5):
        for p, lib, MODE in cols:
            for s in SHAPES:
                name, N, Cin, H, W, Cout, k, stride, gm, pad, up = s
                x, dy, dw, ws, Ho, Wo, fl = bufs[name]
                args = (dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), N, Cin, H, W, Cout, Ho, Wo,
                        k, k, gm, stride, pad, up, 0, MODE, st)
                if name.endswith("_p"):
                    args = (dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, Cin, H, W, Cout, 0, MODE, st)
                    fn = lib.vst_conv_wgrad_up2
                elif name.endswith("_rs"):
                    args = (dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, Cin, H, W, Cout, k, 0, MODE, st)
                    fn = lib.vst_conv_wgrad_rowsplit
                else:
                    fn = lib.vst_conv_wgrad
                assert fn(*args) == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    fn(*args)
                e1.record()
                torch.cuda.synchronize()
                res[(p, MODE, name)].append(e0.elapsed_time(e1) / 5)
    for s in SHAPES:
        fl = bufs[s[0]][-1]
        line = f"{s[0]:10s}"
        for p, _, m in cols:
            ms = statistics.median(res[(p, m, s[0])])
            line += f"  {ms:7.3f} ms {fl / ms / 1e9:6.1f} TF"
        print(line)


if __name__ == "__main__":
    main()
