#!/usr/bin/env python3
"""The SSIM gradient on the MI355X (`vst_ssim_bwd`), at 256 x 512 and 436 x 1024 with B = 8, C = 3 and
the 11-tap window, written to profiles/ssim_grad_bench.json.  Per size:

  bwd_d1      `vst_ssim_bwd` with d2 = NULL (what SSIMLoss launches);
  bwd_d1_d2   `vst_ssim_bwd` with both gradients;
  forward     `vst_ssim` (scores only, the default tile);
  torch_bwd   the torch-autograd backward of the five-conv2d formulation (tests/ssim_grad_ref.py
              `ssim_map_c`) with respect to img1 on the same tensors -- the backward alone, its graph
              built once and kept;
  copy        a device copy of 1.5 planes' worth of bytes read and written once: the three planes of
              traffic (x and y read, d1 written) that bwd_d1 cannot go below.

Timing as tools/lpips_grad_bench.py: HIP events around `iters` calls after a warm-up of every variant,
the variants alternating within one process for `rounds` rounds, the median per variant reported with
its min / max.  The fused gradient is compared with torch's on the timed inputs.  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "video-style-transfer_amd")):
    sys.path.insert(0, p)
import metrics_ref  # noqa: E402
import ssim_grad_ref  # noqa: E402
from vst._lib import lib, ptr, stream  # noqa: E402

WIN = 11


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def alternate(variants, iters, rounds):
    """{name: {us_per_call (median), min, max}}: warm-up of every variant, then A, B, ... per round."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return {k: {"us_per_call": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def bench(H, W, B, C, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(H + W)
    x = torch.rand(B, C, H, W, device="cuda", generator=g)
    y = (x + 0.2 * torch.randn(B, C, H, W, device="cuda", generator=g)).clamp(0, 1)
    gout = torch.randn(B, device="cuda", generator=g)
    taps = np.ascontiguousarray(metrics_ref.gauss_window(WIN, 1.5)[0].numpy(), dtype=np.float32)
    c1, c2 = ssim_grad_ref.constants(1.0)
    d1, d2 = torch.empty_like(x), torch.empty_like(x)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(1, lib.vst_ssim_workspace(B, C, H, W) // 8), dtype=torch.float64, device="cuda")

    def bwd(second):
        lib.vst_ssim_bwd(ptr(x), ptr(y), taps.ctypes.data, WIN, B, C, H, W, c1, c2, ptr(gout), ptr(d1),
                         ptr(d2) if second else None, stream())

    def forward():
        lib.vst_ssim(ptr(x), ptr(y), taps.ctypes.data, WIN, B, C, H, W, ptr(out), None, ws.data_ptr(), 0, stream())

    a = x.clone().requires_grad_(True)
    scores = ssim_grad_ref.ssim_map_c(a, y, WIN, 1.5, c1, c2).mean(dim=[2, 3]).mean(dim=1)

    def torch_bwd():
        return torch.autograd.grad(scores, a, gout, retain_graph=True)[0]

    S = 4 * B * C * H * W  # bytes of one (B,C,H,W) tensor
    src = torch.empty(3 * S // 8, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = alternate({"bwd_d1": lambda: bwd(False), "bwd_d1_d2": lambda: bwd(True), "forward": forward,
                   "torch_bwd": torch_bwd, "copy": lambda: dst.copy_(src)}, iters, rounds)
    bwd(True)
    ref = torch_bwd()
    res = {"size": [H, W], "B": B, "C": C, "window": WIN, "bytes_moved_d1": 3 * S,
           "fused_vs_torch_rel_diff": float((d1 - ref).abs().max() / ref.abs().max()), **t}
    res["bwd_d1"]["bytes_per_s"] = 3 * S / (t["bwd_d1"]["us_per_call"] * 1e-6)
    res["bwd_d1_d2"]["bytes_per_s"] = 4 * S / (t["bwd_d1_d2"]["us_per_call"] * 1e-6)
    res["copy"]["bytes_per_s"] = 3 * S / (t["copy"]["us_per_call"] * 1e-6)
    res["torch_bwd_over_bwd_d1"] = t["torch_bwd"]["us_per_call"] / t["bwd_d1"]["us_per_call"]
    res["bwd_d1_over_copy"] = t["bwd_d1"]["us_per_call"] / t["copy"]["us_per_call"]
    res["bwd_d1_over_forward"] = t["bwd_d1"]["us_per_call"] / t["forward"]["us_per_call"]
    res["bwd_d1_d2_over_bwd_d1"] = t["bwd_d1_d2"]["us_per_call"] / t["bwd_d1"]["us_per_call"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ssim_grad_bench.json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_grad_bench needs the GPU")
    res = {"iters": args.iters, "rounds": args.rounds,
           "ssim_grad": [bench(h, w, 8, 3, args.iters, args.rounds) for h, w in ((256, 512), (436, 1024))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
