#!/usr/bin/env python3
"""The LPIPS gradient on the MI355X (`vst_lpips_head_bwd`, `LPIPS.distance_to`), at 256 x 512 and
436 x 1024 with B = 8 under the bf16x6 policy, written to profiles/lpips_grad_bench.json:

  per trunk level  A: `vst_lpips_head_bwd` with d1 = NULL on [B,C,h,w] features (what `distance_to` launches);
                   B: the torch-autograd backward of the reference's op sequence (tests/lpips_ref.py
                      `head32`) on the same tensors -- the backward alone, its graph built once and kept;
                   C: a device copy that moves the same bytes (the backward reads f0 and f1 and writes
                      d0: 3 S bytes for S = 4 B C P; the copy is of 1.5 S bytes, read and written once);
  whole metric     `distance_to` forward + backward (the gradient with respect to in0, N images through
                   the trunk) against `distance_to` forward alone and `forward` alone (2N images).

Timing as tools/eval_bench.py: HIP events around `iters` calls after a warm-up of every variant, the
variants alternating within one process for `rounds` rounds, the median per variant reported with its
min / max.  A's output is compared with B's on the timed inputs.  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "video-style-transfer_amd")):
    sys.path.insert(0, p)
import lpips_ref  # noqa: E402
from vst import ops  # noqa: E402
from vst._lib import lib, ptr, stream  # noqa: E402
from vst.lpips import LPIPS  # noqa: E402

CHNS = (64, 128, 256, 512, 512)


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


def level(B, C, h, w, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(C + h)
    f0 = torch.relu(torch.randn(B, C, h, w, device="cuda", generator=g))
    f1 = torch.relu(f0 + 0.3 * torch.randn(B, C, h, w, device="cuda", generator=g))
    wl = torch.rand(C, device="cuda", generator=g) * 0.05
    gl = torch.randn(B, device="cuda", generator=g)
    P = h * w
    d0 = torch.empty_like(f0)

    def fused():
        lib.vst_lpips_head_bwd(ptr(f0), C * P, ptr(f1), C * P, ptr(wl), ptr(gl), B, C, P, ptr(d0), C * P, None, 0, stream())

    a = f0.clone().requires_grad_(True)
    layer, _ = lpips_ref.head32(a, f1, wl)

    def composed():
        return torch.autograd.grad(layer, a, gl, retain_graph=True)[0]

    S = 4 * B * C * P
    src = torch.empty(3 * S // 8, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = alternate({"fused": fused, "composed": composed, "copy": lambda: dst.copy_(src)}, iters, rounds)
    fused()
    ref = composed()
    diff = float((d0 - ref).abs().max() / ref.abs().max())
    out = {"C": C, "h": h, "w": w, "P": P, "bytes_moved": 3 * S, "fused_vs_composed_rel_diff": diff, **t}
    out["fused"]["bytes_per_s"] = 3 * S / (t["fused"]["us_per_call"] * 1e-6)
    out["copy"]["bytes_per_s"] = 3 * S / (t["copy"]["us_per_call"] * 1e-6)
    out["fused_over_composed"] = t["fused"]["us_per_call"] / t["composed"]["us_per_call"]
    out["fused_over_copy"] = t["fused"]["us_per_call"] / t["copy"]["us_per_call"]
    return out


def bench(H, W, B, iters, rounds):
    levels, h, w = [], H, W
    for k, C in enumerate(CHNS):
        if k:
            h, w = h // 2, w // 2
        levels.append(level(B, C, h, w, iters, rounds))
        torch.cuda.empty_cache()
    out = {"size": [H, W], "B": B, "levels": levels}
    for name in ("fused", "composed", "copy"):
        out[f"heads_bwd_{name}_us"] = sum(lv[name]["us_per_call"] for lv in levels)
    model = LPIPS(net="vgg", pretrained=False, verbose=False).cuda()
    in0 = (torch.rand(B, 3, H, W, device="cuda") * 2 - 1).requires_grad_(True)
    in1 = (in0.detach() + 0.1 * torch.randn(B, 3, H, W, device="cuda")).clamp(-1, 1)
    plain = in0.detach()
    seed = torch.ones(B, 1, 1, 1, device="cuda")
    old = ops.POLICY_NAME[0] or ops.DEFAULT_POLICY
    ops.use_policy("bf16x6")
    target = model.encode(in1)

    def fwd_bwd():
        return torch.autograd.grad(model.distance_to(target, in0), in0, seed)[0]

    def forward():
        with torch.no_grad():
            return model(plain, in1)

    t = alternate({"distance_to_fwd_bwd": fwd_bwd, "distance_to_fwd": lambda: model.distance_to(target, plain),
                   "forward": forward}, max(2, iters // 5), rounds)
    ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    t["fwd_bwd_over_forward"] = t["distance_to_fwd_bwd"]["us_per_call"] / t["forward"]["us_per_call"]
    t["fwd_bwd_over_distance_to_fwd"] = t["distance_to_fwd_bwd"]["us_per_call"] / t["distance_to_fwd"]["us_per_call"]
    t["heads_bwd_share_of_fwd_bwd"] = out["heads_bwd_fused_us"] / t["distance_to_fwd_bwd"]["us_per_call"]
    out["metric_bf16x6"] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lpips_grad_bench.json")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_grad_bench needs the GPU")
    res = {"iters": args.iters, "rounds": args.rounds,
           "lpips_grad": [bench(h, w, 8, args.iters, args.rounds) for h, w in ((256, 512), (436, 1024))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
