"""Evaluation kernels at Sintel's own frame size (436 x 1024), B = 1 and B = 8, against what they replace.

    python tools/eval_bench.py [--out profiles/eval_bench.json] [--iters 50] [--rounds 5]

  temporal error   A: `vst_temporal_error` (TemporalError.update: warp, masked squared difference and
                      the fp64 sum in one pass, accumulated on the device)
                   B: the composition the project had before: `ops.warp`, then the masked squared
                      difference and a sum through torch on the same GPU
  SSIM             A: `vst_ssim` with the 32 x 32 tile, A2: with the 64 x 16 tile (score only, and with
                      the map written)
                   B: the reference's five `F.conv2d(groups=C)` calls and the map arithmetic through
                      torch on the same GPU (AA/eval.py:199-223)
  LPIPS (--lpips)  at 256 x 512 and 436 x 1024, B = 8 pairs, written to profiles/lpips_bench.json:
                   per trunk level, A: `vst_lpips_head` on the two halves of a [2B,C,h,w] feature batch,
                   B: the reference's op sequence (normalize_tensor twice, squared difference, 1x1
                   conv, spatial mean: AA/lpips/lpips.py:139-152) through torch on the same tensors;
                   the head's bytes/s against its one-read bound 2 B C P 4 bytes; the whole metric
                   (uint8 frames in, distances out) in pairs/s with its trunk / head split, under the
                   f32 and bf16x6 policies
Timing: HIP events around `iters` calls (a window of tens of milliseconds), after a warm-up of every
variant; the variants alternate A, B, A, B ... within one process for `rounds` rounds and the median
per variant is reported with its min / max.  Outputs of A and B are compared on the timed inputs.
Bytes are what the algorithm must move (temporal error: 2 C + 3 floats per pixel read, nothing
written; SSIM: 8 B per pixel, + 4 B with the map), over the 6.29 TB/s measured copy rate.  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd"))
from vst import ops  # noqa: E402
from vst._lib import lib, ptr, stream  # noqa: E402
from vst.lpips import LPIPS  # noqa: E402
from vst.metrics import SSIMMetric, TemporalError, lpips_distance  # noqa: E402

COPY_PEAK = 6.29e12  # bytes/s, measured copy rate of the MI355X
H, W, C = 436, 1024, 3


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def alternate(variants, iters, rounds):
    """{name: (median, min, max) us per call}: warm-up of every variant, then A, B, ... per round."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def temporal(B, iters, rounds):
    g = torch.Generator().manual_seed(B)
    a = (torch.rand(B, C, H, W, generator=g) * 255).cuda()
    b = (torch.rand(B, C, H, W, generator=g) * 255).cuda()
    flo = (torch.randn(B, 2, H, W, generator=g) * 3).cuda()
    flo_hwc = flo.permute(0, 2, 3, 1).contiguous()
    mask = (torch.rand(B, H, W, generator=g) > 0.3).float().cuda()
    te, te_hwc = TemporalError(2), TemporalError(2)
    acc = torch.zeros((), dtype=torch.float64, device="cuda")

    def composed():
        d = a - ops.warp(b, flo)
        acc.add_((mask.unsqueeze(1) * d * d).sum(dtype=torch.float64))

    with torch.no_grad():
        t = alternate({"fused": lambda: te.update(a, b, flo, mask),
                       "fused_flo_hwc": lambda: te_hwc.update(a, b, flo_hwc, mask, flow_hwc=True),
                       "composed": composed}, iters, rounds)
        one = TemporalError(2).update(a, b, flo, mask).state()[0].item() * (C * H * W)
        d = a - ops.warp(b, flo)
        ref = (mask.unsqueeze(1) * d * d).double().sum().item()
    nbytes = B * H * W * 4 * (2 * C + 3)
    out = {"B": B, "bytes": nbytes, "fused_vs_composed_rel_diff": abs(one - ref) / ref}
    for k, (med, lo, hi) in t.items():
        out[k] = {"us_per_call": med, "us_per_pair": med / B, "min": lo, "max": hi,
                  "hbm_fraction": nbytes / (med * 1e-6) / COPY_PEAK}
    out["fused_over_composed"] = t["fused"][0] / t["composed"][0]
    return out


def ssim_torch(x, y, kernel, win=11):
    conv = lambda t: F.conv2d(t, kernel, padding=win // 2, groups=x.shape[1])  # noqa: E731
    C1, C2 = 0.01**2, 0.03**2
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    smap = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return smap.mean(dim=[2, 3]).mean(dim=1)


def ssim(B, iters, rounds):
    g = torch.Generator().manual_seed(10 + B)
    x = torch.rand(B, C, H, W, generator=g).cuda()
    y = (x + 0.2 * torch.randn(B, C, H, W, generator=g).cuda()).clamp(0, 1)
    m = SSIMMetric(11, C, 1.5, reduction="none").cuda()
    with torch.no_grad():
        t = alternate({"tile_32x32": lambda: m(x, y, tile="32x32"),
                       "tile_64x16": lambda: m(x, y, tile="64x16"),
                       "tile_32x32_map": lambda: m(x, y, return_map=True, tile="32x32"),
                       "tile_64x16_map": lambda: m(x, y, return_map=True, tile="64x16"),
                       "torch_conv2d": lambda: ssim_torch(x, y, m.kernel)}, iters, rounds)
        diff = float((m(x, y) - ssim_torch(x, y, m.kernel)).abs().max())
    px = B * C * H * W
    out = {"B": B, "bytes": 8 * px, "bytes_with_map": 12 * px, "hip_vs_torch_abs_diff": diff}
    for k, (med, lo, hi) in t.items():
        nbytes = 12 * px if k.endswith("_map") else 8 * px
        out[k] = {"us_per_call": med, "min": lo, "max": hi, "hbm_fraction": nbytes / (med * 1e-6) / COPY_PEAK}
    out["best_tile_over_torch"] = min(t["tile_32x32"][0], t["tile_64x16"][0]) / t["torch_conv2d"][0]
    return out


LPIPS_CHNS = (64, 128, 256, 512, 512)


def lpips_torch(f0, f1, w):
    """AA/lpips/__init__.py:13-15 and AA/lpips/lpips.py:139-147 as the reference composes them."""
    n0 = f0 / (torch.sqrt(torch.sum(f0**2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1**2, dim=1, keepdim=True)) + 1e-10)
    return F.conv2d((n0 - n1) ** 2, w).mean([2, 3], keepdim=True)


def lpips_level(B, Cl, h, w, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(Cl + h)
    f = torch.relu(torch.randn(2 * B, Cl, h, w, device="cuda", generator=g))
    f[B:] = torch.relu(f[:B] + 0.3 * torch.randn(B, Cl, h, w, device="cuda", generator=g))
    wl = torch.rand(1, Cl, 1, 1, device="cuda", generator=g) * 0.05
    P = h * w
    layer, total = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ws = torch.empty(lib.vst_lpips_head_workspace(B, Cl, P) // 8, dtype=torch.float64, device="cuda")
    wflat = wl.reshape(-1)

    def fused():
        lib.vst_lpips_head(ptr(f), Cl * P, ptr(f) + 4 * B * Cl * P, Cl * P, ptr(wflat), B, Cl, P, ptr(layer), ptr(total), 0,
                           None, ws.data_ptr(), stream())

    f0, f1 = f[:B], f[B:]
    with torch.no_grad():
        t = alternate({"fused": fused, "composed": lambda: lpips_torch(f0, f1, wl)}, iters, rounds)
        fused()
        ref = lpips_torch(f0, f1, wl).reshape(-1)
        diff = float(((layer - ref).abs() / ref.abs()).max())
    nbytes = 2 * B * Cl * P * 4
    out = {"C": Cl, "h": h, "w": w, "P": P, "one_read_bytes": nbytes, "fused_vs_composed_rel_diff": diff}
    for k, (med, lo, hi) in t.items():
        out[k] = {"us_per_call": med, "min": lo, "max": hi}
    out["fused"]["bytes_per_s"] = nbytes / (t["fused"][0] * 1e-6)
    out["fused"]["hbm_fraction"] = out["fused"]["bytes_per_s"] / COPY_PEAK
    out["fused_over_composed"] = t["fused"][0] / t["composed"][0]
    return out


def lpips_bench(Hh, Ww, B, iters, rounds):
    levels, h, w = [], Hh, Ww
    for k, Cl in enumerate(LPIPS_CHNS):
        if k:
            h, w = h // 2, w // 2
        levels.append(lpips_level(B, Cl, h, w, iters, rounds))
        torch.cuda.empty_cache()
    out = {"size": [Hh, Ww], "B": B, "levels": levels,
           "heads_fused_us": sum(lv["fused"]["us_per_call"] for lv in levels),
           "heads_composed_us": sum(lv["composed"]["us_per_call"] for lv in levels), "metric": {}}
    g = torch.Generator().manual_seed(Hh)
    img0 = torch.randint(0, 256, (B, Hh, Ww, 3), generator=g, dtype=torch.uint8).cuda()
    img1 = (img0.int() + torch.randint(-24, 25, (B, Hh, Ww, 3), generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    model = LPIPS(net="vgg", pretrained=False, verbose=False).cuda()
    x = torch.rand(2 * B, 3, Hh, Ww, device="cuda") * 2 - 1
    old = ops.POLICY_NAME[0] or ops.DEFAULT_POLICY
    for policy in ("f32", "bf16x6"):
        ops.use_policy(policy)
        with torch.no_grad():
            t = alternate({"metric": lambda: lpips_distance(model, img0, img1), "trunk": lambda: model.net(x)},
                          max(2, iters // 5), rounds)
        m, tr = t["metric"][0], t["trunk"][0]
        out["metric"][policy] = {"us_per_call": m, "min": t["metric"][1], "max": t["metric"][2], "pairs_per_s": B / (m * 1e-6),
                                 "trunk_us": tr, "trunk_share": tr / m, "heads_fused_share": out["heads_fused_us"] / m}
    ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lpips", action="store_true", help="the LPIPS lines only (profiles/lpips_bench.json)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the GPU")
    if args.out is None:
        args.out = "profiles/lpips_bench.json" if args.lpips else "profiles/eval_bench.json"
    if args.lpips:
        res = {"iters": args.iters, "rounds": args.rounds, "copy_peak_bytes_per_s": COPY_PEAK,
               "lpips": [lpips_bench(hh, ww, 8, args.iters, args.rounds) for hh, ww in ((256, 512), (H, W))]}
    else:
        res = {"size": [H, W], "channels": C, "iters": args.iters, "rounds": args.rounds, "copy_peak_bytes_per_s": COPY_PEAK,
               "temporal_error": [temporal(B, args.iters, args.rounds) for B in (1, 8)],
               "ssim": [ssim(B, args.iters, args.rounds) for B in (1, 8)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
