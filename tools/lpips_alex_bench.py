"""The AlexNet LPIPS trunk's two kernels and the alex metric at 256 x 512 and 436 x 1024, B = 8 pairs.

    python tools/lpips_alex_bench.py [--out profiles/lpips_alex_bench.json] [--iters 50] [--rounds 5]

  stem     A: `vst_conv_cin3_k11s4` (+ bias + ReLU) over the [2B,3,H,W] trunk batch
           B: `torch.nn.functional.conv2d` (+ relu) on the same tensors on the same GPU -- the only other
              runnable form: the library had no stride-4 path before
           C: a device copy of the stem's input plus output bytes (the least any form must move)
           with the stem's achieved FLOP/s (2 x 363 per output) against the fp32 vector rate
  pool     A: `vst_maxpool3x3s2_fwd` on relu1's and relu2's shapes; C: a device copy of its input plus output bytes
  metric   uint8 frames in, distances out, in pairs/s under the f32 and bf16x6 policies, for net="alex" and
           -- re-measured in the same run -- net="vgg", each with its trunk's time and share
Timing as tools/eval_bench.py: HIP events around `iters` calls after a warm-up of every variant; the variants
alternate within one process for `rounds` rounds; the median per variant with its min / max.  A's and B's
outputs are compared on the timed inputs.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd"))
from eval_bench import COPY_PEAK, alternate  # noqa: E402
from vst import ops  # noqa: E402
from vst._lib import lib, ptr, stream  # noqa: E402
from vst.lpips import LPIPS  # noqa: E402
from vst.metrics import lpips_distance  # noqa: E402

VALU_F32_PEAK = 157.3e12  # FLOP/s: 256 CUs x 256 fp32 FLOP per clock (packed FMA) x 2.4 GHz


def _copy_of(nfloats):
    """A device copy that reads and writes `nfloats` floats in all (half in, half out)."""
    src = torch.empty(max(1, nfloats // 2), device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def _stats(t, nbytes=None):
    out = {}
    for k, (med, lo, hi) in t.items():
        out[k] = {"us_per_call": med, "min": lo, "max": hi}
        if nbytes is not None:
            out[k]["bytes_per_s"] = nbytes / (med * 1e-6)
            out[k]["copy_peak_fraction"] = out[k]["bytes_per_s"] / COPY_PEAK
    return out


def stem_bench(Hh, Ww, B, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(Hh)
    x = torch.rand(2 * B, 3, Hh, Ww, device="cuda", generator=g) * 4.9 - 2.2
    w = torch.randn(64, 3, 11, 11, device="cuda", generator=g) * (2.0 / 363) ** 0.5
    b = torch.randn(64, device="cuda", generator=g) * 0.1
    Ho, Wo = (Hh - 7) // 4 + 1, (Ww - 7) // 4 + 1
    out = torch.empty(2 * B, 64, Ho, Wo, device="cuda")
    nfloats = x.numel() + out.numel()

    def hip():
        lib.vst_conv_cin3_k11s4(ptr(x), ptr(w), ptr(b), ptr(out), 2 * B, Hh, Ww, 64, 1, stream())

    with torch.no_grad():
        t = alternate({"hip": hip, "torch_conv2d": lambda: F.relu(F.conv2d(x, w, b, stride=4, padding=2)),
                       "copy": _copy_of(nfloats)}, iters, rounds)
        hip()
        ref = F.relu(F.conv2d(x, w, b, stride=4, padding=2))
        diff = float((out - ref).abs().max() / ref.abs().max())
    flops = 2.0 * 363 * out.numel()
    res = {"shape": [2 * B, 3, Hh, Ww], "out": [2 * B, 64, Ho, Wo], "bytes": 4 * nfloats, "flops": flops,
           "hip_vs_torch_rel_diff": diff, **_stats(t, 4 * nfloats)}
    res["hip"]["flops_per_s"] = flops / (t["hip"][0] * 1e-6)
    res["hip"]["valu_f32_peak_fraction"] = res["hip"]["flops_per_s"] / VALU_F32_PEAK
    res["hip_over_torch"] = t["hip"][0] / t["torch_conv2d"][0]
    res["hip_over_copy"] = t["hip"][0] / t["copy"][0]
    return res


def pool_bench(NC, h, w, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(h)
    x = torch.relu(torch.randn(NC, h, w, device="cuda", generator=g))
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = torch.empty(NC, ho, wo, device="cuda")
    nfloats = x.numel() + out.numel()

    def hip():
        lib.vst_maxpool3x3s2_fwd(ptr(x), ptr(out), NC, h, w, stream())

    with torch.no_grad():
        t = alternate({"hip": hip, "torch_max_pool2d": lambda: F.max_pool2d(x, 3, 2), "copy": _copy_of(nfloats)}, iters, rounds)
        hip()
        same = bool(torch.equal(out, F.max_pool2d(x, 3, 2)))
    res = {"shape": [NC, h, w], "out": [NC, ho, wo], "bytes": 4 * nfloats, "bitwise_torch": same, **_stats(t, 4 * nfloats)}
    res["hip_over_copy"] = t["hip"][0] / t["copy"][0]
    res["hip_over_torch"] = t["hip"][0] / t["torch_max_pool2d"][0]
    return res


def metric_bench(Hh, Ww, B, iters, rounds):
    g = torch.Generator().manual_seed(Hh)
    img0 = torch.randint(0, 256, (B, Hh, Ww, 3), generator=g, dtype=torch.uint8).cuda()
    img1 = (img0.int() + torch.randint(-24, 25, (B, Hh, Ww, 3), generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    x = torch.rand(2 * B, 3, Hh, Ww, device="cuda") * 2 - 1
    out = {}
    old = ops.POLICY_NAME[0] or ops.DEFAULT_POLICY
    models = {net: LPIPS(net=net, pretrained=False, verbose=False).cuda() for net in ("alex", "vgg")}
    for policy in ("f32", "bf16x6"):
        ops.use_policy(policy)
        variants = {}
        for net, model in models.items():
            variants[net + "_metric"] = lambda m=model: lpips_distance(m, img0, img1)
            variants[net + "_trunk"] = lambda m=model: m.net(x)
        with torch.no_grad():
            t = alternate(variants, max(2, iters // 5), rounds)
        out[policy] = {}
        for net in models:
            m, tr = t[net + "_metric"], t[net + "_trunk"]
            out[policy][net] = {"us_per_call": m[0], "min": m[1], "max": m[2], "pairs_per_s": B / (m[0] * 1e-6),
                                "trunk_us": tr[0], "trunk_share": tr[0] / m[0]}
        out[policy]["alex_over_vgg_pairs_per_s"] = out[policy]["alex"]["pairs_per_s"] / out[policy]["vgg"]["pairs_per_s"]
    ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    return out


def size_bench(Hh, Ww, B, iters, rounds):
    Ho, Wo = (Hh - 7) // 4 + 1, (Ww - 7) // 4 + 1
    h2, w2 = (Ho - 3) // 2 + 1, (Wo - 3) // 2 + 1
    res = {"size": [Hh, Ww], "B": B, "stem": stem_bench(Hh, Ww, B, iters, rounds),
           "pool1": pool_bench(2 * B * 64, Ho, Wo, iters, rounds), "pool2": pool_bench(2 * B * 192, h2, w2, iters, rounds)}
    torch.cuda.empty_cache()
    res["metric"] = metric_bench(Hh, Ww, B, iters, rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lpips_alex_bench.json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_alex_bench needs the GPU")
    res = {"iters": args.iters, "rounds": args.rounds, "copy_peak_bytes_per_s": COPY_PEAK,
           "valu_f32_peak_flops_per_s": VALU_F32_PEAK,
           "sizes": [size_bench(hh, ww, 8, args.iters, args.rounds) for hh, ww in ((256, 512), (436, 1024))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
