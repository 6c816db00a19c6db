"""AdaAttN video inference on synthetic frames: frames/s of the cached-style path against the route
through the training forward, and the decoder's last layer alone on both of its kernels.

    python tools/aa_infer_bench.py [--policy bf16x6] [--frames 32] [--out profiles/aa_infer_bench.json]

Whole path at 256x512, batch_frames 1 and 4, seeded (torch.manual_seed) cosine model:
  A      model(vgg(c), fs) under no_grad + ops.tensor_to_frames   (fs = vgg(style) computed once)
  cache  the cached StyleState, last conv still GEMM + tensor_to_frames   (isolates the style cache)
  B      inference.stylize(..., frames=...): cached style + thin forward writing the frame
  each timed on device-resident chunks with HIP events (median of repeats after a warm-up), and
  `VideoInference` itself end to end (host staging, upload, download; host clock to the last frame).
Last layer alone at N x 64 x 256 x 512 (N = 1, 4) and 1 x 64 x 512 x 1024: ops.conv2d (no_grad) +
tensor_to_frames against ops.conv_thin_fwd(frames=...); the bytes are what the algorithm must move
(4 N H W Cin in, 3 N H W out), the peak the 6.29 TB/s measured copy rate.  One process; needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd"))
from vst import ops  # noqa: E402
from vst.adaattn import inference as I  # noqa: E402
from vst.adaattn.network import StylizingNetwork  # noqa: E402
from vst.adaattn.vgg19 import VGG19  # noqa: E402
from vst.synthetic import video_frames  # noqa: E402

COPY_PEAK = 6.29e12  # bytes/s, measured copy rate of the MI355X


def timed(fn, iters, repeats=7, warmup=3):
    """Median over `repeats` of the HIP-event time of `iters` calls, in ms per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def last_layer(res):
    g = torch.Generator().manual_seed(1)
    for N, H, W in ((1, 256, 512), (4, 256, 512), (1, 512, 1024)):
        Cin = 64
        x = torch.rand(N, Cin, H, W, generator=g).cuda()  # (a ReLU output)
        w = (torch.randn(3, Cin, 3, 3, generator=g) * 2.0).cuda()
        b = (torch.randn(3, generator=g) + 100.0).cuda()
        fr_old = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
        fr_new = torch.empty_like(fr_old)

        def old():
            with torch.no_grad(), ops.gemm_scope("stylizer"), ops.gemm_scope("dec"):
                y = ops.conv2d(x, w, b, pad=1, pad_mode="reflect")
                ops.tensor_to_frames(y, bgr=False, frames=fr_old)

        def new():
            ops.conv_thin_fwd(x, w, b, frames=fr_new)

        # each route: the median of 7 windows of 20 calls
        t_old, t_new = timed(old, 20), timed(new, 20)
        d = (fr_old.int() - fr_new.int()).abs()
        nbytes = 4.0 * N * H * W * Cin + 3.0 * N * H * W + 4.0 * w.numel()
        res[f"last_layer_{N}x{Cin}x{H}x{W}"] = {
            "gemm_plus_frames_us": 1e3 * t_old[0], "gemm_plus_frames_us_min_max": [1e3 * t_old[1], 1e3 * t_old[2]],
            "thin_fwd_frames_us": 1e3 * t_new[0], "thin_fwd_frames_us_min_max": [1e3 * t_new[1], 1e3 * t_new[2]],
            "speedup": t_old[0] / t_new[0], "algorithm_bytes": nbytes,
            "thin_fwd_fraction_of_copy_peak": nbytes / (t_new[0] * 1e-3) / COPY_PEAK,
            "frames_max_abs_diff": int(d.max()), "frames_differing_share": float((d > 0).float().mean())}
        print(f"last layer {N}x{Cin}x{H}x{W}: GEMM + frames {1e3 * t_old[0]:.1f} us, thin {1e3 * t_new[0]:.1f} us "
              f"({nbytes / (t_new[0] * 1e-3) / COPY_PEAK:.3f} of copy peak)", flush=True)


def whole_path(res, T):
    H, W = 256, 512
    torch.manual_seed(0)
    model = StylizingNetwork("cosine").cuda().eval()
    vgg = VGG19().cuda().eval()
    style = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8))
    s = ops.pil_resize_to_tensor255(style.cuda().unsqueeze(0), (W, H))
    clip = video_frames(3, T, H, W)
    with torch.no_grad():
        fs = vgg(s)
    state = I.encode_style(vgg, model, s)
    for B in (1, 4):
        c = ops.frames_to_tensor(torch.from_numpy(clip[:B].copy()).cuda())
        fr = {k: torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda") for k in "ACB"}

        def route_a():
            with torch.no_grad():
                ops.tensor_to_frames(model(vgg(c), fs), bgr=False, frames=fr["A"])

        def route_cache():
            I.THIN_FWD = False
            try:
                I.stylize(vgg, model, state, c, frames=fr["C"])
            finally:
                I.THIN_FWD = True

        def route_b():
            I.stylize(vgg, model, state, c, frames=fr["B"])

        t = {k: timed(f, 8) for k, f in (("A", route_a), ("cache", route_cache), ("B", route_b))}
        d = (fr["A"].int() - fr["B"].int()).abs()
        gain = t["A"][0] - t["B"][0]
        t0 = time.perf_counter()
        n = sum(1 for _ in I.VideoInference(model, s, clip, size=(H, W), batch_frames=B, vgg=vgg))
        torch.cuda.synchronize()
        e2e = n / (time.perf_counter() - t0)
        res[f"whole_path_256x512_batch{B}"] = {
            "A_frames_per_s": 1e3 * B / t["A"][0], "cache_only_frames_per_s": 1e3 * B / t["cache"][0],
            "B_frames_per_s": 1e3 * B / t["B"][0],
            "ms_per_chunk": {k: list(v) for k, v in t.items()},
            "gain_share_style_cache": (t["A"][0] - t["cache"][0]) / gain if gain > 0 else None,
            "gain_share_last_layer": (t["cache"][0] - t["B"][0]) / gain if gain > 0 else None,
            "video_inference_end_to_end_frames_per_s": e2e, "video_frames": n,
            "frames_A_vs_B_max_abs_diff": int(d.max()), "frames_A_vs_B_differing_share": float((d > 0).float().mean())}
        print(f"256x512 batch {B}: A {1e3 * B / t['A'][0]:.1f} frames/s, cache only {1e3 * B / t['cache'][0]:.1f}, "
              f"B {1e3 * B / t['B'][0]:.1f}; VideoInference end to end {e2e:.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="bf16x6")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join("profiles", "aa_infer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aa_infer_bench needs the GPU")
    ops.use_policy(a.policy)
    res = {"policy": a.policy, "device": torch.cuda.get_device_name(0)}
    last_layer(res)
    whole_path(res, a.frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
