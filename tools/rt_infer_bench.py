"""RTNSTV video inference on synthetic frames: the split-plane InstanceNorm against the one-workgroup-
per-plane kernel, the uint8 stem and the fused tail against the chains they replace, and frames/s of
`vst.rtnstv.inference.Inference` against the only path there was before it.

    python tools/rt_infer_bench.py [--frames 64] [--out profiles/rt_infer_bench.json]

Every time is a HIP-event time of `iters` back-to-back calls divided by `iters`, after a warm-up; the
figure is the median of `repeats` such windows, with their min and max as the spread.  Candidates of one
table are measured in the same process, interleaved window by window.  The operands of parts 1 and 2
stay resident between calls (L2 / MALL-warm), as they are in the network, where the conv before a norm
has just written them.  One process; needs the GPU.

  1. norm     vst_instnorm_fwd (S = 1) against vst_instnorm_moments + vst_instnorm_apply over a sweep of
              S, with ReLU, for the RTNSTV geometries (N*C, HW) at 360x640: (16, 230400), (32, 57600),
              (48, 14400), (3, 230400), and the same at B = 8; once through the Python ops (`op`: allocation
              and wrapper included, what a caller pays) and once through the C entries on preallocated
              buffers (`c_entries`: close to the kernels' own time).  `rule` is what ops.instnorm_chunks picks.
     rules    `forward_frames` per frame under candidate rules for S inside the network: the extra launch
              of the split costs host time, which is what bounds the network at one frame per forward.
  2. stem     frames_to_tensor + conv2d (3 -> 16, no_grad) against conv_stem_u8;
     tail     instance_norm + tanh_image + tensor_to_frames against instance_norm_tanh_frames;
              both at B = 1 and 8.
  3. frames/s `Inference` at batch_frames 1 and 8 on in-memory 360x640 frames against
              frames_to_tensor -> StylizingNetwork.forward (no_grad) -> tensor_to_frames driven by the same
              loop (same pinned upload, same pinned download, host clock to the last frame), and both
              forwards alone on device-resident chunks (HIP events).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd"))
from vst import _lib, ops  # noqa: E402
from vst.rtnstv import inference as I  # noqa: E402
from vst.rtnstv.network import StylizingNetwork  # noqa: E402
from vst.synthetic import video_frames  # noqa: E402
from vst.video_io import PinnedUploader  # noqa: E402

H, W = 360, 640
L = _lib.lib


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per call


def interleaved(fns, iters, repeats=9, warmup=10):
    """{name: (median, min, max)} in us per call; one window of each candidate per round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(r):
    return {"us": round(r[0], 2), "min": round(r[1], 2), "max": round(r[2], 2)}


def norm_ab(res, iters):
    g = torch.Generator().manual_seed(1)
    rows = []
    for B in (1, 8):
        for C, hw in ((16, (360, 640)), (32, (180, 320)), (48, (90, 160)), (3, (360, 640))):
            HW = hw[0] * hw[1]
            x = torch.randn(B, C, *hw, generator=g).cuda()
            w = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
            b = (0.1 * torch.randn(C, generator=g)).cuda()
            sweep = [s for s in (1, 2, 4, 8, 16, 32, 64, 128) if s == 1 or HW // s >= 1024]
            fns = {s: (lambda s=s: ops.instance_norm_infer(x, w, b, relu=True, chunks=s)) for s in sweep}
            t = interleaved(fns, iters)
            # the C entries alone on preallocated buffers: no allocation, no Python wrapper per launch
            y, stats = torch.empty_like(x), torch.empty(B * C * 2, device="cuda")
            part = torch.empty(B * C * max(sweep) * 2, dtype=torch.float64, device="cuda")
            st = _lib.stream()
            px, pw, pb, py, ps, pp = (v.data_ptr() for v in (x, w, b, y, stats, part))

            def c_call(s):
                if s == 1:
                    return lambda: L.vst_instnorm_fwd(px, pw, pb, None, py, ps, B, C, HW, 1e-5, 1, st)

                def two():
                    L.vst_instnorm_moments(px, pp, B * C, HW, s, st)
                    L.vst_instnorm_apply(px, pp, pw, pb, None, py, ps, B, C, HW, s, 1e-5, 1, st)
                return two

            tc = interleaved({s: c_call(s) for s in sweep}, iters)
            best = min(t, key=lambda s: t[s][0])
            row = {"planes": B * C, "C": C, "HW": HW, "B": B, "rule": ops.instnorm_chunks(C, HW), "best_op": best,
                   "best_c": min(tc, key=lambda s: tc[s][0]),
                   "op": {str(s): fmt(r) for s, r in t.items()}, "c_entries": {str(s): fmt(r) for s, r in tc.items()}}
            rows.append(row)
            print(f"norm ({B * C:3d}, {HW:6d}) op: " + "  ".join(f"S={s}: {r[0]:.1f}" for s, r in t.items()) +
                  f"  | rule {row['rule']} best {best}", flush=True)
            print(f"norm ({B * C:3d}, {HW:6d}) C : " + "  ".join(f"S={s}: {r[0]:.1f}" for s, r in tc.items()) +
                  f"  | best {row['best_c']}", flush=True)
    res["norm"] = rows


def stem_tail(res, iters):
    g = torch.Generator().manual_seed(2)
    rows = []
    for B in (1, 8):
        frames = torch.from_numpy(video_frames(3, B, H, W)).cuda()
        w = (torch.randn(16, 3, 3, 3, generator=g) * (2 / 27) ** 0.5).cuda()
        b = (0.1 * torch.randn(16, generator=g)).cuda()

        def old_stem():
            with torch.no_grad():
                return ops.conv2d(ops.frames_to_tensor(frames), w, b, stride=1, pad=1, pad_mode="reflect")

        t = interleaved({"old": old_stem, "new": lambda: ops.conv_stem_u8(frames, w, b)}, iters)
        rows.append({"what": "stem", "B": B, "old": fmt(t["old"]), "new": fmt(t["new"])})
        print(f"stem B={B}: frames_to_tensor + conv2d {t['old'][0]:.1f} us, conv_stem_u8 {t['new'][0]:.1f} us", flush=True)
        z = (torch.randn(B, 3, H, W, generator=g) * 2).cuda()
        nw = (1 + 0.1 * torch.randn(3, generator=g)).cuda()
        nb = (0.1 * torch.randn(3, generator=g)).cuda()

        def old_tail():
            with torch.no_grad():
                return ops.tensor_to_frames(ops.tanh_image(ops.instance_norm(z, nw, nb), image=True))

        t = interleaved({"old": old_tail, "new": lambda: ops.instance_norm_tanh_frames(z, nw, nb)}, iters)
        rows.append({"what": "tail", "B": B, "S": ops.instnorm_chunks(3, H * W), "old": fmt(t["old"]),
                     "new": fmt(t["new"])})
        print(f"tail B={B}: IN + tanh_image + tensor_to_frames {t['old'][0]:.1f} us, fused {t['new'][0]:.1f} us",
              flush=True)
    res["stem_tail"] = rows


class Baseline:
    """The path before vst.rtnstv.inference: the training forward under no_grad between the two frame
    kernels, driven by Inference's own loop."""

    def __init__(self, model, clip, batch):
        self.model, self.clip, self.B = model, clip, batch
        self.up = PinnedUploader("cuda", batch)

    def __iter__(self):
        host = None
        for i in range(0, len(self.clip), self.B):
            x = self.up.upload(list(self.clip[i:i + self.B]))
            with torch.no_grad():
                frames = ops.tensor_to_frames(self.model(x))
            if host is None or host.shape[0] < frames.shape[0]:
                host = torch.empty(tuple(frames.shape), dtype=torch.uint8, pin_memory=True)
            h = host[:frames.shape[0]]
            h.copy_(frames)
            for img in h.numpy():
                yield img.copy()


def fps(make, n, repeats):
    out = []
    for _ in range(repeats):
        it = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in it)
        out.append(k / (time.perf_counter() - t0))
        assert k == n
    return out


def whole(res, T, iters):
    torch.manual_seed(0)
    model = StylizingNetwork().cuda().eval()
    sd = model.state_dict()
    clip = video_frames(5, T, H, W)
    rows = []
    for B in (1, 8):
        dev = torch.from_numpy(clip[:B]).cuda()

        def old_fwd():
            with torch.no_grad():
                return ops.tensor_to_frames(model(ops.frames_to_tensor(dev)))

        new_frames = I.forward_frames(model, dev)
        d = (new_frames.int() - old_fwd().int()).abs()
        t = interleaved({"old": old_fwd, "new": lambda: I.forward_frames(model, dev)}, max(4, iters // (4 * B)), warmup=3)
        mk_new = lambda: I.Inference(StylizingNetwork, sd, clip, batch_frames=B)  # noqa: E731
        mk_old = lambda: Baseline(model, clip, B)  # noqa: E731
        fps(mk_new, T, 1), fps(mk_old, T, 1)  # warm-up
        f_new, f_old = [], []
        for _ in range(5):
            f_new += fps(mk_new, T, 1)
            f_old += fps(mk_old, T, 1)
        row = {"B": B, "frames": T,
               "forward_us_per_frame": {"old": fmt(tuple(v / B for v in t["old"])), "new": fmt(tuple(v / B for v in t["new"]))},
               "fps_end_to_end": {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                  for k, v in (("old", f_old), ("new", f_new))},
               "new_vs_old_bytes": {"max_abs_diff": int(d.max()), "differing_share": float((d > 0).float().mean())}}
        rows.append(row)
        print(f"B={B}: forward per frame old {t['old'][0] / B:.1f} us new {t['new'][0] / B:.1f} us | end to end "
              f"old {row['fps_end_to_end']['old']['median']} fps new {row['fps_end_to_end']['new']['median']} fps | "
              f"bytes {row['new_vs_old_bytes']}", flush=True)
    res["whole"] = rows


RULES = {  # candidate host rules for S of the norms inside the network (the tail, C == 3, is always split:
    # its moments launch exists whatever S is)
    "tail_only": lambda C, HW, base: base(C, HW) if C == 3 else 1,
    "planes_over_128k": lambda C, HW, base: base(C, HW) if (C == 3 or HW > 131072) else 1,
    "shipped": lambda C, HW, base: base(C, HW),  # every plane past the register-resident kernels (> 32768)
}


def rules(res, iters):
    """forward_frames per frame under each candidate rule, interleaved, B = 1 and 8."""
    torch.manual_seed(0)
    model = StylizingNetwork().cuda().eval()
    clip = video_frames(5, 8, H, W)
    base = ops.instnorm_chunks

    rows = []
    try:
        for B in (1, 8):
            dev = torch.from_numpy(clip[:B]).cuda()

            def run(rule):
                def fn():
                    ops.instnorm_chunks = lambda C, HW: rule(C, HW, base)
                    return I.forward_frames(model, dev)
                return fn

            t = interleaved({k: run(r) for k, r in RULES.items()}, max(4, iters // (4 * B)), warmup=3)
            rows.append({"B": B, "forward_us_per_frame": {k: fmt(tuple(v / B for v in r)) for k, r in t.items()}})
            print(f"rules B={B}: " + "  ".join(f"{k}: {r[0] / B:.1f}" for k, r in t.items()) + " us per frame", flush=True)
    finally:
        ops.instnorm_chunks = base
    res["rules"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--parts", default="norm,rules,stem_tail,whole")
    ap.add_argument("--out", default=os.path.join("profiles", "rt_infer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rt_infer_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "frame": [H, W], "iters": a.iters, "policy": ops.gemm_mode_name(),
           "in_split": ops.IN_SPLIT}
    parts = a.parts.split(",")
    if "norm" in parts:
        norm_ab(res, a.iters)
    if "rules" in parts:
        rules(res, a.iters)
    if "stem_tail" in parts:
        stem_tail(res, a.iters)
    if "whole" in parts:
        whole(res, a.frames, a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
