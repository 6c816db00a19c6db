"""AdaAttN image-batch preparation on synthetic decoded rasters (no codec): the ragged resize-and-crop
(one staged block, one copy, one launch; ops.stage_ragged / ops.resize_crop_ragged) against the best
composition the flow-dataset pieces offer: `prepare_images(stage_images(..), (512, 512))` per side (one
copy, one pil_resize launch and one index_copy_ per distinct source size) followed by the crop slices.

    python tools/aa_dataprep_bench.py [--out profiles/aa_dataprep_bench.json] [--rounds 4] [--iters 10]

Batch: 8 content rasters of COCO-like sizes and 8 style rasters of WikiArt-like sizes, Resize((512, 512)),
crop 256 x 256 at seeded origins (AA/train_image.py's defaults).  Both paths are timed in ONE process in
alternating rounds (A B A B ..), each round the median HIP-event time of `iters` calls after a warm-up;
the spread across rounds is reported with the result.  Two windows per path:
  with_copy     the H2D copies of the staged host buffers plus the kernels (what a loader step pays on
                the device; both paths copy the same raster bytes),
  kernels_only  the rasters already on the device.
Event windows include the gaps between launches, which is the point for the composition's ~48 calls.
Per size class, one item alone (kernels only): the ragged launch against pil_resize_to_tensor255 to
512 x 512, to show whether either path wins only on some sizes.
Host staging (packing decoded rasters into pinned memory) is timed with the host clock and reported
separately; on real data the JPEG decode in front of it dominates loading and is not measured here.
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
from vst.reconet import datasets as RD  # noqa: E402

COPY_PEAK = 6.29e12  # bytes/s, the measured HBM copy rate (tools/calib)
CONTENT = ((480, 640), (427, 640), (640, 480), (375, 500), (480, 640), (640, 427), (500, 375), (427, 640))
STYLE = ((600, 800), (900, 700), (1200, 1600), (1536, 2048), (2000, 1500), (2500, 3200), (3000, 2400), (3500, 3500))
RESIZE, CROP = (512, 512), (256, 256)


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stage_arrays(arrays):
    """stage_images (vst.reconet.datasets) from decoded rasters: pinned staging grouped by source size."""
    groups = {}
    for i, a in enumerate(arrays):
        groups.setdefault(a.shape, []).append((i, a))
    staged = []
    for shape, items in groups.items():
        host = torch.empty((len(items),) + shape, dtype=torch.uint8).pin_memory()
        for j, (_, a) in enumerate(items):
            host[j].numpy()[...] = a
        staged.append(([i for i, _ in items], host))
    return len(arrays), staged


def prepare_on_device(groups, n, resolution, dev):
    """prepare_images (vst.reconet.datasets) with the groups already on the device."""
    out = torch.empty((n, 3, resolution[1], resolution[0]), dtype=torch.float32, device=dev)
    for idx, imgs in groups:
        out.index_copy_(0, idx, ops.pil_resize_to_tensor255(imgs, resolution))
    return out


def window_bytes(staged):
    """Bytes the algorithm must move: every item's source window (the rows and columns its crop reads),
    its sliced tables, and the fp32 output."""
    ints, (Hc, Wc) = staged.ints, staged.crop
    total = 0
    for d in staged.desc:
        hb = ints[d[5]:d[5] + 2 * Wc].reshape(Wc, 2)
        vb = ints[d[8]:d[8] + 2 * Hc].reshape(Hc, 2)
        cols = int(hb[-1].sum() - hb[0, 0])
        rows = int(vb[-1].sum() - vb[0, 0])
        total += rows * cols * 3 + 4 * (2 * Wc + Wc * int(d[7]) + 2 * Hc + Hc * int(d[10])) + 12 * Hc * Wc
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "aa_dataprep_bench.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aa_dataprep_bench needs the GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    sides = [[rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes] for sizes in (CONTENT, STYLE)]
    B = len(CONTENT)
    origins = [(int(rng.integers(0, RESIZE[0] - CROP[0] + 1)), int(rng.integers(0, RESIZE[1] - CROP[1] + 1)))
               for _ in range(2 * B)]
    wh = (RESIZE[1], RESIZE[0])

    # ---- host staging, host clock (median of 5)
    def stage_new():
        return ops.stage_ragged(sides[0] + sides[1], RESIZE, CROP, origins)

    def stage_old():
        return [stage_arrays(s) for s in sides]

    host_ms = {}
    for name, fn in (("ragged", stage_new), ("composition", stage_old)):
        fn()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        host_ms[name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    staged, old = stage_new(), stage_old()

    # ---- device paths
    buf = torch.empty((2, B, 3) + CROP, dtype=torch.float32, device=dev)
    flat = buf.view(2 * B, 3, *CROP)
    block = staged.host.to(dev)
    old_dev = [([(torch.tensor(idx, device=dev), host.to(dev)) for idx, host in groups], n) for n, groups in old]

    def crops(full, org):
        return [full[i, :, y:y + CROP[0], x:x + CROP[1]] for i, (y, x) in enumerate(org)]

    def new_with_copy():
        ops.resize_crop_ragged(staged, flat)

    def new_kernels():
        ops.resize_crop_ragged(staged, flat, block=block)

    def old_with_copy():
        return [crops(RD.prepare_images(st, wh, dev), origins[k * B:(k + 1) * B]) for k, st in enumerate(old)]

    def old_kernels():
        return [crops(prepare_on_device(g, n, wh, dev), origins[k * B:(k + 1) * B]) for k, (g, n) in enumerate(old_dev)]

    def old_kernels_stacked():  # ... and gathered into the contiguous batch buffer a trainer step takes
        for k, side in enumerate(old_kernels()):
            torch.stack(side, out=buf[k])

    new_kernels()
    same = all(torch.equal(buf[k, i], c) for k, side in enumerate(old_kernels()) for i, c in enumerate(side))
    paths = {"ragged_with_copy": new_with_copy, "composition_with_copy": old_with_copy,
             "ragged_kernels_only": new_kernels, "composition_kernels_only": old_kernels,
             "composition_kernels_only_stacked": old_kernels_stacked}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in paths}
    for _ in range(a.rounds):  # A B A B ..: every path once per round
        for k, fn in paths.items():
            rounds[k].append(statistics.median(event_ms(fn, a.iters) for _ in range(3)))
    # ---- per size class, kernels only: one item alone on each path (which side wins where)
    per_item = []
    for i, arr in enumerate(sides[0][:4] + sides[1]):
        org = origins[i if i < 4 else B + i - 4]
        st1 = ops.stage_ragged([arr], RESIZE, CROP, [org])
        blk1, img1, out1 = st1.host.to(dev), torch.from_numpy(arr).to(dev).unsqueeze(0), flat[:1]
        fns = {"ragged": lambda: ops.resize_crop_ragged(st1, out1, block=blk1),
               "composition": lambda: ops.pil_resize_to_tensor255(img1, wh)}
        for fn in fns.values():
            fn()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(event_ms(fn, a.iters))
        per_item.append({"source_hw": list(arr.shape[:2]), "ragged_us": 1e3 * statistics.median(ms["ragged"]),
                         "composition_us": 1e3 * statistics.median(ms["composition"]),
                         "ragged_us_min_max": [1e3 * min(ms["ragged"]), 1e3 * max(ms["ragged"])],
                         "composition_us_min_max": [1e3 * min(ms["composition"]), 1e3 * max(ms["composition"])]})
        print(f"  {arr.shape[0]}x{arr.shape[1]}: ragged {per_item[-1]['ragged_us']:.1f} us, "
              f"pil_resize 512x512 {per_item[-1]['composition_us']:.1f} us", flush=True)
    tiled, fallback = staged.tile_paths()
    nbytes = window_bytes(staged)
    res = {"device": torch.cuda.get_device_name(0), "batch": {"content_hw": CONTENT, "style_hw": STYLE, "resize": RESIZE,
                                                               "crop": CROP, "origins": origins},
           "outputs_bitwise_equal": bool(same), "rounds": a.rounds, "iters_per_window": a.iters,
           "device_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "per_round": v,
                             "spread": max(v) - min(v)} for k, v in rounds.items()},
           "host_staging_ms": host_ms, "staged_block_bytes": staged.host.numel(),
           "tiles_tiled_path": tiled.tolist(), "tiles_per_pixel_path": fallback.tolist(),
           "items_all_tiled": int((fallback == 0).sum()), "items_with_per_pixel_tiles": int((fallback > 0).sum()),
           "algorithm_bytes": nbytes, "single_item_kernels_only": per_item}
    t_new = res["device_ms"]["ragged_kernels_only"]["median"]
    res["ragged_kernel_bytes_per_s"] = nbytes / (t_new * 1e-3)
    res["ragged_kernel_fraction_of_copy_peak"] = res["ragged_kernel_bytes_per_s"] / COPY_PEAK
    for w in ("with_copy", "kernels_only"):
        res[f"speedup_{w}"] = res["device_ms"][f"composition_{w}"]["median"] / res["device_ms"][f"ragged_{w}"]["median"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for k, v in res["device_ms"].items():
        print(f"{k}: {v['median']:.3f} ms (rounds {v['min']:.3f} .. {v['max']:.3f})")
    print(f"host staging: ragged {host_ms['ragged']['median']:.1f} ms, composition {host_ms['composition']['median']:.1f} ms; "
          f"bitwise equal {same}; {res['ragged_kernel_fraction_of_copy_peak']:.4f} of copy peak")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
