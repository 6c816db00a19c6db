"""torch-CPU restatement of the RTNSTV per-frame inference chain.  TEST INFRASTRUCTURE ONLY.

What RT/utilities.py:296-332 (`Inference.__iter__`) does with one cv2 frame, written from it (not
imported): BGR -> RGB, `toTensor255` (ToTensor then mul(255)), `StylizingNetwork.forward`
(oracle.rtnstv_ref.stylizer_forward), HWC, RGB -> BGR, `astype("uint8")`.  Pinned against the
reference's own frames by tests/golden/gen_golden_rt_infer.py and tests/test_rtnstv_inference.py.
Shared by the CPU and GPU tests of the inference path, with the fixture's cases and parameters.
"""
import numpy as np
import torch

import oracle
from oracle import rtnstv_ref as R
from oracle import shapes
from vst.synthetic import video_frames


def to255(rgb_u8):
    """toTensor255 of an HxWx3 uint8 RGB array: (1,3,H,W) fp32, x / 255 * 255."""
    return torch.from_numpy(np.ascontiguousarray(rgb_u8.transpose(2, 0, 1))).float().div(255).mul(255).unsqueeze(0)


def stylise(P, clip_bgr):
    """(T,H,W,3) uint8 BGR frames -> the (T,H,W,3) uint8 BGR frames Inference yields."""
    out = []
    with torch.no_grad():
        for f in clip_bgr:
            y = R.stylizer_forward(P, to255(f[..., ::-1]))
            out.append(np.ascontiguousarray(y[0].permute(1, 2, 0).numpy()[..., ::-1]).astype("uint8"))
    return np.stack(out)


def case_clip(tag, meta):
    """The input frames of a fixture case from its stored metadata (seed_model, seed_video, T, H, W)."""
    _, sv, T, H, W = (int(v) for v in meta)
    if tag == "a":
        return video_frames(sv, T, H, W)
    return np.random.default_rng(sv).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)


_PARAMS = {}


def case_params(g, tag):
    """The case's seeded StylizingNetwork parameters (CPU, detached, shared between tests), with the
    fixture's stored change of conv4.norm.weight applied."""
    if tag not in _PARAMS:
        P = {k: v.detach() for k, v in oracle.seeded_params(shapes.rtnstv(), int(g[f"{tag}_meta"][0])).items()}
        P["conv4.norm.weight"] = P["conv4.norm.weight"] * float(g[f"{tag}_norm_scale"])
        _PARAMS[tag] = P
    return _PARAMS[tag]


def frame_bars(frames, ref, what):
    """(max |diff|, share of differing bytes) of two uint8 frame stacks; printed before any assert."""
    d = np.abs(np.asarray(frames).astype(int) - np.asarray(ref).astype(int))
    share = float((d > 0).mean())
    print(f"{what}: max |diff| {d.max()}, differing share {share:.5f}")
    return int(d.max()), share


def case_bars(g, tag, frames, what):
    """The bars of a case's frames against the fixture: case a stores frame 0 whole, the first 48 rows
    of the others and per-channel sums (rc_infer.npz's layout), case b every frame."""
    frames = np.asarray(frames)
    if f"{tag}_frames" in g:
        return frame_bars(frames, g[f"{tag}_frames"], what)
    d0 = frame_bars(frames[0], g[f"{tag}_frame0"], what + " frame 0")
    dr = frame_bars(frames[:, :48], g[f"{tag}_rows"], what + " rows")
    sums = np.stack([f.reshape(-1, 3).astype(np.int64).sum(0) for f in frames])
    # |diff| <= 1 on at most 1 % of a channel's bytes moves its sum by at most that many
    px = frames.shape[1] * frames.shape[2]
    ds = float(np.abs(sums - g[f"{tag}_sums"]).max()) / px
    print(f"{what}: largest channel-sum difference / pixels {ds:.5f}")
    return max(d0[0], dr[0]), max(d0[1], dr[1], ds)
