"""Generate tests/golden/aa_infer.npz by running the REFERENCE's AdaAttN inference chain.

CONTAINER-ONLY (needs /root/reference, which never travels to the GPU box).  Re-run with
    python tests/golden/gen_golden_aa_infer.py
It imports the reference's own `network.py`, `vgg19.py` and `utilities.py` (with tests/golden/_stubs
ahead on sys.path, like gen_golden.py, plus a cv2 stand-in whose cvtColor is the channel reversal
OpenCV's BGR2RGB is) and runs, per frame, what AA/infer_video.py:54-68 runs: the reference's
`cv2_to_tensor` -> VGG19 -> StylizingNetwork(fc, fs) -> clamp(0, 255) -> HWC -> astype(uint8), with
the style's VGG features computed once.  Models are seeded (oracle/seeding.py), so the tests rebuild
them from the stored seeds; no weights are stored.

Seeded weights give outputs of about +-4, which clamp + truncation would turn into a trivial image:
the last conv's weight is multiplied by a scale and its bias shifted (both constants stored per case;
the tests apply the same change), and the generator asserts that 5-30 % of the output bytes are
saturated and that the others span at least 200 levels.

It also runs oracle.adaattn_ref.stylize on the same inputs and asserts |diff| <= 1 everywhere with at
most 0.25 % of the bytes differing from the reference's frames -- the condition behind the GPU
tests' 1 % cap -- and stores the measured share.  Nothing from the reference is copied into the
repository: only inputs / outputs (data) are saved.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
AA_DIR = "/root/reference/Revisit-Attention-Mechanism-in-Arbitrary-Neural-Style-Transfer-(AdaAttN)"

sys.path.insert(0, os.path.join(HERE, "_stubs"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "video-style-transfer_amd"))

from oracle import adaattn_ref as A  # noqa: E402
from oracle import seeded_params, shapes  # noqa: E402
from oracle.seeding import seed_module  # noqa: E402
from vst.synthetic import video_frames  # noqa: E402

torch.set_num_threads(8)

# tag: activation, frames, frame (H, W), style (H, W), seeds (model, vgg, video, style), and the
# last conv's (weight scale, bias shift): the seeded outputs' 5 % / 95 % points (a: 1.2 / 6.2, b: -2.7 /
# 13.7 before the change) land just outside [0, 255]
CASES = {
    "a": ("cosine", 3, (32, 64), (32, 64), (71, 72, 73, 74), (56.0, -75.0)),
    "b": ("softmax", 2, (48, 80), (32, 64), (81, 82, 83, 84), (16.0, 40.0)),
}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(AA_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def style_picture(seed, hw):
    return np.random.default_rng(seed).integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)


def rescale_conv8(sd, scale, shift):
    """The fixture's change of the last conv, on a state dict / parameter dict (in place)."""
    sd["decoder.conv8.conv.weight"].mul_(scale)
    sd["decoder.conv8.conv.bias"].add_(shift)


def main():
    for n in ("utilities", "vgg19", "network"):
        sys.modules.pop(n, None)
    sys.path.insert(0, AA_DIR)
    util = _load("utilities")
    util.cv2.COLOR_BGR2RGB = 4
    util.cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])
    vgg_mod, net_mod = _load("vgg19"), _load("network")
    out = {}
    for tag, (activation, T, (H, W), shw, seeds, conv8) in CASES.items():
        clip = video_frames(seeds[2], T, H, W)
        pic = style_picture(seeds[3], shw)
        with torch.no_grad():
            vgg = vgg_mod.VGG19().eval()
            seed_module(vgg, seeds[1])
            net = net_mod.StylizingNetwork(activation=activation).eval()
            seed_module(net, seeds[0])
            rescale_conv8(net.state_dict(), *conv8)
            s = util.toTensor255(pic).unsqueeze(0)
            fs = vgg(s)
            frames, pre0 = [], None
            for i, frame in enumerate(clip):
                c = util.cv2_to_tensor(frame).unsqueeze(0)
                cs = net(vgg(c), fs)
                if i == 0:
                    pre0 = cs[0].numpy().copy()
                frames.append(cs.clamp(0, 255).squeeze(0).permute(1, 2, 0).numpy().astype(np.uint8))
            frames = np.stack(frames)
            sat = float(((frames == 0) | (frames == 255)).mean())
            levels = len(np.unique(frames[(frames > 0) & (frames < 255)]))
            assert 0.05 <= sat <= 0.30 and levels >= 200, (tag, sat, levels)
            # the oracle on the same inputs
            P = seeded_params(shapes.stylizing_network(), seeds[0])
            rescale_conv8(P, *conv8)
            VP = seeded_params(shapes.vgg19(), seeds[1])
            ofs = A.vgg19(VP, s)
            oframes = []
            for frame in clip:
                c = torch.from_numpy(np.ascontiguousarray(frame[..., ::-1].transpose(2, 0, 1))).float().div(255).mul(255)
                y = A.stylize(P, A.vgg19(VP, c.unsqueeze(0)), ofs, activation)
                oframes.append(y.clamp(0, 255)[0].permute(1, 2, 0).numpy().astype(np.uint8))
            d = np.abs(np.stack(oframes).astype(int) - frames.astype(int))
            share = float((d > 0).mean())
            assert d.max() <= 1 and share <= 0.0025, (tag, d.max(), share)
        out[f"{tag}_frames"] = frames
        out[f"{tag}_pre0"] = pre0.astype(np.float32)
        out[f"{tag}_meta"] = np.array([*seeds, T, H, W, *shw])
        out[f"{tag}_conv8"] = np.array(conv8, dtype=np.float64)
        out[f"{tag}_activation"] = np.array(activation)
        out[f"{tag}_oracle_share"] = np.array(share)
        print(tag, activation, "saturated", round(sat, 4), "levels", levels, "oracle differing share", share,
              "pre0 range", float(pre0.min()), float(pre0.max()))
    np.savez_compressed(os.path.join(HERE, "aa_infer.npz"), **out)
    print("aa_infer fixture written")


if __name__ == "__main__":
    main()
