"""Every library call of one step of each trainer and one forward of each inference path, one line
per call: the entry name, every int / long / float / double argument by value, every pointer as 0 or 1
(NULL or not), the stream as s0, s1, ... in order of first appearance.  Two trees that print the same
trace issue the same calls with the same arguments on the same streams; a host-side refactor is checked
by comparing the sha256 of the two traces.

    python tools/launch_trace.py > trace.txt        (needs a GPU; the hash goes to stderr)

Only vst._lib internals are replaced (_Lib.__getattr__), so the tool runs unchanged on any tree that
has that binding.  Shapes are the golden-step shapes of the tests, the smallest the networks accept.
"""
import ctypes
import hashlib
import os
import re
import sys
import threading
import traceback

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "video-style-transfer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402
from oracle import shapes  # noqa: E402
from vst import _lib, ops  # noqa: E402

DEV = "cuda:0"
POLICIES = ("f32", "bf16x6", "parity", "f16")
LINES = []
_LOCK = threading.Lock()
_STREAMS = {}
_BY_VALUE = (ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double)


def _stream_entries():
    """Names of the entry points whose last parameter is `void* stream` (the header names it)."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"(vst_\w+)\s*\(([^)]*)\bstream\s*\)\s*;", text)}


_HAS_STREAM = _stream_entries()


def _fmt(name, fn, args):
    out = [name]
    types = fn.argtypes or []
    for i, (t, a) in enumerate(zip(types, args)):
        if i == len(types) - 1 and name in _HAS_STREAM:
            key = int(a or 0)
            out.append(_STREAMS.setdefault(key, f"s{len(_STREAMS)}"))
        elif t in _BY_VALUE:
            out.append(repr(float(a)) if t in (ctypes.c_float, ctypes.c_double) else str(int(a)))
        else:
            out.append("0" if a is None or a == 0 else "1")
    return " ".join(out)


def _recording_getattr(self, name):
    fn = getattr(self.load(), name)

    def call(*args):
        with _LOCK:
            LINES.append(_fmt(name, fn, args))
        rc = fn(*args)
        if fn.restype is ctypes.c_int and rc != 0:
            raise _lib.VstError(f"{name} failed: {self.load().vst_strerror(rc).decode()} (rc={rc})")
        return rc

    return call


_lib._Lib.__getattr__ = _recording_getattr


def seeded(module, spec, seed):
    module.load_state_dict(dict(oracle.seeded_params(spec, seed)))
    return module


def G(t):
    return t.contiguous().to(DEV)


# ------------------------------------------------------------------------------------------ trainers
def _pair_inputs(B=2, H=32, W=64):
    from vst.synthetic import frame_pair_parts, style_image

    img1, img2, f01, f10, motion = frame_pair_parts(11, B, H, W)
    frames = G(torch.stack([img1, img2]))
    occ = ops.flow_warp_mask(G(f01), G(f10))
    mask = G(occ.cpu() * motion)
    return frames, G(f10), mask, G(style_image(12, H, W))


def reconet(config):
    from vst.reconet import network as N
    from vst.reconet.train import ReCoNetTrainer

    frames, flow, mask, style = _pair_inputs()
    model = seeded(N.ReCoNet(), shapes.reconet(), 1).to(DEV)
    vgg = seeded(N.Vgg16(), shapes.vgg16(), 2).to(DEV)
    tr = ReCoNetTrainer.for_script("train_coco2014" if config == 2 else "train_candy", model, vgg, style)
    if tr.single:
        tr.step(frames.reshape(-1, *frames.shape[2:]))
    else:
        tr.step(frames, flow, mask)


def sd2():
    from vst.reconet import network as N
    from vst.reconet.train import SD_LOSS_WEIGHTS, ReCoNetTrainer

    frames, flow, mask, style = _pair_inputs()
    teacher = seeded(N.ReCoNetSD1(), shapes.reconet_sd1(), 3)
    student = seeded(N.ReCoNetSD2(), shapes.reconet_sd2(), 4)
    student.load_state_dict(teacher.state_dict(), strict=False)
    vgg = seeded(N.Vgg16(), shapes.vgg16(), 2).to(DEV)
    tr = ReCoNetTrainer(student.to(DEV), vgg, style, weights=SD_LOSS_WEIGHTS, teacher=teacher.to(DEV).eval(),
                        sd_index=(0, 0))
    tr.step(frames, flow, mask)


def rtnstv():
    from vst.rtnstv.network import StylizingNetwork
    from vst.rtnstv.train import RTNSTVTrainer
    from vst.rtnstv.vgg19 import VGG19

    frames, flow, mask, style = _pair_inputs()
    net = seeded(StylizingNetwork(), shapes.rtnstv(), 5).to(DEV)
    vgg = seeded(VGG19(), shapes.vgg19_rt(), 6).to(DEV)
    RTNSTVTrainer(net, vgg, style).step(frames, flow, mask)


def _adaattn(activation):
    from vst.adaattn.network import StylizingNetwork
    from vst.adaattn.vgg19 import VGG19

    model = seeded(StylizingNetwork(activation), shapes.stylizing_network(), 7).to(DEV)
    return model, seeded(VGG19(), shapes.vgg19(), 8).to(DEV)


def adaattn_video(activation):
    from vst.adaattn.train import AdaAttNTrainer
    from vst.synthetic import content_style_batch

    model, vgg = _adaattn(activation)
    tr = AdaAttNTrainer(model, vgg, activation=activation)
    tr.step(G(torch.stack(content_style_batch(13, 2, 64, 128))))


def adaattn_image(activation):
    from vst.adaattn.train import AdaAttNTrainer
    from vst.synthetic import content_style_batch

    model, vgg = _adaattn(activation)
    tr = AdaAttNTrainer(model, vgg, activation=activation)
    c1, _, s = content_style_batch(14, 2, 64, 96)
    tr.image_step(G(c1), G(s))


# ----------------------------------------------------------------------------------------- inference
def reconet_infer():
    from vst.reconet import network as N
    from vst.synthetic import video_frames

    model = seeded(N.ReCoNet(), shapes.reconet(), 1).to(DEV).eval()
    frames = torch.from_numpy(video_frames(15, 2, 36, 60)).to(DEV)
    with torch.no_grad():
        *_, y = model(ops.frames_to_tensor(frames))
        ops.tensor_to_frames(y, frames=torch.empty_like(frames))


def adaattn_infer(activation):
    from vst.adaattn import inference as I
    from vst.synthetic import content_style_batch

    model, vgg = _adaattn(activation)
    c1, _, s = content_style_batch(16, 2, 64, 128)
    state = I.encode_style(vgg.eval(), model.eval(), G(s[:1]))
    I.stylize(vgg, model, state, G(c1), frames=torch.empty((2, 64, 128, 3), dtype=torch.uint8, device=DEV))


def rtnstv_infer():
    from vst.rtnstv import inference as I
    from vst.rtnstv.network import StylizingNetwork
    from vst.synthetic import video_frames

    net = seeded(StylizingNetwork(), shapes.rtnstv(), 5).to(DEV).eval()
    I.forward_frames(net, torch.from_numpy(video_frames(17, 2, 36, 60)).to(DEV))


def lpips_fwd():
    from vst.lpips import LPIPS

    torch.manual_seed(18)
    m = LPIPS(pretrained=False, net="vgg", pnet_rand=True, verbose=False).to(DEV)
    a, b = (torch.rand(2, 3, 32, 64, device=DEV) * 2 - 1 for _ in range(2))
    with torch.no_grad():
        m(a, b)


CASES = [("reconet.c2", lambda: reconet(2)), ("reconet.c3", lambda: reconet(3)), ("sd2", sd2), ("rtnstv", rtnstv),
         ("aa.video.cosine", lambda: adaattn_video("cosine")), ("aa.video.softmax", lambda: adaattn_video("softmax")),
         ("aa.image.cosine", lambda: adaattn_image("cosine")), ("aa.image.softmax", lambda: adaattn_image("softmax")),
         ("reconet.infer", reconet_infer), ("aa.infer.cosine", lambda: adaattn_infer("cosine")),
         ("aa.infer.softmax", lambda: adaattn_infer("softmax")), ("rtnstv.infer", rtnstv_infer), ("lpips", lpips_fwd)]


def main():
    only = sys.argv[1:]
    for policy in POLICIES:
        for name, run in CASES:
            if only and not any(o in f"{policy}.{name}" for o in only):
                continue
            ops.use_policy(policy)
            LINES.append(f"# {policy} {name}")
            try:
                run()
                torch.cuda.synchronize()
            except Exception as e:  # a trainer that does not take this policy: the refusal is the record
                LINES.append(f"# {policy} {name}: {type(e).__name__}: {e}")
                print(f"[launch_trace] {policy} {name}:\n{traceback.format_exc()}", file=sys.stderr, flush=True)
    text = "\n".join(LINES) + "\n"
    sys.stdout.write(text)
    print(f"[launch_trace] {len(LINES)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
