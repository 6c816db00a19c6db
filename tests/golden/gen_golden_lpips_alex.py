"""Generate tests/golden/lpips_alex.npz by running the REFERENCE's lpips package with its AlexNet trunk.

CONTAINER-ONLY (needs the reference tree gen_golden_eval.py names, which never travels to the GPU box).  Re-run with
    python tests/golden/gen_golden_lpips_alex.py
Like gen_golden_lpips.py it imports the reference's own `lpips` package with tests/golden/_stubs ahead on
sys.path.  The stub `torchvision.models` has no `alexnet`, so this script sets `torchvision.models.alexnet`
at run time: a function that accepts and ignores `pretrained=` / `weights=` and returns a module whose
`features` is torchvision's documented layer list (Conv 3->64 k11 s4 p2, ReLU, MaxPool(3,2), Conv 64->192
k5 p2, ReLU, MaxPool(3,2), Conv 192->384 k3 p1, ReLU, Conv 384->256 k3 p1, ReLU, Conv 256->256 k3 p1, ReLU,
MaxPool(3,2)).  No real torchvision model is constructed and nothing is downloaded: the reference's
`tv.alexnet(pretrained=True)` is that local call.

Recorded (inputs and outputs only -- no program text of the reference):
  * the trunk's seed (`seed_module(model.net, 511)`, oracle/seeding.py; the weights are not stored) and the
    five learned 1x1 weight vectors the reference's `LPIPS(net="alex")` loaded from its own
    weights/v0.1/alex.pth (1,152 floats);
  * the list of the model's state_dict key names;
  * the uint8 RGB image pairs of tests/lpips_alex_ref.py `PAIRS`: 31x31 (N=1, the minimum), 35x67 (N=2),
    64x98 (N=1);
  * per pair: the total and the five per-level values (`retPerLayer=True`), the `normalize=True` value on
    the [0,1] form, the `lpips=False` baseline, the `version="0.0"` value (no ScalingLayer; the same v0.1
    linear weights loaded into it), and for 35x67 the `spatial=True` map.
`forward(t0, t0) == 0` exactly and every level contributes at least 2 % of each total (both asserted).  The
archive is written with fixed zip timestamps, so a re-run is byte-identical.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_eval as G  # noqa: E402  (puts _stubs, the repository and tests/ on sys.path)
import gen_golden_lpips as GL  # noqa: E402

import lpips_alex_ref as A  # noqa: E402
import lpips_ref as L  # noqa: E402
from oracle.seeding import seed_module  # noqa: E402


class _AlexNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2))


def _alexnet(pretrained=False, weights=None, **_):
    return _AlexNet()


def _import_lpips():
    import torchvision.models as tvm  # the stub

    assert os.path.dirname(os.path.abspath(tvm.__file__)).startswith(os.path.join(HERE, "_stubs")), tvm.__file__
    tvm.alexnet = _alexnet
    return GL._import_lpips()[0]


def _model(pkg, lins=None, **kw):
    m = pkg.LPIPS(net="alex", verbose=False, **kw)
    seed_module(m.net, A.TRUNK_SEED)
    if lins is not None:
        m.load_state_dict(lins, strict=False)
    return m


def main():
    torch.set_num_threads(8)
    lpips = _import_lpips()
    out = {"trunk_seed": np.array(A.TRUNK_SEED)}
    model = _model(lpips)
    out["state_dict_keys"] = np.array(list(model.state_dict()))
    lins = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("lin")}
    for k in range(5):
        w = model.state_dict()[f"lin{k}.model.1.weight"]
        assert w.shape == (1, A.CHNS[k], 1, 1) and torch.equal(w, model.state_dict()[f"lins.{k}.model.1.weight"])
        out[f"lin{k}"] = w.reshape(-1).numpy().astype(np.float32)
    base = _model(lpips, lpips=False)
    v00 = _model(lpips, lins=lins, version="0.0", pretrained=False)
    spat = _model(lpips, spatial=True)

    with torch.no_grad():
        for key in A.PAIRS:
            img0, img1 = A.image_pair(key)
            t0 = torch.cat([lpips.im2tensor(i) for i in img0])
            t1 = torch.cat([lpips.im2tensor(i) for i in img1])
            val, res = model.forward(t0, t1, retPerLayer=True)
            total = val.reshape(-1).numpy().astype(np.float32)
            layers = np.stack([r.reshape(-1).numpy() for r in res]).astype(np.float32)
            share = layers / total[None]
            assert share.min() >= 0.02, (key, share)
            assert torch.equal(model.forward(t0, t0), torch.zeros_like(val))
            out[key + "_img0"], out[key + "_img1"] = img0, img1
            out[key + "_total"], out[key + "_layers"] = total, layers
            out[key + "_norm01"] = model.forward(L.unit01(img0), L.unit01(img1), normalize=True).reshape(-1).numpy()
            out[key + "_baseline"] = base.forward(t0, t1).reshape(-1).numpy()
            out[key + "_v00"] = v00.forward(t0, t1).reshape(-1).numpy()
            if key == "a35":
                out[key + "_spatial"] = spat.forward(t0, t1).numpy().astype(np.float32)
            print(key, "total", total, "shares", share.min(axis=1), "norm01", out[key + "_norm01"], "baseline",
                  out[key + "_baseline"], "v0.0", out[key + "_v00"])

    path = os.path.join(HERE, "lpips_alex.npz")
    G.save_npz(path, out)
    print("lpips alex fixture written:", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
