"""Generate tests/golden/lpips_vgg.npz by running the REFERENCE's lpips package and AA/eval.py lpips_loss.

CONTAINER-ONLY (needs the reference tree gen_golden_eval.py names, which never travels to the GPU box).  Re-run with
    python tests/golden/gen_golden_lpips.py
Like gen_golden_eval.py it imports the reference's own modules with tests/golden/_stubs ahead on
sys.path (architecture-only torchvision; the cv2 stand-in, completed here with `imread` through Pillow)
and puts empty stand-ins for `SIFID`, `matplotlib` and -- where they are absent -- `tqdm` into
sys.modules so that the `lpips` package and AA/eval.py import.

Recorded (inputs and outputs only -- no program text of the reference):
  * the trunk's seed (`seed_module(model.net, seed)`, oracle/seeding.py; the weights are not stored) and
    the five learned 1x1 weight vectors the reference's `LPIPS(net="vgg")` loaded from its own
    weights/v0.1/vgg.pth (1,472 floats);
  * the uint8 RGB image pairs of tests/lpips_ref.py `PAIRS`: 16x16 (N=1), 32x48 (N=2), ragged 36x60 (N=1);
  * per pair: the total and the five per-level values (`retPerLayer=True`), the `normalize=True` value on
    the [0,1] form, the `lpips=False` baseline, the `version="0.0"` value (no ScalingLayer; the same v0.1
    linear weights loaded into it, so one set of weights serves the whole fixture), and for 32x48 the
    `spatial=True` map;
  * AA/eval.py `lpips_loss` over the 36x60 pair as PNG files, `lpips_loss.loss_fn` preassigned to the
    seeded model;
  * the (256,3) table of `im2tensor` followed by `ScalingLayer`.
Every level contributes at least 0.5 % of each total (asserted).  The archive is written with fixed zip
timestamps, so a re-run is byte-identical.
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_eval as G  # noqa: E402  (puts _stubs, the repository and tests/ on sys.path)

import lpips_ref as L  # noqa: E402
import metrics_ref as M  # noqa: E402
from oracle.seeding import seed_module  # noqa: E402

AA_DIR = G.AA_DIR


def _import_lpips():
    G._complete_cv2()
    for name in ("matplotlib", "matplotlib.pyplot"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = t
    sifid = types.ModuleType("SIFID")
    sifid.InceptionV3 = sifid.calculate_activation_statistics = sifid.calculate_frechet_distance = None
    sys.modules["SIFID"] = sifid
    sys.modules.pop("lpips", None)
    sys.path.insert(0, AA_DIR)
    import lpips  # the reference's package

    for n in ("utilities", "vgg19", "network", "eval"):
        sys.modules.pop(n, None)
    G._load(AA_DIR, "utilities")
    G._load(AA_DIR, "vgg19")
    ev = G._load(AA_DIR, "eval")
    sys.path.remove(AA_DIR)
    return lpips, ev


def _model(pkg, lins=None, **kw):
    m = pkg.LPIPS(net="vgg", verbose=False, **kw)
    seed_module(m.net, L.TRUNK_SEED)
    if lins is not None:
        m.load_state_dict(lins, strict=False)
    return m


def main():
    torch.set_num_threads(8)
    lpips, ev = _import_lpips()
    out = {"trunk_seed": np.array(L.TRUNK_SEED)}
    model = _model(lpips)
    lins = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("lin")}
    for k in range(5):
        w = model.state_dict()[f"lin{k}.model.1.weight"]
        assert w.shape == (1, L.CHNS[k], 1, 1) and torch.equal(w, model.state_dict()[f"lins.{k}.model.1.weight"])
        out[f"lin{k}"] = w.reshape(-1).numpy().astype(np.float32)
    base = _model(lpips, lpips=False)
    v00 = _model(lpips, lins=lins, version="0.0", pretrained=False)
    spat = _model(lpips, spatial=True)

    with torch.no_grad():
        for key in L.PAIRS:
            img0, img1 = L.image_pair(key)
            t0 = torch.cat([lpips.im2tensor(i) for i in img0])
            t1 = torch.cat([lpips.im2tensor(i) for i in img1])
            val, res = model.forward(t0, t1, retPerLayer=True)
            total = val.reshape(-1).numpy().astype(np.float32)
            layers = np.stack([r.reshape(-1).numpy() for r in res]).astype(np.float32)
            share = layers / total[None]
            assert share.min() >= 0.005, (key, share)
            assert torch.equal(model.forward(t0, t0), torch.zeros_like(val))
            out[key + "_img0"], out[key + "_img1"] = img0, img1
            out[key + "_total"], out[key + "_layers"] = total, layers
            out[key + "_norm01"] = model.forward(L.unit01(img0), L.unit01(img1), normalize=True).reshape(-1).numpy()
            out[key + "_baseline"] = base.forward(t0, t1).reshape(-1).numpy()
            out[key + "_v00"] = v00.forward(t0, t1).reshape(-1).numpy()
            if key == "p32":
                out[key + "_spatial"] = spat.forward(t0, t1).numpy().astype(np.float32)
            print(key, "total", total, "shares", share.min(axis=1), "norm01", out[key + "_norm01"], "baseline",
                  out[key + "_baseline"], "v0.0", out[key + "_v00"])

        # AA/eval.py lpips_loss over PNG files (cv2.imread is BGR: write_png takes BGR)
        img0, img1 = L.image_pair("p36")
        with tempfile.TemporaryDirectory() as tmp:
            opt = argparse.Namespace(device="cpu", path0=os.path.join(tmp, "a.png"), path1=os.path.join(tmp, "b.png"))
            M.write_png(opt.path0, img0[0][..., ::-1])
            M.write_png(opt.path1, img1[0][..., ::-1])
            ev.lpips_loss.loss_fn = model
            out["p36_lpips_loss"] = np.array(ev.lpips_loss(opt, no_print=True), dtype=np.float64)
        print("lpips_loss", float(out["p36_lpips_loss"]))

        ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # (256,1,3)
        table = model.scaling_layer(lpips.im2tensor(ramp))  # (1,3,256,1)
        out["input_table"] = table[0, :, :, 0].numpy().T.astype(np.float32).copy()

    path = os.path.join(HERE, "lpips_vgg.npz")
    G.save_npz(path, out)
    print("lpips fixture written:", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
