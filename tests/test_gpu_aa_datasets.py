"""AdaAttN datasets on a real MI355X: the ragged resize-and-crop kernel bit-exact against Pillow, the
dataset items and loader batches against tests/aa_datasets_ref.py, and one `fit` epoch per trainer fed
from a tiny on-disk tree.  Everything here is integer work followed by one fp32 `(b / 255) * 255`, so
every comparison is `torch.equal`."""
import random

import numpy as np
import pytest
import torch

import aa_datasets_ref as A
import oracle
from oracle import shapes

pytestmark = pytest.mark.gpu
DEV = "cuda"

RESIZE = (96, 80)
# source (Hs, Ws): upscale in both axes; identity; 1.4x / 3.5x with odd row bytes; 8.3x vertical (19 taps)
# with odd row bytes; tiny; 37x horizontal (77 taps): beyond the LDS bounds, the per-pixel path
SOURCES = ((30, 40), (96, 80), (131, 277), (800, 97), (7, 9), (64, 3001))
CROPS = ((19, 70), (96, 80), (1, 1))


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(17)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SOURCES]
    imgs[2][::2] //= 4  # structure, so that a misplaced tap shows
    return imgs


def _origins(crop):
    my, mx = RESIZE[0] - crop[0], RESIZE[1] - crop[1]
    return [(0, 0), (my, mx), (min(33, my), min(7, mx)), (min(51, my), min(3, mx)), (my, 0), (min(77, my), min(9, mx))]


@pytest.mark.parametrize("crop", CROPS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_ragged_kernel_bit_exact(sources, crop):
    from vst import ops

    origins = _origins(crop)
    st = ops.stage_ragged(sources, RESIZE, crop, origins)
    tiled, fallback = st.tile_paths()
    if crop != (1, 1):
        assert fallback[5] > 0 and not fallback[:5].any() and tiled[:5].all()
    N = len(sources)
    buf = torch.full((3, N, 3) + crop, float("nan"), device=DEV)
    ops.resize_crop_ragged(st, buf[1])
    again = ops.resize_crop_ragged(st)  # the same batch, the same draws, a fresh output
    got = buf.cpu()
    assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all()
    for i, (a, org) in enumerate(zip(sources, origins)):
        assert torch.equal(got[1, i], A.crop_ref(a, RESIZE, org, crop)), (i, SOURCES[i], org)
    assert torch.equal(again.cpu(), got[1])


def test_ragged_per_item_resize_targets(sources):
    from vst import ops

    sizes = [(96, 80), (40, 33), (50, 131), (20, 21), (64, 64), (25, 300)]
    origins = [(3, 5), (0, 0), (17, 100), (1, 0), (31, 23), (4, 271)]
    out = ops.resize_crop_ragged(ops.stage_ragged(sources, sizes, (19, 21), origins)).cpu()
    for i, a in enumerate(sources):
        assert torch.equal(out[i], A.crop_ref(a, sizes[i], origins[i], (19, 21))), i


def test_ragged_rejects_bad_outputs(sources):
    from vst import ops
    from vst._lib import VstError

    st = ops.stage_ragged(sources[:2], RESIZE, (8, 8), [(0, 0), (1, 1)])
    with pytest.raises(VstError):
        ops.resize_crop_ragged(st, torch.empty(2, 3, 8, 9, device=DEV))
    with pytest.raises(VstError):
        ops.resize_crop_ragged(st, torch.empty(2, 3, 8, 8))


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("aa_trees")
    coco, wiki, vid = (str(root / n) for n in ("coco", "wikiart", "videvo"))
    A.write_image_tree(coco, 31, classes=("train",), per_class=8)
    A.write_image_tree(wiki, 32, classes=("cubism", "ukiyo_e"), per_class=4)
    A.write_videvo_tree(vid, 33, (64, 64), folders=2, frames=3)
    return coco, wiki, vid


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


IMG = dict(size_resize=(96, 80), size_crop=(64, 64))
VID = dict(size_resize=(96, 64), size_crop=(64, 64))  # full-width crop: the j draw is consumed and zero


def test_dataset_items_match_reference(trees):
    from vst.adaattn import datasets as DS

    coco, wiki, vid = trees
    cs, ws, frames = A.make_dataset(coco), A.make_dataset(wiki), A.videvo_index(vid)
    ds = DS.CocoWikiArt(coco, wiki, device=DEV, **IMG)
    _seed(3)
    got = [ds[i] for i in (0, 3, 7, 2)]
    _seed(3)
    for i, (c, s) in zip((0, 3, 7, 2), got):
        rc, rs = A.coco_wikiart_item(cs, ws, i, IMG["size_resize"], IMG["size_crop"])
        assert torch.equal(c.cpu(), rc) and torch.equal(s.cpu(), rs), i
    vds = DS.VidevoWikiArt(vid, wiki, device=DEV, **VID)
    _seed(4)
    got = [vds[i] for i in (1, 3)]
    _seed(4)
    for i, item in zip((1, 3), got):
        ref = A.videvo_wikiart_item(frames, ws, i, VID["size_resize"], VID["size_crop"])
        assert len(item) == 3 and all(torch.equal(g.cpu(), r) for g, r in zip(item, ref)), i
    # the plain folder datasets and Videvo alone (frame_num 2: channel-stacked frames)
    folder = DS.WikiArt(wiki, size_crop=(64, 80), size_resize=(96, 80), device=DEV)
    _seed(5)
    img, cls = folder[6]
    _seed(5)
    assert cls == 1 and torch.equal(img.cpu(), A.to_tensor_crop(A.load_rgb(ws[6][0]), (96, 80), (64, 80)))
    v2 = DS.Videvo(vid, frame_num=2, device=DEV)
    assert len(v2) == 2
    a, b = v2[1]
    ra, rb = A.videvo_item(A.videvo_index(vid, 2)[1])
    assert tuple(a.shape) == (6, 64, 64) and torch.equal(a.cpu(), ra) and torch.equal(b.cpu(), rb)


def _count_ragged(monkeypatch):
    from vst import ops

    calls, real = [], ops.resize_crop_ragged

    def counted(staged, out=None, device=None):
        calls.append(staged.n)
        return real(staged, out, device)

    monkeypatch.setattr(ops, "resize_crop_ragged", counted)
    return calls


def test_loaders_match_per_item_path(trees, monkeypatch):
    from vst.adaattn import datasets as DS

    coco, wiki, vid = trees
    ds = DS.CocoWikiArt(coco, wiki, device=DEV, **IMG)
    shards = [DS.CocoWikiArtLoader(ds, batch_size=2, shuffle=True, seed=7, rank=r, world_size=2) for r in (0, 1)]
    assert len(shards[0]) == len(shards[1]) == 2
    loader = shards[1]
    order = [j for idx in loader._index_batches() for j in idx]
    loader.rng = random.Random(7)  # the permutation above advanced the loader's own generator
    calls = _count_ragged(monkeypatch)
    _seed(8)
    batches = list(loader)
    assert calls == [4, 4]  # one ragged launch per batch, content and style together
    del calls[:]
    _seed(8)
    items = [ds[j] for j in order]
    for k, buf in enumerate(batches):
        assert tuple(buf.shape) == (2, 2, 3, 64, 64)
        for b in range(2):
            assert torch.equal(buf[0, b], items[2 * k + b][0]) and torch.equal(buf[1, b], items[2 * k + b][1])
    vds = DS.VidevoWikiArt(vid, wiki, device=DEV, **VID)
    vloader = DS.VidevoWikiArtLoader(vds, batch_size=2, shuffle=True, seed=7, rank=0, world_size=2)
    assert len(vloader) == 1
    order = [j for idx in vloader._index_batches() for j in idx]
    vloader.rng = random.Random(7)
    del calls[:]
    _seed(9)
    (buf,) = list(vloader)
    assert calls == [2] and tuple(buf.shape) == (3, 2, 3, 64, 64)
    _seed(9)
    for b, j in enumerate(order):
        for t, ref in enumerate(vds[j]):
            assert torch.equal(buf[t, b], ref), (t, b)


def test_video_loader_refuses_mismatched_frames(trees):
    from vst._lib import VstError
    from vst.adaattn import datasets as DS

    _, wiki, vid = trees
    vds = DS.VidevoWikiArt(vid, wiki, size_resize=(96, 80), size_crop=(32, 48), device=DEV)
    with pytest.raises(VstError, match="64x64.*32x48"):
        next(iter(DS.VidevoWikiArtLoader(vds, batch_size=2)))


def _seeded(module, spec, seed):
    module.load_state_dict(oracle.seeded_params(spec, seed))
    return module


@pytest.mark.parametrize("kind", ["image", "video"])
def test_fit_one_epoch_from_a_tree(trees, kind, monkeypatch):
    from vst.adaattn import datasets as DS
    from vst.adaattn.network import StylizingNetwork
    from vst.adaattn.train import AdaAttNTrainer
    from vst.adaattn.vgg19 import VGG19
    from vst.reconet.loop import StepLog, fit

    coco, wiki, vid = trees
    act = "softmax" if kind == "image" else "cosine"
    model = _seeded(StylizingNetwork(act), shapes.stylizing_network(), 41).to(DEV)
    vgg = _seeded(VGG19(), shapes.vgg19(), 42).to(DEV)
    tr = AdaAttNTrainer(model, vgg, activation=act)
    if kind == "image":
        loader = DS.CocoWikiArtLoader(DS.CocoWikiArt(coco, wiki, device=DEV, **IMG), batch_size=1, shuffle=True, seed=1,
                                      rank=0, world_size=4)
        lead = 2
    else:
        loader = DS.VidevoWikiArtLoader(DS.VidevoWikiArt(vid, wiki, device=DEV, **VID), batch_size=2, shuffle=True,
                                        seed=1)
        lead = 3
    assert len(loader) == 2
    seen, real = [], tr.step_batch
    monkeypatch.setattr(tr, "step_batch", lambda batch: seen.append(batch) or real(batch))
    before = tr.flat.p.detach().clone()
    _seed(2)
    log = fit(tr, loader, epochs=1, log=StepLog(every=1))
    assert len(seen) == 2 and all(isinstance(b, torch.Tensor) and b.shape[0] == lead for b in seen)
    assert len(log.records) == 2
    for rec in log.records:
        assert np.isfinite(rec["loss"]) and np.isfinite(rec["loss_gs"]) and np.isfinite(rec["loss_lf"])
        assert ("loss_is" in rec) == (kind == "video")
    assert torch.isfinite(tr.flat.p).all() and not torch.equal(before, tr.flat.p.detach())
