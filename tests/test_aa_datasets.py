"""AdaAttN datasets (AA/datasets.py:16-185), host side: file indexing, the staged block of the ragged
resize-and-crop, the order of the random draws, loader prefetch, refusals and the trainer's batch
dispatch.  Oracle: tests/aa_datasets_ref.py (Pillow plus short restatements of torchvision, unpinned:
torchvision is not installed here).  Nothing in this file needs a GPU."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import aa_datasets_ref as A
from oracle import dataprep_ref as D
from vst import _lib

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libvst_hip.so not built")


def _touch_png(path, hw=(5, 4)):
    from PIL import Image

    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros(hw + (3,), np.uint8)).save(path, format="PNG")


def test_image_folder_order(tmp_path):
    from vst.adaattn import datasets as DS

    root = str(tmp_path / "wiki")
    names = ["b_cls/z.PNG", "b_cls/a.png", "b_cls/sub/k.JpEg", "b_cls/Sub2/deep/m.png", "a_cls/2.png", "a_cls/10.png",
             "a_cls/nested/0.png"]
    for n in names:
        _touch_png(os.path.join(root, n))
    with open(os.path.join(root, "a_cls", "notes.txt"), "w") as f:
        f.write("not an image")
    with open(os.path.join(root, "stray.png"), "w") as f:  # files directly under root belong to no class
        f.write("x")
    ds = DS.ImageFolder(root)
    want = ["a_cls/10.png", "a_cls/2.png", "a_cls/nested/0.png", "b_cls/a.png", "b_cls/z.PNG", "b_cls/Sub2/deep/m.png",
            "b_cls/sub/k.JpEg"]
    assert [os.path.relpath(p, root) for p, _ in ds.samples] == want
    assert [c for _, c in ds.samples] == [0, 0, 0, 1, 1, 1, 1]
    assert ds.classes == ["a_cls", "b_cls"] and len(ds) == 7
    assert ds.samples == A.make_dataset(root)


def test_image_folder_empty_class(tmp_path):
    from vst.adaattn import datasets as DS

    root = str(tmp_path / "coco")
    _touch_png(os.path.join(root, "full", "a.png"))
    os.makedirs(os.path.join(root, "hollow"))
    with open(os.path.join(root, "hollow", "readme.md"), "w") as f:
        f.write("x")
    with pytest.raises(FileNotFoundError, match="hollow"):
        DS.ImageFolder(root)
    with pytest.raises(FileNotFoundError):
        A.make_dataset(root)
    os.makedirs(str(tmp_path / "none"))
    with pytest.raises(FileNotFoundError):
        DS.ImageFolder(str(tmp_path / "none"))


def _walk_block(st, i):
    """Item i of a staged block evaluated in numpy from the block alone (per pixel, as the kernel's
    fallback does): what the device is asked to compute."""
    ints, raw = st.ints, st.host.numpy()
    d = st.desc[i]
    Hc, Wc = st.crop
    Hs, Ws, hks, vks = int(d[1]), int(d[2]), int(d[7]), int(d[10])
    row0, nrows = int(d[13]), int(d[14])
    img = np.zeros((Hs, Ws, 3), np.int64)  # only rows row0 .. row0 + nrows are staged
    img[row0:row0 + nrows] = raw[int(d[0]) * 16:int(d[0]) * 16 + nrows * Ws * 3].reshape(nrows, Ws, 3)
    hb = ints[d[5]:d[5] + 2 * Wc].reshape(Wc, 2)
    hk = ints[d[6]:d[6] + Wc * hks].reshape(Wc, hks).astype(np.int64)
    vb = ints[d[8]:d[8] + 2 * Hc].reshape(Hc, 2)
    vk = ints[d[9]:d[9] + Hc * vks].reshape(Hc, vks).astype(np.int64)
    half = 1 << (D.PRECISION_BITS - 1)
    out = np.empty((Hc, Wc, 3), np.uint8)
    for y in range(Hc):
        rows = img[vb[y, 0]:vb[y, 0] + vb[y, 1]]
        for x in range(Wc):
            win = rows[:, hb[x, 0]:hb[x, 0] + hb[x, 1]]
            h = np.clip((half + (win * hk[x, :hb[x, 1], None]).sum(1)) >> D.PRECISION_BITS, 0, 255)
            out[y, x] = np.clip((half + (h * vk[y, :vb[y, 1], None]).sum(0)) >> D.PRECISION_BITS, 0, 255)
    return D.to_tensor255(out)


@needs_lib
def test_staged_block_layout():
    from vst import ops

    rng = np.random.default_rng(3)
    shapes = [(30, 40), (131, 277), (7, 9), (24, 20)]
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    resize, crop = (24, 20), (5, 6)
    origins = [(0, 0), (19, 14), (3, 7), (11, 5)]
    st = ops.stage_ragged(imgs, resize, crop, origins)
    assert st.host.dtype == torch.uint8 and st.host.dim() == 1 and st.n == 4 and st.crop == crop
    desc, ints, raw = st.desc, st.ints, st.host.numpy()
    assert desc.shape == (4, ops.RAGGED_DESC_INTS)
    ends = []
    for i, (a, (y0, x0)) in enumerate(zip(imgs, origins)):
        Hs, Ws = a.shape[:2]
        d = desc[i]
        assert (d[1], d[2], d[3], d[4], d[11], d[12]) == (Hs, Ws, x0, y0, resize[0], resize[1])
        hb, hk = ops.pil_bilinear_coeffs(Ws, resize[1])
        vb, vk = ops.pil_bilinear_coeffs(Hs, resize[0])
        # the raster: only the source rows the crop's vertical taps read
        row0, row1 = int(vb[y0, 0]), int(vb[y0 + crop[0] - 1].sum())
        assert (d[13], d[14]) == (row0, row1 - row0)
        a = a[row0:row1]
        off = int(d[0]) * 16  # 16-byte aligned by construction of the field; inside the block, past the tables
        assert off + a.size + 3 <= raw.size
        np.testing.assert_array_equal(raw[off:off + a.size].reshape(a.shape), a)
        ends.append((off, off + a.size))
        assert (d[7], d[10]) == (hk.shape[1], vk.shape[1])
        np.testing.assert_array_equal(ints[d[5]:d[5] + 2 * crop[1]].reshape(-1, 2), hb[x0:x0 + crop[1]])
        np.testing.assert_array_equal(ints[d[6]:d[6] + crop[1] * d[7]].reshape(crop[1], -1), hk[x0:x0 + crop[1]])
        np.testing.assert_array_equal(ints[d[8]:d[8] + 2 * crop[0]].reshape(-1, 2), vb[y0:y0 + crop[0]])
        np.testing.assert_array_equal(ints[d[9]:d[9] + crop[0] * d[10]].reshape(crop[0], -1), vk[y0:y0 + crop[0]])
        assert min(d[5], d[6], d[8], d[9]) >= 4 * ops.RAGGED_DESC_INTS
        assert 4 * max(d[5] + 2 * crop[1], d[6] + crop[1] * d[7], d[8] + 2 * crop[0], d[9] + crop[0] * d[10]) <= min(
            int(x[0]) * 16 for x in desc)
        # the block alone reproduces Pillow's resize + crop
        assert torch.equal(_walk_block(st, i), A.crop_ref(imgs[i], resize, (y0, x0), crop))
    ends.sort()
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
    # the library's validator (host code) accepts it, and refuses a block whose descriptor lies
    lib = _lib.lib.load()
    args = (st.host.data_ptr(), st.host.numel(), 4, crop[0], crop[1])
    assert lib.vst_pil_ragged_check(*args) == 0
    tiled, fallback = st.tile_paths()
    assert tiled.tolist() == [1, 1, 1, 1] and fallback.tolist() == [0, 0, 0, 0]
    for field, value in ((0, raw.size // 16), (2, 100000), (5, ints.size - 3), (7, 1), (3, resize[1]), (1, 6),
                         (13, int(desc[1, 13]) + 1), (14, int(desc[1, 14]) - 1), (14, 1 << 20)):
        keep = int(desc[1, field])
        desc[1, field] = value
        assert lib.vst_pil_ragged_check(*args) == -1, field
        desc[1, field] = keep
    assert lib.vst_pil_ragged_check(*args) == 0
    assert lib.vst_pil_ragged_check(st.host.data_ptr(), 4 * 16 * 4 - 1, 4, crop[0], crop[1]) == -1
    with pytest.raises(_lib.VstError):
        ops.stage_ragged(imgs[:1], resize, crop, [(20, 0)])
    with pytest.raises(_lib.VstError):
        ops.stage_ragged([imgs[0][:, :, 0]], resize, crop, [(0, 0)])


@needs_lib
def test_per_item_resize_targets_and_fallback_split():
    from vst import ops

    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (12, 1600, 3), dtype=np.uint8), rng.integers(0, 256, (9, 8, 3), dtype=np.uint8)]
    st = ops.stage_ragged(imgs, [(10, 70), (12, 80)], (3, 66), [(2, 4), (9, 14)])
    assert (st.desc[:, 11].tolist(), st.desc[:, 12].tolist()) == ([10, 12], [70, 80])
    tiled, fallback = st.tile_paths()  # 1600 -> 70 over 64 columns: a window row beyond the LDS bound
    assert (tiled.tolist(), fallback.tolist()) == ([1, 2], [1, 0])
    for i, (res, org) in enumerate(zip([(10, 70), (12, 80)], [(2, 4), (9, 14)])):
        assert torch.equal(_walk_block(st, i), A.crop_ref(imgs[i], res, org, (3, 66)))


@pytest.fixture()
def trees(tmp_path):
    coco, wiki, vid = (str(tmp_path / n) for n in ("coco", "wikiart", "videvo"))
    A.write_image_tree(coco, 11, classes=("train",), per_class=6)
    A.write_image_tree(wiki, 12, classes=("cubism", "ukiyo_e"), per_class=4)
    A.write_videvo_tree(vid, 13, (16, 24), folders=2, frames=3)
    return coco, wiki, vid


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


def _rng_state():
    return random.getstate(), torch.get_rng_state().clone()


def _same_state(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1])


def test_draw_order_matches_reference(trees, capsys):
    from vst.adaattn import datasets as DS

    coco, wiki, vid = trees
    resize, crop = (48, 40), (20, 24)
    ds = DS.CocoWikiArt(coco, wiki, size_resize=resize, size_crop=crop)
    cs, ws = A.make_dataset(coco), A.make_dataset(wiki)
    assert len(ds) == 6 and ds.wikiart_len == 8
    _seed(5)
    got = [ds.draw(i) for i in (3, 0, 5)]
    state = _rng_state()
    _seed(5)
    for i, (c, s) in zip((3, 0, 5), got):
        widx = random.randint(0, len(ws) - 1)
        assert c == (cs[i][0], resize, crop, A.get_params(resize, crop))
        assert s == (ws[widx][0], resize, crop, A.get_params(resize, crop))
    assert _same_state(state, _rng_state())
    # the video dataset: the style crop spans the full width, and its zero j draw is still consumed
    vresize, vcrop = (40, 24), (16, 24)
    vds = DS.VidevoWikiArt(vid, wiki, size_resize=vresize, size_crop=vcrop)
    frames = A.videvo_index(vid)
    assert vds.videvo.frames == frames and len(vds) == 4
    _seed(6)
    got = [vds.draw(i) for i in (2, 1)]
    state = _rng_state()
    _seed(6)
    for i, (f, s) in zip((2, 1), got):
        widx = random.randint(0, len(ws) - 1)
        before = torch.get_rng_state().clone()
        org = A.get_params(vresize, vcrop)
        assert org[1] == 0 and not torch.equal(before, torch.get_rng_state())
        assert f == frames[i] and s == (ws[widx][0], vresize, vcrop, org)
    assert _same_state(state, _rng_state())
    # equal sizes: RandomCrop draws nothing
    same = DS.toTensorCrop((32, 32), (32, 32))
    before = _rng_state()
    assert same.get_params() == (0, 0) and _same_state(before, _rng_state())
    with pytest.raises(ValueError):
        DS.toTensorCrop((32, 32), (33, 32)).get_params()


@needs_lib
def test_loader_draws_identically_with_and_without_prefetch(trees, monkeypatch):
    from vst.adaattn import datasets as DS

    coco, wiki, vid = trees
    ds = DS.CocoWikiArt(coco, wiki, size_resize=(48, 40), size_crop=(20, 24))
    vds = DS.VidevoWikiArt(vid, wiki, size_resize=(40, 24), size_crop=(16, 24))

    def run(cls, dataset, prefetch):
        loader = cls(dataset, batch_size=2, shuffle=True, seed=9, prefetch=prefetch)
        monkeypatch.setattr(loader, "_finish", lambda st: st)  # the device half needs a GPU
        _seed(21)
        out = list(loader)
        return out, _rng_state()

    (a, sa), (b, sb) = run(DS.CocoWikiArtLoader, ds, True), run(DS.CocoWikiArtLoader, ds, False)
    assert len(a) == len(b) == 3 and _same_state(sa, sb)
    for (na, x), (nb, y) in zip(a, b):
        assert na == nb == 2 and x.n == 4 and torch.equal(x.host, y.host)
    # ... and equal to drawing item by item in the loader's order
    order = [j for idx in DS.CocoWikiArtLoader(ds, batch_size=2, shuffle=True, seed=9)._index_batches() for j in idx]
    _seed(21)
    plans = [ds.draw(j) for j in order]
    for k, (_, x) in enumerate(a):
        want = DS.stage_crops([plans[2 * k][0], plans[2 * k + 1][0], plans[2 * k][1], plans[2 * k + 1][1]])
        assert torch.equal(x.host, want.host)
    (a, sa), (b, sb) = run(DS.VidevoWikiArtLoader, vds, True), run(DS.VidevoWikiArtLoader, vds, False)
    assert len(a) == len(b) == 2 and _same_state(sa, sb)
    for (fa, x), (fb, y) in zip(a, b):
        assert tuple(fa.shape) == (2, 2, 16, 24, 3) and torch.equal(fa, fb) and torch.equal(x.host, y.host)


def test_dataloader_worker_is_refused(trees, monkeypatch):
    from vst.adaattn import datasets as DS

    coco, wiki, vid = trees
    ds = DS.CocoWikiArt(coco, wiki, size_resize=(48, 40), size_crop=(20, 24))
    vds = DS.VidevoWikiArt(vid, wiki, size_resize=(40, 24), size_crop=(16, 24))
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: types.SimpleNamespace(id=0))
    for d in (ds, vds, ds.coco, vds.videvo):
        with pytest.raises(_lib.VstError, match=r"prepared on the GPU.*DataLoader\(num_workers>0\)"):
            d[0]


def test_out_of_scope_entry_points_say_so(monkeypatch):
    from vst.adaattn import datasets as DS

    with pytest.raises(_lib.VstError, match="raft_large.*sintel_temporal_error"):
        DS.Sintel()
    monkeypatch.setitem(sys.modules, "cv2", None)  # `import cv2` raises ImportError
    with pytest.raises(_lib.VstError, match="OpenCV"):
        DS.get_frames("nowhere")


def test_drop_in_module_exports_reference_names():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-style-transfer_amd",
                        "adaattn", "datasets.py")
    ns = {"__file__": path, "__name__": "datasets"}
    exec(compile(open(path).read(), path, "exec"), ns)
    for name in ("Coco", "WikiArt", "CocoWikiArt", "Sintel", "get_frames", "Videvo", "VidevoWikiArt"):
        assert name in ns, name


def test_step_batch_dispatch():
    from vst.adaattn.train import AdaAttNTrainer

    tr = AdaAttNTrainer.__new__(AdaAttNTrainer)
    calls = []
    tr.image_step = lambda c, s: calls.append(("image", c, s)) or "image"
    tr.step = lambda c1, c2=None, s=None: calls.append(("video", c1, c2, s)) or "video"
    buf2, buf3 = torch.zeros(2, 1, 3, 4, 4), torch.zeros(3, 1, 3, 4, 4)
    buf2[1] += 1
    assert tr.step_batch(buf2) == "image"
    kind, c, s = calls.pop()
    assert kind == "image" and c.data_ptr() == buf2[0].data_ptr() and s.data_ptr() == buf2[1].data_ptr()
    assert tr.step_batch((buf2[0], buf2[1])) == "image"
    kind, c, s = calls.pop()
    assert kind == "image" and c.data_ptr() == buf2[0].data_ptr() and s.data_ptr() == buf2[1].data_ptr()
    assert tr.step_batch(buf3) == "video"
    kind, c1, c2, s = calls.pop()
    assert kind == "video" and c1 is buf3 and c2 is None and s is None
    assert tr.step_batch((buf3[0], buf3[1], buf3[2] + 2)) == "video"
    kind, c1, c2, s = calls.pop()
    assert kind == "video" and tuple(c1.shape) == (3, 1, 3, 4, 4) and float(c1[2].mean()) == 2 and c2 is None
