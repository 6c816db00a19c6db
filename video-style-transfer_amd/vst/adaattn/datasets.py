"""Datasets of the AdaAttN trainers with the per-item work on the GPU (AA/datasets.py:16-185,
AA/utilities.py:31-43): drop-ins for `Coco`, `WikiArt`, `CocoWikiArt`, `Videvo`, `VidevoWikiArt` (same
names and constructors, same file indexing, same item tuples, the same random draws in the same order
from the global `random` / torch generators), plus `CocoWikiArtLoader` / `VidevoWikiArtLoader`, the
batched replacements of `DataLoader(dataset, batch_size, shuffle=True)` (AA/train_image.py,
AA/train_video.py) that yield what `AdaAttNTrainer.step_batch` takes.

Split of the work:
  host   -- file indexing (torchvision's ImageFolder order, restated below: torchvision is not a
            dependency), JPEG / PNG decode (Pillow, `Image.open(p).convert("RGB")` as pil_loader; video
            frames through vst.metrics.imread), every random draw, and the packing of one pinned block
            per batch (ops.stage_ragged): descriptors, Pillow coefficient tables sliced to the crop,
            the decoded rasters;
  device -- `toTensorCrop` = Resize(size_resize) -> RandomCrop(size_crop) -> toTensor255 of all images
            of a batch, whatever their source sizes, as ONE copy and ONE launch that computes the crop
            window only (ops.resize_crop_ragged, bit-exact with Pillow); video frames through
            ops.frames_to_tensor.
Items come back as device tensors; there is no CPU compute path.
"""
import os
import random

import numpy as np
import torch
from PIL import Image

from .. import ops
from .._lib import VstError
from ..metrics import imread
from ..reconet.datasets import _no_worker, _prefetched, _ShardedLoader

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def list_files(directory):
    """AA/utilities.py:58-60."""
    return sorted(f.path for f in os.scandir(directory) if f.is_file())


def list_folders(directory):
    """AA/utilities.py:63-65."""
    return sorted(f.path for f in os.scandir(directory) if f.is_dir())


def pil_loader(path):
    """torchvision.datasets.folder.pil_loader, as a raster: (H, W, 3) uint8."""
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


class toTensorCrop:  # noqa: N801 (reference name)
    """AA/utilities.py:31-43: Compose([Resize(size_resize), RandomCrop(size_crop), toTensor255]); sizes
    are (height, width).  Calling it on a decoded image draws the crop origin as RandomCrop does and
    makes the (3, Hc, Wc) item on the GPU."""

    def __init__(self, size_resize: tuple = (512, 512), size_crop: tuple = (256, 256), device=None):
        self.size_resize, self.size_crop = tuple(size_resize), tuple(size_crop)
        self.device = torch.device(device) if device is not None else None

    def get_params(self):
        """RandomCrop.get_params on the resized image: the origin (i, j) = (top, left).  Draws nothing
        only when both sizes match; a matching width alone still consumes its (zero) draw."""
        (h, w), (th, tw) = self.size_resize, self.size_crop
        if h < th or w < tw:
            raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(h, w)}")
        if w == tw and h == th:
            return 0, 0
        i = torch.randint(0, h - th + 1, size=(1,)).item()
        j = torch.randint(0, w - tw + 1, size=(1,)).item()
        return i, j

    def __call__(self, img):
        staged = ops.stage_ragged([np.asarray(img)], self.size_resize, self.size_crop, [self.get_params()])
        return ops.resize_crop_ragged(staged, device=self.device)[0]


class ImageFolder(torch.utils.data.Dataset):
    """torchvision.datasets.ImageFolder's indexing (find_classes + make_dataset): classes are the sorted
    sub-directories of root; per class `sorted(os.walk(dir, followlinks=True))`, then `sorted(fnames)`,
    files whose lower-cased name ends in IMG_EXTENSIONS; a class without one raises FileNotFoundError.
    Items are (transform(image), class index)."""

    def __init__(self, root, transform=None):
        self.root, self.transform = root, transform
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples, seen = [], set()
        for cls in self.classes:
            for d, _, fnames in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
                for fname in sorted(fnames):
                    if fname.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(d, fname), self.class_to_idx[cls]))
                        seen.add(cls)
        empty = sorted(set(self.classes) - seen)
        if empty:
            raise FileNotFoundError(f"Found no valid file for the classes {', '.join(empty)}. "
                                    f"Supported extensions are: {', '.join(IMG_EXTENSIONS)}")
        self.imgs = self.samples
        self.targets = [s[1] for s in self.samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        _no_worker("ImageFolder")
        path, target = self.samples[idx]
        sample = pil_loader(path)
        if self.transform is not None:
            sample = self.transform(sample)
        return sample, target


def Coco(path="../datasets/coco", size_crop: tuple = (256, 256), size_resize: tuple = (512, 512), device=None):  # noqa: N802
    """AA/datasets.py:16-21.  size_crop: (height, width)."""
    return ImageFolder(root=path, transform=toTensorCrop(size_resize, size_crop, device))


def WikiArt(path="../datasets/WikiArt", size_crop: tuple = (256, 256), size_resize: tuple = (512, 512), device=None):  # noqa: N802
    """AA/datasets.py:24-29.  size_crop: (height, width)."""
    return ImageFolder(root=path, transform=toTensorCrop(size_resize, size_crop, device))


def stage_crops(plan):
    """Host half of a batch of crops: plan = [(path, (Hr, Wr), (Hc, Wc), (y0, x0))] with one crop size;
    decode every file and pack the block (ops.stage_ragged)."""
    crop = plan[0][2]
    for p in plan:
        if tuple(p[2]) != tuple(crop):
            raise VstError(f"{p[0]}: crop {tuple(p[2])} differs from the batch's {tuple(crop)} (one launch, one crop size)")
    return ops.stage_ragged([pil_loader(p[0]) for p in plan], [p[1] for p in plan], crop, [p[3] for p in plan])


def _planned(folder, idx):
    """(path, resize, crop, freshly drawn origin) of item idx of a Coco / WikiArt folder."""
    t = folder.transform
    return folder.samples[idx][0], t.size_resize, t.size_crop, t.get_params()


class CocoWikiArt(torch.utils.data.Dataset):
    """AA/datasets.py:32-44: item idx = (coco[idx], wikiart[random index]).  The size / device keywords
    are additions (the reference fixes 512 -> 256 x 256)."""

    def __init__(self, coco_path="../datasets/coco", wikiart_path="../datasets/WikiArt", size_resize=(512, 512),
                 size_crop=(256, 256), device=None):
        self.coco = Coco(coco_path, size_crop, size_resize, device)
        self.wikiart = WikiArt(wikiart_path, size_crop, size_resize, device)
        self.coco_len, self.wikiart_len = len(self.coco), len(self.wikiart)
        self.size_crop = tuple(size_crop)
        self.device = torch.device(device) if device is not None else None

    def __len__(self):
        return self.coco_len

    def draw(self, idx):
        """Every random draw of item idx, in the reference's order: the style index (`random`), the
        content crop origin, the style crop origin (torch).  Returns the two planned crops."""
        wikiart_idx = random.randint(0, self.wikiart_len - 1)
        return _planned(self.coco, idx), _planned(self.wikiart, wikiart_idx)

    def __getitem__(self, idx):
        _no_worker("CocoWikiArt")
        out = ops.resize_crop_ragged(stage_crops(list(self.draw(idx))), device=self.device)
        return out[0], out[1]


class Sintel(torch.utils.data.Dataset):
    """AA/datasets.py:47-101 builds a RAFT model in its constructor to estimate the flows; RAFT is out
    of scope here."""

    def __init__(self, image_size: tuple = (256, 512), path="../datasets/MPI-Sintel-complete", scene="all",
                 device: str = "cuda"):
        raise VstError("Sintel estimates its flows with torchvision's raft_large, which this project does not "
                       "provide (DESIGN.md §7); evaluate against MPI-Sintel's ground-truth flows with "
                       "vst.adaattn.evaluate.sintel_temporal_error")


def get_frames(video_path="../datasets/Videvo", img_size=(512, 256)):
    """AA/datasets.py:104-133: every video under video_path -> ./Videvo/frames/<video>/<frame>.jpg,
    resized with cv2.INTER_AREA.  Video decode and INTER_AREA are cv2's; without cv2 this raises."""
    try:
        import cv2  # noqa: PLC0415
    except ImportError:
        cv2 = None
    if cv2 is None or not hasattr(cv2, "VideoCapture"):
        raise VstError("get_frames needs OpenCV (cv2.VideoCapture, cv2.resize INTER_AREA), which is not "
                       "installed; extract the frames elsewhere into <path>/frames/<video>/<frame>.jpg")
    for videos_idx, file in enumerate(list_files(video_path)):
        save_dir = f"./Videvo/frames/{videos_idx:05d}/"
        os.makedirs(save_dir, exist_ok=True)
        cap = cv2.VideoCapture(file)
        frames_idx = 0
        while True:
            ret, frame = cap.read()
            if not ret:
                break
            frame = cv2.resize(frame, img_size, interpolation=cv2.INTER_AREA)
            cv2.imwrite(os.path.join(save_dir, f"{frames_idx:05d}.jpg"), frame)
            frames_idx += 1
        cap.release()


def stage_frames(groups):
    """Host half of video items: groups = B lists of T frame paths -> pinned (T, B, H, W, 3) uint8 cv2
    (BGR) frames; all frames of a batch share one size."""
    frames = None
    for b, paths in enumerate(groups):
        for t, p in enumerate(paths):
            a = imread(p)
            if frames is None:
                frames = torch.empty((len(paths), len(groups)) + a.shape, dtype=torch.uint8,
                                     pin_memory=torch.cuda.is_available())
            if tuple(frames.shape[2:]) != a.shape or len(paths) != frames.shape[0]:
                raise VstError(f"{p}: frame {a.shape} differs from the batch's {tuple(frames.shape[2:])}")
            frames[t, b].numpy()[...] = a
    return frames


def frames_to_device(frames, out):
    """Device half: one H2D copy, cv2 frames -> RGB fp32 in [0, 255] (toTensor255 of cvtColor(BGR2RGB))
    written into `out`, (T * B, 3, H, W) contiguous."""
    fr = frames.to(out.device, non_blocking=True)
    return ops.frames_to_tensor(fr.view((-1,) + tuple(fr.shape[2:])), bgr=True, out=out)


class Videvo(torch.utils.data.Dataset):
    """AA/datasets.py:136-170: every window of frame_num + 1 consecutive frames of each folder of
    <path>/frames; items (img1, img2) = channel-stacked frames [0, F) and [1, F]."""

    def __init__(self, path: str = "./Videvo", frame_num: int = 1, device=None):
        super().__init__()
        path_frame = os.path.join(path, "frames")
        assert os.path.exists(path_frame), f"Path {path_frame} does not exist."
        assert 1 <= frame_num, "Frame number must be equal or greater than 1."
        self.frames = []
        for folder in list_folders(path_frame):
            files = list_files(folder)
            for i in range(len(files) - frame_num):
                self.frames.append(files[i:i + frame_num + 1])
        self.frame_num = frame_num
        self.length = len(self.frames)
        self.device = torch.device(device) if device is not None else None
        print(f"Videvo total data: {self.length}")

    def __len__(self):
        return self.length

    def __getitem__(self, idx: int):
        _no_worker("Videvo")
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        fr = stage_frames([self.frames[idx]])
        T, _, H, W, _ = fr.shape
        imgs = frames_to_device(fr, torch.empty((T, 3, H, W), dtype=torch.float32, device=dev))
        F = self.frame_num  # torch.cat(imgs[a:b], dim=0) of (3, H, W) frames: a view of the stacked frames
        return imgs[:F].reshape(3 * F, H, W), imgs[1:].reshape(3 * F, H, W)


class VidevoWikiArt(torch.utils.data.Dataset):
    """AA/datasets.py:173-185: item idx = (videvo[idx] frames 1 and 2, wikiart[random index] at a
    (256, 512) crop).  The size / device keywords are additions."""

    def __init__(self, videvo_path="./Videvo", wikiart_path="../datasets/WikiArt", size_resize=(512, 512),
                 size_crop=(256, 512), device=None):
        self.videvo = Videvo(videvo_path, device=device)
        self.wikiart = WikiArt(wikiart_path, size_crop, size_resize, device)
        self.videvo_len, self.wikiart_len = len(self.videvo), len(self.wikiart)
        self.size_crop = tuple(size_crop)
        self.device = self.videvo.device

    def __len__(self):
        return self.videvo_len

    def draw(self, idx):
        """The reference's draws of item idx: the style index (`random`), then the style crop origin
        (the frames draw nothing).  Returns (frame paths, planned style crop)."""
        wikiart_idx = random.randint(0, self.wikiart_len - 1)
        return self.videvo.frames[idx], _planned(self.wikiart, wikiart_idx)

    def __getitem__(self, idx):
        _no_worker("VidevoWikiArt")
        paths, style = self.draw(idx)
        buf = _video_batch(stage_frames([paths]), stage_crops([style]), self.size_crop, self.device)
        return buf[0, 0], buf[1, 0], buf[2, 0]


def _video_batch(frames, staged, crop, device):
    """[3, B, 3, H, W] = content1, content2, style from staged frames and staged style crops."""
    T, B, H, W, _ = frames.shape
    if (H, W) != tuple(crop):
        raise VstError(f"video frames are {H}x{W} but the style crop is {crop[0]}x{crop[1]}: "
                       "one batch buffer holds both, so the sizes must match")
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    buf = torch.empty((3, B, 3, H, W), dtype=torch.float32, device=dev)
    frames_to_device(frames, buf[:2].view(2 * B, 3, H, W))
    ops.resize_crop_ragged(staged, buf[2])
    return buf


# ------------------------------------------------------------------------------- loaders
class _PlannedLoader(_ShardedLoader):
    """Rank sharding and the seeded permutation of _ShardedLoader.  Every random draw of a batch is made
    on the consumer thread, in item order, when the batch's plan is built (`dataset.draw`); only the
    plan -- paths and drawn origins -- goes to the staging thread, so prefetching never reorders the
    global generators' streams.  prefetch=False stages on the consumer thread as well."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, seed=None, device=None, rank=None,
                 world_size=None, prefetch=True):
        super().__init__(dataset, batch_size, shuffle, drop_last, seed, device, rank, world_size)
        self.prefetch = prefetch
        if self.device is None:
            self.device = dataset.device

    def _plans(self):
        for idx in self._index_batches():
            yield [self.dataset.draw(j) for j in idx]

    def __iter__(self):
        if not self.prefetch:
            for plan in self._plans():
                yield self._finish(self._stage(plan))
            return
        box = {}

        def stage(plan):
            try:
                box["staged"] = self._stage(plan)
            except BaseException as e:  # re-raised on the consumer side
                box["error"] = e

        yield from _prefetched(self._plans(), stage, box, self._finish)


class CocoWikiArtLoader(_PlannedLoader):
    """`DataLoader(CocoWikiArt(...), batch_size, shuffle)` replacement (AA/train_image.py): yields one
    [2, B, 3, Hc, Wc] device buffer, content then style -- one staged block, one copy and one ragged
    launch for all 2B images."""

    def _stage(self, plan):
        return len(plan), stage_crops([c for c, _ in plan] + [s for _, s in plan])

    def _finish(self, st):
        B, staged = st
        Hc, Wc = staged.crop
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        buf = torch.empty((2, B, 3, Hc, Wc), dtype=torch.float32, device=dev)
        ops.resize_crop_ragged(staged, buf.view(2 * B, 3, Hc, Wc))
        return buf


class VidevoWikiArtLoader(_PlannedLoader):
    """`DataLoader(VidevoWikiArt(...), batch_size, shuffle)` replacement (AA/train_video.py:48-52): yields
    one [3, B, 3, H, W] device buffer (content1, content2, style), the form AdaAttNTrainer.encode takes:
    frames through frames_to_tensor, styles through one ragged launch into slice 2."""

    def _stage(self, plan):
        return stage_frames([f for f, _ in plan]), stage_crops([s for _, s in plan])

    def _finish(self, st):
        frames, staged = st
        return _video_batch(frames, staged, staged.crop, self.device)
