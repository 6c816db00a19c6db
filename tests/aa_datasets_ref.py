"""CPU oracle (test infrastructure only) for the AdaAttN datasets (AA/datasets.py:16-185,
AA/utilities.py:31-43).

The crop reference is Pillow itself -- `Image.fromarray(a).resize((Wr, Hr), Image.BILINEAR).crop(box)`
is what torchvision's Resize / RandomCrop do to a PIL image -- followed by the oracle's toTensor255.
torchvision is not installed where this suite runs, so the three pieces of it the datasets depend on
are restated here in a few lines each, every one citing the function it restates; they are NOT pinned
against torchvision.
"""
import os
import random

import numpy as np
import torch
from PIL import Image

from oracle import dataprep_ref as D

# torchvision/datasets/folder.py: IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def find_classes(directory):
    """torchvision/datasets/folder.py find_classes: sorted sub-directory names -> index."""
    classes = sorted(entry.name for entry in os.scandir(directory) if entry.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {directory}.")
    return classes, {cls_name: i for i, cls_name in enumerate(classes)}


def make_dataset(directory):
    """torchvision/datasets/folder.py make_dataset (extensions=IMG_EXTENSIONS, allow_empty=False):
    [(path, class index)] in class order, os.walk order sorted, file names sorted."""
    _, class_to_idx = find_classes(directory)
    instances, available = [], set()
    for target_class in sorted(class_to_idx.keys()):
        target_dir = os.path.join(directory, target_class)
        for root, _, fnames in sorted(os.walk(target_dir, followlinks=True)):
            for fname in sorted(fnames):
                path = os.path.join(root, fname)
                if path.lower().endswith(IMG_EXTENSIONS):  # has_file_allowed_extension
                    instances.append((path, class_to_idx[target_class]))
                    available.add(target_class)
    empty = set(class_to_idx.keys()) - available
    if empty:
        raise FileNotFoundError(f"Found no valid file for the classes {', '.join(sorted(empty))}. ")
    return instances


def get_params(hw, out_hw):
    """torchvision/transforms/transforms.py RandomCrop.get_params: (i, j) = (top, left); no draw only
    when both sizes match, otherwise BOTH draws (a zero-range one included)."""
    (h, w), (th, tw) = hw, out_hw
    if h < th or w < tw:
        raise ValueError("Required crop size is larger than input image size")
    if w == tw and h == th:
        return 0, 0
    i = torch.randint(0, h - th + 1, size=(1,)).item()
    j = torch.randint(0, w - tw + 1, size=(1,)).item()
    return i, j


def load_rgb(path):
    """torchvision/datasets/folder.py pil_loader."""
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


def crop_ref(a, resize, origin, crop):
    """toTensor255(Resize(resize)(img) cropped at origin): Pillow's resize and crop."""
    (Hr, Wr), (y0, x0), (Hc, Wc) = resize, origin, crop
    img = Image.fromarray(a).resize((Wr, Hr), Image.BILINEAR).crop((x0, y0, x0 + Wc, y0 + Hc))
    return D.to_tensor255(np.asarray(img))


def to_tensor_crop(a, resize, crop):
    """AA/utilities.py:31-43 toTensorCrop on a decoded image, drawing as RandomCrop does."""
    return crop_ref(a, resize, get_params(resize, crop), crop)


def coco_wikiart_item(coco, wikiart, idx, resize, crop):
    """AA/datasets.py:42-44 from the two make_dataset lists."""
    wikiart_idx = random.randint(0, len(wikiart) - 1)
    c = to_tensor_crop(load_rgb(coco[idx][0]), resize, crop)
    s = to_tensor_crop(load_rgb(wikiart[wikiart_idx][0]), resize, crop)
    return c, s


def videvo_index(path, frame_num=1):
    """AA/datasets.py:139-148."""
    frames = []
    for folder in sorted(f.path for f in os.scandir(os.path.join(path, "frames")) if f.is_dir()):
        files = sorted(f.path for f in os.scandir(folder) if f.is_file())
        for i in range(len(files) - frame_num):
            frames.append(files[i:i + frame_num + 1])
    return frames


def videvo_item(paths):
    """AA/datasets.py:157-170: cv2.imread + BGR2RGB is the RGB decode; toTensor255; channel concat."""
    imgs = [D.to_tensor255(load_rgb(p)) for p in paths]
    fn = len(paths) - 1
    return torch.cat(imgs[0:fn], dim=0), torch.cat(imgs[1:fn + 1], dim=0)


def videvo_wikiart_item(frames, wikiart, idx, resize, crop):
    """AA/datasets.py:183-185."""
    wikiart_idx = random.randint(0, len(wikiart) - 1)
    img1, img2 = videvo_item(frames[idx])
    return img1, img2, to_tensor_crop(load_rgb(wikiart[wikiart_idx][0]), resize, crop)


# ------------------------------------------------------------------------------- on-disk trees
IMAGE_SIZES = ((40, 70), (33, 29), (96, 128), (61, 45))  # (H, W); the fourth file of a class is greyscale


def write_image_tree(root, seed, classes=("a", "b"), per_class=4):
    """<root>/<class>/img_<k>.png, deterministic in `seed`: four sizes, every fourth file greyscale."""
    rng = np.random.default_rng(seed)
    for cls in classes:
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for k in range(per_class):
            H, W = IMAGE_SIZES[k % 4]
            a = rng.integers(0, 256, (H, W) if k % 4 == 3 else (H, W, 3), dtype=np.uint8)
            Image.fromarray(a).save(os.path.join(root, cls, f"img_{k:03d}.png"))


def write_videvo_tree(root, seed, hw, folders=2, frames=3):
    """<root>/frames/<folder>/<frame>.png of one size."""
    rng = np.random.default_rng(seed)
    for v in range(folders):
        d = os.path.join(root, "frames", f"{v:05d}")
        os.makedirs(d, exist_ok=True)
        for t in range(frames):
            Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(os.path.join(d, f"{t:05d}.png"))
