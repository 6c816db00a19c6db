"""Drop-in for AA/datasets.py: put this directory first on sys.path (the reference's trainers do
`from datasets import CocoWikiArt` / `VidevoWikiArt`).  Implementation: vst.adaattn.datasets (items made
on the GPU; iterate with CocoWikiArtLoader / VidevoWikiArtLoader instead of a DataLoader with workers)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vst.adaattn.datasets import (Coco, CocoWikiArt, CocoWikiArtLoader, ImageFolder, Sintel, Videvo,  # noqa: E402,F401
                                  VidevoWikiArt, VidevoWikiArtLoader, WikiArt, get_frames, toTensorCrop)
