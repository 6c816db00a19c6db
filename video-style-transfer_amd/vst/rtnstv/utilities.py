"""Drop-in MI355X implementation of the hot-path helpers of RT/utilities.py (video inference:
vst.rtnstv.inference, re-exported here)."""
import os

import numpy as np
import torch

from .. import ops
from ..metrics import TemporalError, imread, read_sintel_flow  # noqa: F401  (RT/utilities.py:113-152)
from ..reconet.utilities import flow_warp_mask  # noqa: F401  (RT/utilities.py:80-110, same arithmetic)
from .inference import Inference, cvframe_to_tensor  # noqa: F401  (RT/utilities.py:182-191, 296-332)


def warp(x, flo, padding_mode="zeros"):
    """RT/utilities.py:59-77 (grid normalised by max(W - 1, 1): the same as RC's for W, H > 1)."""
    if padding_mode != "zeros":
        raise ValueError("only padding_mode='zeros' is on the reference path")
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError("warp: frames must be at least 2x2")
    return ops.warp(x, flo)


def gram_matrix(y):
    """RT/utilities.py:155-160: F F^T / (H W) (not C H W as in ReCoNet / AdaAttN)."""
    return ops.gram_matrix(y, per_hw=True)


def vgg_normalize(batch):
    """RT/utilities.py:163-169: (batch / 255 - mean) / std, out of place."""
    return ops.VggNormalizeFn.apply(batch.float())


def list_files(directory):
    """RT/utilities.py:24-26."""
    return sorted(f.path for f in os.scandir(directory) if f.is_file())


def temporal_errors_sintel(model_class, model_path, scene, device="cuda", root="../datasets/MPI-Sintel-complete"):
    """RT/utilities.py:194-240: the scene's temporal error sqrt(mean over pairs of mean(mask *
    (styled0 - warp(styled1, flow))^2)).  `root` (the one addition to the reference's signature) is
    the MPI-Sintel-complete folder the reference hard-codes relative to its working directory.

    Each frame is stylised once (the reference runs every inner frame twice); frames go up as uint8
    and through the frame kernel, the .flo payload goes up as it lies in the file, and the masked
    squared warping error of every pair is accumulated on the device by `vst_temporal_error`: one host
    synchronisation per scene.  The reference's `toTensor` scales its uint8 0/1 mask by 1/255
    (torchvision's ToTensor on a uint8 array), so the mask values here are 1/255 as well."""
    frames_files = list_files(f"{root}/training/final/{scene}")
    mask_files = list_files(f"{root}/training/occlusions/{scene}")
    flow_files = list_files(f"{root}/training/flow/{scene}")

    model = model_class().to(device)
    model.load_state_dict(torch.load(model_path, weights_only=True), strict=True)
    model.eval()

    def styled(idx):
        frame = torch.from_numpy(imread(frames_files[idx])).to(device)
        with torch.no_grad():
            return model(ops.frames_to_tensor(frame.unsqueeze(0), bgr=True))

    te = TemporalError(power=2, convention="rt")
    styled_img1 = styled(0) if flow_files else None
    for idx in range(len(flow_files)):
        styled_img0, styled_img1 = styled_img1, styled(idx + 1)
        flow = torch.from_numpy(read_sintel_flow(flow_files[idx])).to(device)
        mask = (imread(mask_files[idx], gray=True) == 0).astype(np.float32) / np.float32(255)
        te.update(styled_img0, styled_img1, flow.unsqueeze(0), torch.from_numpy(mask).to(device).unsqueeze(0),
                  flow_hwc=True)
    return te.result()
