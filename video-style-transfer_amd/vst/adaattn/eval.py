"""Drop-in for the LPIPS / SSIM / Gram / KL entries of AA/eval.py on HIP kernels (vst.metrics, vst.lpips).

`opt` is the reference's argparse namespace (`path0`, `path1`, `device`); `no_print=True` returns the
value instead of printing it, as in the reference.  Image files are read with cv2 when it is
importable and with Pillow otherwise.  Not carried: sifid (an InceptionV3 trunk whose weights are a
download) and nth_order_moment / uniformity / average_entropy (OpenCV's BGR2GRAY), DESIGN.md 4.11.
"""
import torch

from .. import ops
from ..lpips import LPIPS
from ..metrics import SSIMMetric, gram_distance, imread, kl_divergence, lpips_distance  # noqa: F401
from .vgg19 import VGG19


def _frame(path, device, bgr):
    """The file as a (1,3,H,W) fp32 tensor in [0,255]: planes in RGB order (bgr=True swaps cv2's
    BGR, `cv2_to_tensor(cv2.imread(p))`), or in the file's BGR order."""
    return ops.frames_to_tensor(torch.from_numpy(imread(path)).to(device).unsqueeze(0), bgr=bgr)


def lpips_loss(opt, no_print=False):
    """AA/eval.py:19-35.  The model is built once and kept on the function like the reference's; assign
    `lpips_loss.loss_fn` beforehand to evaluate with given weights.  The files go to the device as uint8
    frames; im2tensor and the ScalingLayer are one kernel pass there."""
    if not hasattr(lpips_loss, "loss_fn"):
        lpips_loss.loss_fn = LPIPS(net="vgg").to(opt.device)
    img0 = torch.from_numpy(imread(opt.path0)).to(opt.device).unsqueeze(0)
    img1 = torch.from_numpy(imread(opt.path1)).to(opt.device).unsqueeze(0)
    dist01 = lpips_distance(lpips_loss.loss_fn, img0, img1, bgr=True)
    if not no_print:
        print("Distance: %f" % dist01.item())
    else:
        return dist01.item()


def kl_loss(opt, no_print=False):
    """AA/eval.py:49-67."""
    KL = kl_divergence(torch.from_numpy(imread(opt.path0)).to(opt.device),
                       torch.from_numpy(imread(opt.path1)).to(opt.device))
    if not no_print:
        print("KL: %f" % KL)
    else:
        return KL


def gram_matrix(x):
    """AA/eval.py:70-75: F F^T / (H W)."""
    return ops.gram_matrix(x, per_hw=True)


def gram_loss(opt, no_print=False):
    """AA/eval.py:78-108.  The encoder is built once and kept on the function like the reference's;
    assign `gram_loss.vgg19` beforehand to evaluate with given weights."""
    if not hasattr(gram_loss, "vgg19"):
        gram_loss.vgg19 = VGG19().to(opt.device)
        gram_loss.vgg19.eval()
    loss = gram_distance(gram_loss.vgg19, _frame(opt.path0, opt.device, True), _frame(opt.path1, opt.device, True)).item()
    if not no_print:
        print("Gram Loss: %f" % loss)
    else:
        return loss


def ssim_loss(opt, no_print=False):
    """AA/eval.py:226-243 (the reference swaps the channels twice: the planes are in BGR order, which
    the channel mean does not see)."""
    if not hasattr(ssim_loss, "metric"):
        ssim_loss.metric = SSIMMetric(window_size=11, channel=3, sigma=1.5, reduction="mean").to(opt.device)
    ssim = ssim_loss.metric(_frame(opt.path0, opt.device, False), _frame(opt.path1, opt.device, False))
    if not no_print:
        print("SSIM: %f" % ssim.item())
    else:
        return ssim.item()
