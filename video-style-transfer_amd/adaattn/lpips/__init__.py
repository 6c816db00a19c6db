"""Drop-in for the reference's `lpips` package (AA/lpips/): put the directory above first on sys.path (the
reference's scripts do `import lpips`).  Implementation: vst.lpips (HIP kernels; the AlexNet trunk --
the package's default, forward only -- and the VGG trunk).  The learned linear layers are looked for in
weights/v0.1/alex.pth and weights/v0.1/vgg.pth beside this file; the repository does not ship them --
copy the reference's lpips/weights/v0.1/alex.pth and vgg.pth there."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vst.lpips import (LPIPS, LPIPSTarget, NetLinLayer, PerceptualLoss, ScalingLayer, alexnet,  # noqa: E402,F401
                       im2tensor, load_image, normalize_tensor, spatial_average, upsample, vgg16)
