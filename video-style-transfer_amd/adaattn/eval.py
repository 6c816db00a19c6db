"""Drop-in for AA/eval.py's LPIPS / SSIM / Gram / KL entries: put this directory first on sys.path (the
reference's experiment scripts do `from eval import ...`).  Implementation: vst.adaattn.eval (HIP kernels)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vst.adaattn.eval import SSIMMetric, gram_loss, gram_matrix, kl_loss, lpips_loss, ssim_loss  # noqa: E402,F401
