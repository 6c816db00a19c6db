"""Drop-in for RT/utilities.py: put this directory first on sys.path (the reference's train.py does
`from utilities import ...`).  Implementation: vst.rtnstv.utilities (HIP kernels)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vst.rtnstv.utilities import *  # noqa: E402,F401,F403
from vst.rtnstv.utilities import (Inference, cvframe_to_tensor, flow_warp_mask, gram_matrix,  # noqa: E402,F401
                                   list_files, read_sintel_flow, temporal_errors_sintel, vgg_normalize, warp)
