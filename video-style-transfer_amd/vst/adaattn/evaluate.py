"""The Sintel temporal-consistency experiment of AA/exps_sintel.py:66-110 on the MI355X."""
from ..metrics import TemporalError
from . import inference


def sintel_temporal_error(model, vgg, style, pairs, activation="cosine"):
    """The loop body of AA/exps_sintel.py:66-107 over `pairs`, an iterable of (c1, c2, flow, mask):
    c1, c2 (B,3,H,W) fp32 RGB in [0,255], flow (B,2,H,W), mask (B,H,W), all on the device (the
    reference's loader yields B = 1).  Returns sqrt(sum of the pairs' masked mean absolute warping
    errors) / pairs, the reference's own formula (`TemporalError`, convention "aa").

    The style (Nk,3,H,W) is encoded once (`inference.encode_style`); both frames of a pair run
    through `inference.stylize`; clamp(0,255)/255, the warp of cs1, the masked absolute difference
    from cs2 and the sum are one kernel pass accumulated on the device -- one host synchronisation
    for the whole scene.  Where the flows come from (ground-truth .flo files and occlusion maps, or
    `flow_warp_mask` of two estimated flows) is the caller's business."""
    model = inference.load_model(model, activation, style.device)
    vgg = inference.load_vgg(vgg, style.device)
    state = inference.encode_style(vgg, model, style)
    te = TemporalError(power=1, clamp_unit=True, convention="aa")
    for c1, c2, flow, mask in pairs:
        cs1 = inference.stylize(vgg, model, state, c1)
        cs2 = inference.stylize(vgg, model, state, c2)
        te.update(cs2, cs1, flow, mask)
    return te.result()
