"""The reference's evaluation helpers (utils/evaluate.py) on the fused metrics op.

    evaluate(imL, imR, dispL, dispL_gt=None) -> (d1, epe, pixelerror)         evaluate.py:9-34
    imwrap_pixel_errors(imL, imR, dispL) -> pixelerror over elements           evaluate.py:36-44
    compute_errors(gt, pred) -> (abs_rel, sq_rel, rmse, rmse_log, d1, a1, a2, a3)   evaluate.py:46-73

Arguments are numpy arrays or tensors, images (B,C,H,W) and maps (B,1,H,W) (or (B,H,W)); they are
moved to the device as float32, go through ``costvolume.stereo_metrics`` (two launches) and
``stereo_metrics_finish`` over the whole batch, and come back as Python floats -- one host read
per call, where the reference spends one per number.  There is no CPU path.

``evaluate`` and ``imwrap_pixel_errors`` keep the reference's ``imwrap_BCHW(imR, -dispL)``
(evaluate.py:26,40; the training losses warp by ``+disp``: use ``stereo_metrics`` directly, or
``train.evaluate_step``, for that sign).  Their ``> 0`` masks mean "inside the right image" only
when the images are NON-NEGATIVE -- raw [0,1] or [0,255] pixels, not ImageNet-normalised ones:
a warped sample is exactly 0 outside and ``(pixel + delt) * weight > 0`` inside.
evaluate.py:28-29 indexes (B,C,H,W) with a (B,1,H,W) mask, which current torch refuses; it is read
as the broadcast it means (every channel of the pixels whose warped channel sum is > 0).
"""
import numpy as np
import torch

from . import costvolume as cv


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("dsmnet_amd.evaluate: the metrics run on the MI355X through libdsmnet_hip.so only "
                           "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(x, device):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.as_tensor(x)
    return t.to(device=device, dtype=torch.float32)


def _finish(pred, gt, imL, imR, delt, device):
    dev = _device(device)
    sums = cv.stereo_metrics(_to_device(pred, dev), _to_device(gt, dev), _to_device(imL, dev),
                             _to_device(imR, dev), delt=delt, negate_warp=True)
    out = cv.stereo_metrics_finish(sums)
    host = torch.stack([out[k] for k in cv.METRIC_KEYS]).cpu().tolist()      # the call's one host read
    return dict(zip(cv.METRIC_KEYS, host))


def evaluate(imL, imR, dispL, dispL_gt=None, delt=None, device=None):
    """(d1, epe, pixelerror): D1 % and end-point error over ``dispL_gt > 0`` (-1, -1 without ground
    truth, as evaluate.py:12) and 255 * the mean ``|imL - imwrap_BCHW(imR, -dispL)|`` over the pixels
    warped from inside the right image (over every pixel when there is none).  ``delt``: the warp's
    epsilon; None draws it as the reference does."""
    m = _finish(dispL, dispL_gt, imL, imR, delt, device)
    if dispL_gt is None:
        return -1, -1, m["pixelerror"]
    return m["d1"], m["epe"], m["pixelerror"]


def imwrap_pixel_errors(imL, imR, dispL, delt=None, device=None):
    """255 * the mean ``|imL - w|`` over the ELEMENTS with ``w = imwrap_BCHW(imR, -dispL) > 0``
    (NaN when there is none, as the reference's empty mean)."""
    return _finish(dispL, None, imL, imR, delt, device)["pixelerror_elem"]


def compute_errors(gt, pred, device=None):
    """The KITTI set over ``gt > 0`` in the reference's order: abs_rel, sq_rel, rmse, rmse_log,
    d1 (bad: error >= 3 px AND >= 5 %), a1, a2, a3.  NaN without a valid pixel, as numpy gives."""
    m = _finish(pred, gt, None, None, None, device)
    return tuple(m[k] for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3"))
