"""Post-processing of predicted disparity maps on the device: the left-right consistency check of both
views and the background fill of the pixels it rejects (csrc/lrcheck.hip, ``costvolume.lr_check`` and
``costvolume.fill_background``).

The check is the one the ``-mask`` objectives train with (losses/loss.py:451-455: each view's map is
compared with the other view's map warped by ``imwrap_BCHW(.., fliplr=True)``); the right view is
predicted as ``deploy --flip`` does it, from the mirrored and swapped pair (stereo.py:142-150).

``predict_confidence`` answers the same question from ONE forward of a cost-volume network: the softmax its
head regresses from, read for its peak, the mass and the disparity of the window around it, and its entropy
(csrc/soft_argmin.hip ``dsm_disp_confidence_fwd``, ``costvolume.soft_argmin_confidence``).
"""
import torch

from . import costvolume as cv


def _first_map(out):
    """The full-resolution map of a forward's result: ``(loss, [disp, ...])`` of the factory's networks."""
    _, disps = out
    return disps[0]


def _is_lr_pair(out):
    """``gcnet_LR``'s return convention: a pair of tensors ``(oL, oR)``, each in its own camera's frame."""
    return isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(t) for t in out)


def predict_confidence(model, imL, imR, radius=4):
    """The disparity of one batch with the confidence its cost head carries, from ONE forward:
    ``costvolume.soft_argmin_confidence`` on what ``model.head_cost`` hands to the soft-argmin.

    ``model``: a cost-volume network of the factory (``psmnet``, ``gcnet``).  Eval mode, no gradients.
    Returns a dict of device tensors shaped like the network's first map ((B,H,W) for PSMNet, (B,1,H,W)
    for GCNet, cropped as its ``forward`` crops): ``disp`` (the map ``forward`` returns), ``peak`` (the
    regression over ``[d* - radius, d* + radius]`` around the arg-max bin, which does not average across
    the modes at a depth edge), ``pmax``, ``pwin`` (the probability mass of that window: near 1 where the
    distribution is unimodal) and ``entropy`` (nats).

    ``dispnet``, ``dispnetcorr`` and ``iresnet`` regress disparity directly -- there is no distribution
    over disparities to read a confidence from -- and are refused with a ``TypeError``."""
    if not callable(getattr(model, "head_cost", None)):
        raise TypeError("predict_confidence: %s regresses disparity directly and has no distribution over "
                        "disparities (no head_cost); confidence maps exist for the cost-volume networks "
                        "(psmnet, gcnet) only" % (getattr(model, "name", None) or type(model).__name__))
    model.eval()
    with torch.no_grad():
        cost, out_size, negate, align_corners, crop = model.head_cost(imL, imR)
        maps = cv.soft_argmin_confidence(cost, out_size, negate=negate, align_corners=align_corners, radius=radius)
    res = {}
    for name, t in zip(maps._fields, maps):
        if crop is not None:                     # GCNet: (B,1,H,W), cut as its forward cuts
            t = t.unsqueeze(1)[:, :, : crop[0], : crop[1]]
        res[name] = t
    return res


def _speckle_pair(speckle):
    """``speckle=(max_size, max_diff)`` of the entry points, checked: (int, float)."""
    try:
        max_size, max_diff = speckle
    except (TypeError, ValueError):
        raise ValueError("speckle is a pair (max_size, max_diff), got %r" % (speckle,))
    return max_size, max_diff


def remove_speckles(disp, max_size, max_diff, valid=None):
    """One map with its speckles removed: ``(out, keep)`` of ``costvolume.filter_speckles``.

    A speckle is a connected region of at most ``max_size`` pixels: 4-neighbours are joined where both are
    finite (and allowed by ``valid``, if given) and differ by at most ``max_diff`` in float32 -- OpenCV's
    ``filterSpeckles(img, 0, max_size, max_diff)``.  ``disp``: (B,1,H,W) or (B,H,W) float32 on the device;
    ``valid``: the same shape, ``torch.bool`` or ``torch.uint8``.  ``out`` is ``disp`` with the removed
    pixels (and those that were not finite or not valid) set to 0, ``keep`` the ``torch.bool`` mask of what
    stayed -- what ``fill_background`` and ``encode_disparity`` take as their mask.  No host read; capturable."""
    r = cv.filter_speckles(disp, max_size, max_diff, valid=valid, new_val=0.0, want=("out", "keep"))
    return r.out, r.keep


def left_right_check(model, imL, imR, threshold=1.0, fill=True, speckle=None):
    """Both views' disparity, consistency mask and weight, and the filled maps, of one batch.

    ``model``: a network of the factory (``forward(imL, imR) -> (_, [disp, ...])``, the first map (B,1,H,W)
    or PSMNet's (B,H,W)), run twice -- on the pair and on the mirrored, swapped pair
    ``(flip(imR), flip(imL))`` -- or one with ``gcnet_LR``'s convention ``forward(imL, imR) -> (oL, oR)``,
    run once.  Eval mode, no gradients, one ``amax_scope``.  ``imL`` / ``imR``: (B,3,H,W) on the device, as
    the network expects them (normalised or not).

    Returns a dict of device tensors shaped like the network's map:
      dispL, dispR      the two views' maps, each in its own camera's frame
      maskL, maskR      ``torch.bool``: |d - warped other view| < ``threshold`` and the sample inside
      weightL, weightR  the reference's soft weight (loss.py:393-404), factor 1
      filledL, filledR  with ``fill``: the maps with the rejected pixels filled from the background
    The right view is checked in the mirrored frame (loss.py:452) and its results are flipped back.

    ``speckle=(max_size, max_diff)``: after the check each view's map goes through
    ``costvolume.filter_speckles`` with ``valid=`` its check mask (the right view in the mirrored frame,
    like the rest), so that an island of at most ``max_size`` pixels that passed the check by accident
    does not decide the fill of its row.  The result gains
      keepL, keepR      ``torch.bool``: passed the check and lies in a region of more than ``max_size`` pixels
    and ``filledL`` / ``filledR`` are filled from ``keep``; ``maskL`` / ``maskR`` stay the check's own."""
    flip = lambda t: torch.flip(t, dims=[-1])
    want = ("weight", "mask")
    if speckle is not None:
        max_size, max_diff = _speckle_pair(speckle)
    model.eval()
    with torch.no_grad(), cv.amax_scope(imL.device):
        out = model(imL, imR)
        if _is_lr_pair(out):
            dL, dR = out[0].contiguous(), out[1].contiguous()
            dRm = flip(dR)
            left = cv.lr_check(dL, dR, mirrored=False, threshold=threshold, want=want)
        else:
            dL = _first_map(out).contiguous()
            dRm = _first_map(model(flip(imR), flip(imL))).contiguous()
            left = cv.lr_check(dL, dRm, mirrored=True, threshold=threshold, want=want)
        right = cv.lr_check(dRm, dL, mirrored=True, threshold=threshold, want=want)
        res = {"dispL": dL, "dispR": flip(dRm), "maskL": left.mask, "maskR": flip(right.mask),
               "weightL": left.weight, "weightR": flip(right.weight)}
        okL, okR = left.mask, right.mask
        if speckle is not None:
            okL = cv.filter_speckles(dL, max_size, max_diff, valid=left.mask, want=("keep",)).keep
            okR = cv.filter_speckles(dRm, max_size, max_diff, valid=right.mask, want=("keep",)).keep
            res["keepL"], res["keepR"] = okL, flip(okR)
        if fill:
            res["filledL"] = cv.fill_background(dL, okL)
            res["filledR"] = flip(cv.fill_background(dRm, okR))
    return res
