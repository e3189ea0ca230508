"""Restatement in numpy of what the reference's dataset does between the decoded files and the
transform (myDatasets_stereo/Dataset_stereo.py), written from its documented behaviour:

  :63-74    Crop_center_bottom: the last h_min rows, the w_min columns from (w - w_min) // 2
  :86-99    np.float32 of every plane, concatenated imL | imR [| dispL [| dispR]] on the channel axis
  :121-123  np.flip(img, axis=1): every channel mirrored, the views not swapped

``frame(planes, size_min, flip, disp_format)`` is the (H0, W0, C) fp32 frame that
``dsm_stereo_spatial_raw`` stands for; ``disp_format`` uses the numbers of include/dsmnet_hip.h
(0 float32 with non-finite -> 0 as img_rw.load_gray makes it, 1 uint16 / 256, 2 uint16, 3 uint8).
``frame_at`` takes an explicit window origin instead of the centre-bottom one.
"""
import numpy as np

F32 = np.float32
DISP_F32, DISP_U16_256, DISP_U16, DISP_U8 = 0, 1, 2, 3
DISP_DTYPE = {DISP_F32: np.float32, DISP_U16_256: np.uint16, DISP_U16: np.uint16, DISP_U8: np.uint8}


def crop_origin(hw, size_min):
    """(y0, x0) of Crop_center_bottom's window."""
    if size_min is None:
        return 0, 0
    h, w = hw
    assert size_min[0] <= h and size_min[1] <= w
    return h - size_min[0], (w - size_min[1]) // 2


def disp_values(plane, disp_format):
    plane = np.asarray(plane)
    assert plane.dtype == DISP_DTYPE[disp_format], (plane.dtype, disp_format)
    v = plane.astype(F32)
    if disp_format == DISP_F32:
        v[~np.isfinite(v)] = 0
    elif disp_format == DISP_U16_256:
        v = v / F32(256.0)
    return v


def frame_at(planes, origin, hw, flip=False, disp_format=DISP_U16):
    """``planes`` = [imL, imR (Hs, Ws, 3) uint8, then dispL [, dispR] (Hs, Ws)] -> (H0, W0, C) fp32."""
    (y0, x0), (H0, W0) = origin, hw
    parts = []
    for i, p in enumerate(planes):
        p = np.asarray(p)
        if i < 2:
            assert p.dtype == np.uint8 and p.ndim == 3 and p.shape[2] == 3
            v = p.astype(F32)
        else:
            v = disp_values(p, disp_format)[:, :, None]
        assert y0 >= 0 and x0 >= 0 and y0 + H0 <= p.shape[0] and x0 + W0 <= p.shape[1]
        parts.append(v[y0:y0 + H0, x0:x0 + W0])
    img = np.concatenate(parts, axis=2)
    if flip:
        img = np.flip(img, axis=1)
    return np.ascontiguousarray(img)


def frame(planes, size_min, flip=False, disp_format=DISP_U16):
    hw = planes[0].shape[:2]
    return frame_at(planes, crop_origin(hw, size_min), hw if size_min is None else tuple(size_min), flip, disp_format)


def getitem(planes, size_min, Train, disp_format=DISP_U16):
    """``Dataset_stereo.__getitem__`` up to the transform, drawing the flip from ``np.random`` as
    the reference does: only when Train and the channel count is even."""
    flip = bool(Train and len(planes) % 2 == 0 and np.random.rand() > 0.5)
    return frame(planes, size_min, flip, disp_format), flip
