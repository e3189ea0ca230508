"""Restatements of the reference's spatial transform (myTransforms/aug_spatial.py:7-88) and
ToTensor_numpy (aug_color.py:15-26) in numpy, written from their documented behaviour.

``resize_linear(img, (w1, h1))``: cv2's linear resize of an fp32 HWC (or HW) array, stated as a
rule: tap coordinates in float64 cast to float32, clamped at the borders, fp32 horizontal pass
``S[sx]*(1-fx) + S[sx+1]*fx`` then the same form vertically, no antialiasing.  That this rule
equals the cv2 binary has not been measured (cv2 is not available where the fixture is written).

``restate(x, record, out_hw, to_tensor_channels)``: the contract of ``costvolume.stereo_spatial``
/ ``dsm_stereo_spatial`` for one (H0, W0, C) frame and one explicit record, fp32 in the order the
kernel is specified in.  ``tap_bound`` gives the per-pixel magnitude M of the GPU tests' bound.

``lighting_normalize_torch``: the colour steps of the reference's Stereo_train (Lighting, group 2,
shared draw; Normalize_Imagenet) with stock torch ops on the batch's device.
"""
import numpy as np
import torch

from tests import color_oracle as CO

F32 = np.float32


def _taps(n_out, n_in):
    scale = 1.0 / (float(n_out) / n_in)
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f)
    f = (f - s).astype(F32)
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= n_in - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), f


def resize_linear(img, size, *stray):
    """``cv2.resize(img, (w1, h1))`` with the default (linear) interpolation, by the rule above.
    Further positional arguments are accepted and ignored (the reference passes the interpolation
    flag where ``dst`` goes)."""
    img = np.asarray(img)
    assert img.dtype == F32, img.dtype
    w1, h1 = size
    h, w = img.shape[:2]
    flat = img.reshape(h, w, -1)
    sx, sx1, fx = _taps(w1, w)
    sy, sy1, fy = _taps(h1, h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    rows = flat[:, sx] * (F32(1) - fx) + flat[:, sx1] * fx              # (h, w1, C)
    out = rows[sy] * (F32(1) - fy) + rows[sy1] * fy                     # (h1, w1, C)
    assert out.dtype == F32
    return out.reshape((h1, w1) + img.shape[2:])


def _shifted(x, shift):
    """The frame after shift_stereo (aug_spatial.py:17-41), as a new (H0, W0 - shift, C) array."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 3
    H0, W0, C = x.shape
    out = x[:, :W0 - shift].copy()
    out[:, :, 3:6] = x[:, shift:, 3:6]
    if C >= 8:
        out[:, :, 7] = x[:, shift:, 7]
    for c in range(6, C):
        mask = out[:, :, c] != 0
        out[:, :, c][mask] += F32(shift)
    return out


def restate(x, record, out_hw, to_tensor_channels=6):
    """(C, h, w) fp32 output of one (H0, W0, C) frame for ``record`` = (shift, ws, hs, w, h,
    resize, scale_rand, scale_x, scale_y).  scale_x / scale_y are implied by the window and the
    output size (the planner's 1/(w1/w)) and are not read."""
    shift, ws, hs, w, h, resize, scale_rand = record[:7]
    win = _shifted(x, shift)[hs:hs + h, ws:ws + w]
    assert win.shape[:2] == (h, w), "window outside the shifted frame"
    if resize:
        win = resize_linear(win, (out_hw[1], out_hw[0]))
        win[:, :, 6:] *= F32(scale_rand)
    else:
        assert (h, w) == tuple(out_hw)
    out = np.ascontiguousarray(win.transpose(2, 0, 1))
    out[:to_tensor_channels] /= F32(255.0)
    return out


def tap_bound(x, record, out_hw, to_tensor_channels=6):
    """(C, h, w): the largest magnitude among each output pixel's four taps, in output units."""
    shift, ws, hs, w, h, resize, scale_rand = record[:7]
    win = np.abs(_shifted(x, shift)[hs:hs + h, ws:ws + w]).astype(np.float64)
    if resize:
        sx, sx1, _ = _taps(out_hw[1], w)
        sy, sy1, _ = _taps(out_hw[0], h)
        win = np.maximum(np.maximum(win[sy][:, sx], win[sy][:, sx1]),
                         np.maximum(win[sy1][:, sx], win[sy1][:, sx1]))
        win[:, :, 6:] *= abs(float(F32(scale_rand)))
    out = win.transpose(2, 0, 1).copy()
    out[:to_tensor_channels] /= 255.0
    return out


def restate_batch(x, records, out_hw, to_tensor_channels=6):
    return np.stack([restate(x[b], records[b], out_hw, to_tensor_channels) for b in range(len(records))])


def tap_bound_batch(x, records, out_hw, to_tensor_channels=6):
    return np.stack([tap_bound(x[b], records[b], out_hw, to_tensor_channels) for b in range(len(records))])


def lighting_normalize_torch(batch, alphastd=0.1):
    """In place on ``batch`` (B, C >= 6, H, W): Lighting(alphastd, group=2, same_group=True) and
    Normalize_Imagenet(group=2), image by image, drawing one 3-element ``normal_`` per image on
    the batch's device (aug_color.py:28-45, 66-101)."""
    ev = torch.tensor(CO.EIGVEC, dtype=batch.dtype, device=batch.device)
    el = torch.tensor(CO.EIGVAL, dtype=batch.dtype, device=batch.device)
    for img in batch:
        alpha = img.new_empty(3).normal_(0, alphastd)
        rgb = (ev * alpha.view(1, 3) * el.view(1, 3)).sum(1)
        for g in range(2):
            img[3 * g:3 * g + 3] = (img[3 * g:3 * g + 3] + rgb.view(3, 1, 1)).clamp(0, 1)
            for c in range(3):
                img[3 * g + c].sub_(CO.MEAN[c]).div_(CO.STD[c])
    return batch
