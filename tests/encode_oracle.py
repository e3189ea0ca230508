"""fp32 numpy restatement, operation for operation, of the rules of ``dsm_disp_encode``
(include/dsmnet_hip.h, csrc/encode.hip).  Every operation there is a correctly rounded fp32 or an
integer one, so the kernel's bytes equal these exactly."""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ERR_EDGES = [F(2.0 ** k) for k in range(-4, 5)]                 # 1/16 ... 16: upper edge of bins 0..8
ERR_COLOURS = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248],
                        [254, 224, 144], [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], np.uint8)


def header_lut():
    """The committed table of csrc/viridis_lut.hpp as a (256,3) uint8 array."""
    text = open(os.path.join(ROOT, "dsmnet_amd", "csrc", "viridis_lut.hpp")).read()
    body = re.search(r"dsm_viridis_lut\[[^\]]*\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    vals = [int(v) for v in re.findall(r"\d+", body)]
    assert len(vals) == 768 and max(vals) <= 255
    return np.array(vals, np.uint8).reshape(256, 3)


def _window(a, window, flip):
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim == 4:
        a = a[:, 0]
    if window is not None:
        y0, x0, h, w = window
        a = a[:, y0:y0 + h, x0:x0 + w]
    return a[:, :, ::-1] if flip else a


def _valid(d, mask):
    ok = np.isfinite(d)
    return ok if mask is None else ok & (mask != 0)


def u16(d, mask=None):
    with np.errstate(all="ignore"):
        q = np.clip(np.rint(d * F(256.0)), F(1.0), F(65535.0))
    return np.where(_valid(d, mask), q, F(0)).astype(np.uint16)


def u8(d, mask=None):
    with np.errstate(all="ignore"):
        q = np.clip(np.rint(d), F(0.0), F(255.0))
    carries = ~np.isnan(d) if mask is None else ~np.isnan(d) & (mask != 0)
    return np.where(carries, q, F(0)).astype(np.uint8)


def auto_range(d, mask=None):
    """Per image (lo, hi) over the finite, unmasked pixels; (+inf, -inf) when there is none."""
    out = []
    for i in range(d.shape[0]):
        v = d[i][_valid(d[i], None if mask is None else mask[i])]
        out.append((F(v.min()), F(v.max())) if v.size else (F(np.inf), F(-np.inf)))
    return out


def rgb(d, mask=None, vrange=None, lut=None):
    lut = header_lut() if lut is None else lut
    ranges = auto_range(d, mask) if vrange is None else [(F(vrange[0]), F(vrange[1]))] * d.shape[0]
    out = np.zeros(d.shape + (3,), np.uint8)
    for i, (lo, hi) in enumerate(ranges):
        with np.errstate(all="ignore"):
            v = ((d[i] - lo) / (hi - lo)) * F(256.0)
            assert v.dtype == np.float32
            idx = np.where(v >= F(256.0), 255, np.trunc(np.where(v >= F(0.0), v, F(0.0))).astype(np.int64))
        idx = np.where((hi == lo) | ~(v >= F(0.0)), 0, idx).clip(0, 255)
        out[i] = np.where(_valid(d[i], None if mask is None else mask[i])[..., None], lut[idx], 0)
    return out


def err(d, gt, mask=None):
    with np.errstate(all="ignore"):
        scored = np.isfinite(gt) & (gt > F(0.0))
        if mask is not None:
            scored &= mask != 0
        e = np.abs(gt - d)
        n = np.fmin(e / F(3.0), (e / gt) / F(0.05))
        assert n.dtype == np.float32
        bins = np.full(d.shape, 9, np.int64)
        for k in range(8, -1, -1):
            bins = np.where(n < ERR_EDGES[k], k, bins)
    return np.where(scored[..., None], ERR_COLOURS[bins], 0).astype(np.uint8)


def encode(disp, gt=None, mask=None, window=None, flip=False, want=("u16",), vrange=None):
    """The dict ``costvolume.encode_disparity`` returns, as numpy arrays."""
    d = np.ascontiguousarray(_window(disp, window, flip), dtype=np.float32)
    g = None if gt is None else np.ascontiguousarray(_window(gt, window, flip), dtype=np.float32)
    m = None if mask is None else np.ascontiguousarray(_window(mask, window, flip)).astype(np.uint8)
    out = {}
    for name in want:
        if name == "u16":
            out[name] = u16(d, m)
        elif name == "u8":
            out[name] = u8(d, m)
        elif name == "rgb":
            out[name] = rgb(d, m, vrange)
        elif name == "err":
            out[name] = err(d, g, m)
        else:
            raise ValueError(name)
    return out
