"""float64 numpy restatement of the head-confidence op (csrc/soft_argmin.hip: dsm_disp_confidence_fwd).

Let ``v_d`` (d = 0..D-1) be the sign times the trilinearly interpolated cost at a pixel (torch's
``area_pixel_compute_source_index`` arithmetic) and ``p = softmax(v)``.  For an integer radius r >= 0:

    disp     sum_d d p_d
    pmax     p_{d*},  d* the smallest d with v_d = max v
    pwin     sum_{d in Wn} p_d,  Wn = [max(0, d* - r), min(D - 1, d* + r)]
    peak     sum_{d in Wn} d p_d / pwin
    entropy  -sum_d p_d ln p_d  (nats, 0 ln 0 = 0)

The interpolation is explicit, axis by axis, and takes the plane's value itself wherever the two
interpolation indices coincide (the clamped top end): ``w0 P + w1 P`` would let rounding decide between
two bins that are equal mathematically, and ``d*`` with it.  The bottom clamp has w1 = 0 and is exact as it is.
"""
import numpy as np
import torch

MAPS = ("disp", "peak", "pmax", "pwin", "entropy")

# (cost shape, out size or None, negate, align_corners, seed): the smallest shapes that reach each branch
CASES = {
    "up4_empty_seg": ((2, 6, 3, 18), (24, 12, 70), False, False, 100),     # x4; a lane without planes; W tail; B > 1
    "up4_full": ((1, 8, 2, 5), (32, 8, 20), False, False, 101),            # x4, full segments
    "up4_d192": ((1, 48, 4, 18), (192, 16, 70), False, False, 102),        # x4 at the model's D
    "interp_align": ((2, 5, 4, 9), (13, 9, 23), False, True, 103),         # interpolating form
    "interp_ratio": ((1, 5, 3, 6), (12, 7, 15), False, False, 104),        # non-integer ratio
    "x4_small_dc": ((1, 2, 3, 5), (8, 6, 10), False, False, 105),          # D = 4 Dc but Dc < 4
    "gc_ds4": ((2, 10, 5, 70), None, True, False, 106),                    # GCNet form, DSPLIT 4
    "gc_ds2": ((1, 6, 3, 17), None, True, False, 107),                     # DSPLIT 2
    "gc_ds1": ((1, 3, 2, 9), None, True, False, 108),                      # DSPLIT 1
}


def case_cost(name):
    """The seeded ``4 * randn`` cost of a case, float32 on the CPU."""
    shape, _, _, _, seed = CASES[name]
    return 4.0 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def source_index(out_size, in_size, align):
    """(i0, i1, w0, w1) of every output index: area_pixel_compute_source_index + guard_index_and_lambda."""
    o = np.arange(out_size, dtype=np.float64)
    if in_size == out_size:
        i = o.astype(np.int64)
        return i, i, np.ones(out_size), np.zeros(out_size)
    if align:
        scale = (in_size - 1) / (out_size - 1) if out_size > 1 else 0.0
        src = scale * o
    else:
        src = np.maximum(in_size / out_size * (o + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    w1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, 1.0 - w1, w1


def interp_axis(a, axis, out_size, align):
    i0, i1, w0, w1 = source_index(out_size, a.shape[axis], align)
    shape = [1] * a.ndim
    shape[axis] = out_size
    a0, a1 = np.take(a, i0, axis=axis), np.take(a, i1, axis=axis)
    v = w0.reshape(shape) * a0 + w1.reshape(shape) * a1
    return np.where((i0 == i1).reshape(shape), a0, v)


def fine_values(cost, out_size=None, negate=False, align_corners=False):
    """(B, D, H, W) float64: sign * trilinear(cost)."""
    c = np.asarray(cost.detach().cpu().numpy() if torch.is_tensor(cost) else cost, dtype=np.float64)
    if c.ndim == 5:
        c = c[:, 0]
    if out_size is not None:
        D, H, W = out_size
        c = interp_axis(c, 3, W, align_corners)
        c = interp_axis(c, 2, H, align_corners)
        c = interp_axis(c, 1, D, align_corners)
    return -c if negate else c


def from_values(v, radius):
    """The five maps, ``dstar`` and ``gap`` (largest minus second-largest DISTINCT fine value; inf when all
    are equal) from (B, D, H, W) values."""
    D = v.shape[1]
    m = v.max(axis=1, keepdims=True)
    e = np.exp(v - m)
    p = e / e.sum(axis=1, keepdims=True)
    d = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    dstar = np.argmax(v, axis=1)                                   # the first maximum
    lo = np.maximum(dstar - radius, 0)[:, None]
    hi = np.minimum(dstar + radius, D - 1)[:, None]
    win = (d >= lo) & (d <= hi)
    pwin = (p * win).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    below = np.where(v < m, v, -np.inf).max(axis=1)
    return {"disp": (d * p).sum(axis=1), "peak": (d * p * win).sum(axis=1) / pwin,
            "pmax": np.take_along_axis(p, dstar[:, None], axis=1)[:, 0], "pwin": pwin,
            "entropy": -plogp.sum(axis=1), "dstar": dstar, "gap": m[:, 0] - below}


def heads(cost, out_size=None, negate=False, align_corners=False, radius=4):
    return from_values(fine_values(cost, out_size, negate, align_corners), radius)


def torch_heads(cost, out_size=None, negate=False, align_corners=False, radius=4, dtype=torch.float32,
                dstar=None):
    """The yardstick: ``F.interpolate`` -> ``softmax`` -> the sums of the definition, in ``dtype`` on the CPU.
    Returns the five maps as float64 numpy arrays plus the (B, D, H, W) values.  ``dstar``: the arg-max
    to centre the window on (the oracle's, when float32 error is measured: ``F.interpolate`` does not keep
    the exact end ties, and a window one bin off would inflate the yardstick's error, not sharpen it)."""
    import torch.nn.functional as F
    c = cost.detach().cpu().to(dtype)
    if c.dim() == 4:
        c = c.unsqueeze(1)
    if out_size is not None:
        c = F.interpolate(c, size=tuple(out_size), mode="trilinear", align_corners=align_corners)
    v = (-c if negate else c)[:, 0]
    D = v.shape[1]
    p = torch.softmax(v, dim=1)
    d = torch.arange(D, dtype=dtype).view(1, D, 1, 1)
    dstar = v.argmax(dim=1, keepdim=True) if dstar is None else torch.as_tensor(dstar).unsqueeze(1)
    win =((d >= (dstar - radius).clamp_min(0)) & (d <= (dstar + radius).clamp_max(D - 1))).to(dtype)
    pwin = (p * win).sum(1)
    plogp = torch.where(p > 0, p * torch.log(p.clamp_min(torch.finfo(dtype).tiny)), torch.zeros_like(p))
    out = {"disp": (d * p).sum(1), "peak": (d * p * win).sum(1) / pwin, "pmax": p.gather(1, dstar)[:, 0],
           "pwin": pwin, "entropy": -plogp.sum(1)}
    out = {k: t.double().numpy() for k, t in out.items()}
    out["values"] = v.double().numpy()
    return out
