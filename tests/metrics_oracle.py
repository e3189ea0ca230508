"""TEST INFRASTRUCTURE ONLY: float64 stock-torch restatement of the reference's evaluation metrics,
the yardstick of the fused csrc/metrics.hip path.

  sums      the 16 per-image sums of ``costvolume.stereo_metrics`` (slot table: DESIGN.md, the header)
  finish    the metrics of such sums: ``costvolume.stereo_metrics_finish`` restated
  evaluate / imwrap_pixel_errors / compute_errors     utils/evaluate.py:9-34, 36-44, 46-73

The warp is ``selfsup_oracle.imwrap_bchw`` (utils/imwrap.py:37-72: fp32 linspace base grid, then
``F.grid_sample`` in the inputs' dtype, align_corners=False).  evaluate.py:28-29 indexes a (B,C,H,W)
tensor with a (B,1,H,W) mask, which today's torch refuses; it is read as the broadcast it means: every
channel of the pixels whose warped channel sum is > 0.

Pinned against the reference's own lines (tests/golden/make_goldens_metrics.py, fixture
tests/golden/golden_metrics.npz).  Works on CPU and GPU tensors; computes in float64.
"""
import math

import torch

from tests import selfsup_oracle as SO

NSLOTS = 16
COUNT_SLOTS = (0, 2, 3, 8, 9, 10, 11, 13)
KEYS = ("d1", "epe", "abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3",
        "pixelerror", "pixelerror_elem")
EPS = 1e-6


def _as4(pred):
    return pred.unsqueeze(1) if pred.dim() == 3 else pred


def warp(imR, pred, delt, negate_warp=False):
    p = _as4(pred).to(torch.float64)
    return SO.imwrap_bchw(imR.to(torch.float64), -p if negate_warp else p, delt)


def sums(pred, gt=None, imL=None, imR=None, delt=0.0, negate_warp=False):
    """(B,16) float64: the slots of an absent input are 0."""
    pred = _as4(pred).to(torch.float64)
    B = pred.shape[0]
    out = torch.zeros(B, NSLOTS, dtype=torch.float64, device=pred.device)
    tot = lambda t: t.to(torch.float64).reshape(B, -1).sum(1)
    if gt is not None:
        gt = gt.to(torch.float64)
        m = gt > 0
        g = torch.where(m, gt, torch.ones_like(gt))          # holes never reach a sum: any finite stand-in
        diff = (g - pred).abs()
        rel = diff / g
        thresh = torch.maximum(g / (pred + EPS), pred / g)
        lg = (torch.log(g) - torch.log(pred + EPS)) ** 2
        zero = torch.zeros_like(g)
        w = lambda t: tot(torch.where(m, t.to(torch.float64), zero))
        out[:, 0] = tot(m)
        out[:, 1] = w(diff)
        out[:, 2] = w((diff <= 3) | (rel <= 0.05))
        out[:, 3] = w((diff >= 3) & (rel >= 0.05))
        out[:, 4] = w(diff ** 2)
        out[:, 5] = w(lg)
        out[:, 6] = w(rel)
        out[:, 7] = w(diff ** 2 / g)
        out[:, 8] = w(thresh < 1.25)
        out[:, 9] = w(thresh < 1.25 ** 2)
        out[:, 10] = w(thresh < 1.25 ** 3)
    if imL is not None:
        wimg = warp(imR, pred, delt, negate_warp)
        ad = (imL.to(torch.float64) - wimg).abs()
        elem = wimg > 0
        pix = wimg.sum(1, keepdim=True) > 0
        out[:, 11] = tot(elem)
        out[:, 12] = tot(ad * elem)
        out[:, 13] = tot(pix)
        out[:, 14] = tot(ad * pix)
        out[:, 15] = tot(ad)
    return out


def finish(s, image_shape=None, per_image=False):
    """dict of float64 tensors; ``image_shape`` = (C, H, W) of the images (pixelerror needs it)."""
    nimg = s.shape[0]
    s = s if per_image else s.sum(0)
    c = [s[..., k] for k in range(NSLOTS)]
    n = c[0]
    out = {"d1": 100 - 100.0 * c[2] / n, "epe": c[1] / n, "abs_rel": c[6] / n, "sq_rel": c[7] / n,
           "rmse": (c[4] / n).sqrt(), "rmse_log": (c[5] / n).sqrt(), "d1_kitti": 100.0 * c[3] / n,
           "a1": c[8] / n, "a2": c[9] / n, "a3": c[10] / n, "pixelerror_elem": 255.0 * c[12] / c[11]}
    if image_shape is None:
        out["pixelerror"] = torch.full_like(n, math.nan)
    else:
        C, H, W = image_shape
        every = (1 if per_image else nimg) * C * H * W
        some = c[13] > 0
        out["pixelerror"] = 255.0 * torch.where(some, c[14] / (C * c[13].clamp(min=1)), c[15] / every)
    return out


# ----------------------------------------------------------------------------
# Test inputs.  The counted slots are step functions of the inputs, so a float32 implementation can
# only be held to exact counts on inputs that stay away from every step: no counted threshold may be
# within MARGIN of being crossed (checked in float64).
# ----------------------------------------------------------------------------
MARGIN = 1e-3


def _smooth(g, B, C, H, W, lo, hi, cell):
    coarse = torch.rand(B, C, max(2, H // cell + 2), max(2, W // cell + 2), generator=g, dtype=torch.float64)
    return lo + (hi - lo) * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)


def offenders(pred, gt=None, warp_signs=(1.0, -1.0)):
    """(near a ground-truth threshold, near the warp's in-bounds edge): boolean (B,1,H,W) maps."""
    p = _as4(pred).to(torch.float64)
    W = p.shape[-1]
    near_gt = torch.zeros_like(p, dtype=torch.bool)
    if gt is not None:
        g = gt.to(torch.float64)
        m = g > 0
        g = torch.where(m, g, torch.ones_like(g))
        diff = (g - p).abs()
        thresh = torch.maximum(g / (p + EPS), p / g)
        near_gt = ((diff - 3).abs() < MARGIN) | ((diff / g - 0.05).abs() < MARGIN)
        for k in (1, 2, 3):
            near_gt |= (thresh - 1.25 ** k).abs() < MARGIN
        near_gt &= m
    near_warp = torch.zeros_like(near_gt)
    x = torch.arange(W, dtype=torch.float64, device=p.device).view(1, 1, 1, W)
    for sgn in warp_signs:
        ix = (x - sgn * p) * W / (W - 1.0) - 0.5       # grid_sample's source column, align_corners=False
        near_warp |= ((ix + 1).abs() < MARGIN) | ((ix - W).abs() < MARGIN)
    return near_gt, near_warp


def precondition_holds(pred, gt=None, warp_signs=(1.0, -1.0)):
    a, b = offenders(pred, gt, warp_signs)
    return not bool(a.any()) and not bool(b.any())


def condition(pred, gt=None, warp_signs=(1.0, -1.0)):
    """Move the offending predictions (never mask them): a disparity near the warp's edge is shifted by
    0.25, a prediction near a ground-truth threshold is set to gt.  Returns (pred, pixels moved)."""
    pred = pred.clone()
    moved = torch.zeros_like(_as4(pred), dtype=torch.bool)
    for _ in range(10):
        near_gt, near_warp = offenders(pred, gt, warp_signs)
        if not bool(near_gt.any()) and not bool(near_warp.any()):
            return pred, int(moved.sum())
        moved |= near_gt | near_warp
        v = _as4(pred)
        v[near_warp] += 0.25
        if gt is not None:
            near_gt, _ = offenders(pred, gt, warp_signs)
            v[near_gt] = gt[near_gt]
    raise AssertionError("could not move the inputs away from the thresholds")


def make_inputs(seed, B, C, H, W, dlo=1.0, dhi=60.0, holes=0.3):
    """(imgs uint8 (B,2C,H,W): left | right, gt float32 (B,1,H,W) with holes = 0, pred float32 (B,1,H,W)):
    independent smooth-noise images, smooth ground truth in [dlo, dhi], predictions gt * (0.5 .. 2.4) +- 0.2,
    conditioned for both warp signs."""
    g = torch.Generator().manual_seed(seed)
    imgs = _smooth(g, B, 2 * C, H, W, 0, 255, 6) + 12 * torch.rand(B, 2 * C, H, W, generator=g, dtype=torch.float64)
    imgs = imgs.clamp(0, 255).round().to(torch.uint8)
    full = _smooth(g, B, 1, H, W, dlo, dhi, 4)
    factor = _smooth(g, B, 1, H, W, 0.5, 2.4, 4)
    pred = (full * factor + 0.2 * (2 * torch.rand(B, 1, H, W, generator=g, dtype=torch.float64) - 1)).float()
    gt = torch.where(torch.rand(B, 1, H, W, generator=g) < holes, torch.zeros(()), full.float())
    pred, _ = condition(pred, gt)
    return imgs, gt, pred


def images_of(imgs):
    """float32 (imL, imR) in [0,1] of ``make_inputs``' uint8 batch."""
    x = imgs.float() / 255.0
    C = x.shape[1] // 2
    return x[:, :C].contiguous(), x[:, C:].contiguous()


def compute_errors(gt, pred):
    """evaluate.py:46-73: (abs_rel, sq_rel, rmse, rmse_log, d1, a1, a2, a3) as floats."""
    f = finish(sums(torch.as_tensor(pred), torch.as_tensor(gt)))
    return tuple(float(f[k]) for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3"))


def imwrap_pixel_errors(imL, imR, dispL, delt):
    """evaluate.py:36-44."""
    s = sums(torch.as_tensor(dispL), None, torch.as_tensor(imL), torch.as_tensor(imR), delt, True)
    return float(finish(s)["pixelerror_elem"])


def evaluate(imL, imR, dispL, dispL_gt=None, delt=0.0):
    """evaluate.py:9-34: (d1, epe, pixelerror); d1 = epe = -1 without ground truth."""
    imL = torch.as_tensor(imL)
    s = sums(torch.as_tensor(dispL), None if dispL_gt is None else torch.as_tensor(dispL_gt), imL,
             torch.as_tensor(imR), delt, True)
    f = finish(s, tuple(imL.shape[1:]))
    if dispL_gt is None:
        return -1, -1, float(f["pixelerror"])
    return float(f["d1"]), float(f["epe"]), float(f["pixelerror"])
