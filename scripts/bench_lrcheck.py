"""Left-right check and background fill of one batch: the stock torch sequence against the fused ops
(csrc/lrcheck.hip, costvolume.lr_check and costvolume.fill_background) in ONE process, alternating the two
so that both see the same machine.  The stock check is what the tree offers without the op: the flip grid
built with ``torch.linspace``, ``F.grid_sample``, the ``where`` chain of weight_common (loss.py:393-404),
the comparisons of the mask and the masked map.  The stock fill is a numpy-free torch restatement: the
nearest valid column on either side through ``cummax`` of the masked column index and two gathers, then the
same along the rows for the empty ones; it is checked against the fused result before it is timed.
Event-timed after warm-up; median and min..max of the repeats.  Also the HBM floor of each fused form:
check -- disp and other once, wrap, weight, masked and the byte mask written, 21 bytes per pixel; fill --
disp and the byte mask once, the result written, 9 bytes per pixel.  Prints one JSON line.

    python scripts/bench_lrcheck.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import costvolume as cv          # noqa: E402

COPY_BYTES_PER_S = 6.3e12                        # MI355X: what a device copy reaches


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def stock_check(disp, other, threshold=1.0, factor=1.0):
    bn, _, h, w = disp.shape
    row = torch.linspace(-1, 1, w, device=disp.device)
    col = torch.linspace(-1, 1, h, device=disp.device)
    gx = -(row.view(1, 1, w) - disp[:, 0] * 2.0 / (w - 1))
    grid = torch.stack([gx, col.view(1, h, 1).expand(bn, h, w)], -1)
    wrap = F.grid_sample(other, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    delta = (disp - wrap).abs() / factor
    weight = torch.where(delta < 1, torch.ones_like(delta),
                         torch.where(delta < 3, 1.0 - (delta - 1) * (0.99 / 2), torch.full_like(delta, 0.01)))
    ix = ((gx + 1) * w - 1) / 2
    mask = (delta < threshold) & ((ix >= 0) & (ix <= w - 1)).unsqueeze(1)
    return wrap, weight, mask, disp * mask


def _nearest(valid, dim):
    """Index of the nearest True at or before each position along ``dim`` (-1: none), and at or after."""
    n = valid.shape[dim]
    shape = [1] * valid.dim()
    shape[dim] = n
    ar = torch.arange(n, device=valid.device).view(shape).expand_as(valid)
    before = torch.where(valid, ar, -1).cummax(dim).values
    after = torch.where(valid.flip(dim), ar, -1).cummax(dim).values.flip(dim)
    return before, torch.where(after >= 0, n - 1 - after, after)


def stock_fill(disp, mask):
    d, m = disp[:, 0], mask[:, 0]
    d = torch.where(m, d, torch.zeros_like(d))                       # an invalid value is never used
    li, ri = _nearest(m, 2)
    lv, rv = d.gather(2, li.clamp(min=0)), d.gather(2, ri.clamp(min=0))
    rows = torch.where((li >= 0) & (ri >= 0), torch.minimum(lv, rv), torch.where(li >= 0, lv, rv))
    full = m.any(2)
    ui, di = _nearest(full, 1)
    w = d.shape[2]
    take = lambda idx: rows.gather(1, idx.clamp(min=0).unsqueeze(2).expand(-1, -1, w))
    uv, dv = take(ui), take(di)
    hasu, hasd = (ui >= 0).unsqueeze(2), (di >= 0).unsqueeze(2)
    out = torch.where(hasu & hasd, torch.minimum(uv, dv), torch.where(hasu, uv, torch.where(hasd, dv, torch.zeros_like(uv))))
    return out.unsqueeze(1)


def case(B, H, W, reps, warmup):
    g = torch.Generator().manual_seed(0)
    base = F.interpolate(torch.rand(B, 1, H // 32 + 2, W // 32 + 2, generator=g) * 60, size=(H, W), mode="bilinear",
                         align_corners=True)
    disp = base.clone()
    disp[:, :, H // 4: H // 2, W // 3: W // 2] += 20.0                 # an occluding box
    other = (base.flip(-1) + torch.rand(B, 1, H, W, generator=g)).contiguous()
    disp, other = disp.cuda(), other.cuda()
    mask = cv.lr_check(disp, other, want=("mask",)).mask
    mask[:, :, 5] = False                                              # one empty row per image
    fill_equal = bool(torch.equal(stock_fill(disp, mask), cv.fill_background(disp, mask)))
    s, f = stock_check(disp, other), cv.lr_check(disp, other)
    check_maxdiff = float((s[0] - f.wrap).abs().max())
    mask_diff = int((s[2] != f.mask).sum())

    runs = {"check_stock": lambda: stock_check(disp, other), "check_fused": lambda: cv.lr_check(disp, other),
            "fill_stock": lambda: stock_fill(disp, mask), "fill_fused": lambda: cv.fill_background(disp, mask)}
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():                                       # alternate
            ts[k].append(one(fn))
    px = float(B * H * W)
    out = {"shape": [B, H, W], "valid_fraction": float(mask.float().mean()), "fill_equal": fill_equal,
           "wrap_maxdiff_stock_fused": check_maxdiff, "mask_differs_stock_fused": mask_diff,
           "check_floor_ms": 21.0 * px / COPY_BYTES_PER_S * 1e3, "fill_floor_ms": 9.0 * px / COPY_BYTES_PER_S * 1e3}
    out.update({k: stats(v) for k, v in ts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lrcheck.py measures on the GPU: none found")
    print(json.dumps({"reps": a.reps, "cases": [case(1, 384, 1280, a.reps, a.warmup),
                                                case(4, 540, 960, a.reps, a.warmup)]}))


if __name__ == "__main__":
    main()
