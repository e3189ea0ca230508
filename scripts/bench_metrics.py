"""Evaluation metrics of one batch: the stock torch sequence against the fused op
(csrc/metrics.hip, costvolume.stereo_metrics + stereo_metrics_finish) in ONE process, alternating the
two so that both see the same machine.  The stock sequence is what the tree offers without the op:
``train.accuracy`` (D1, EPE), a torch restatement of utils/evaluate.py compute_errors (boolean gather,
one mean per metric) and the photometric errors through ``F.grid_sample`` and masks
(utils/imwrap.py:37-72, evaluate.py:26-32, 40-44), all in fp32 on the device, results left there.
Event-timed after warm-up; median and min..max of the repeats.  Also the HBM floor of the fused form:
pred, gt, imL and imR once, (2 + 2C) * 4 bytes per pixel.  Prints one JSON line.

    python scripts/bench_metrics.py [--reps 30] [--warmup 5]
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
from dsmnet_amd import train                     # noqa: E402

HBM_BYTES_PER_S = 8.0e12                         # MI355X peak
DELT = 6.25e-05


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


def stock_compute_errors(gt, pred):
    mask = gt > 0
    gt, pred = gt[mask], pred[mask]
    diff = (gt - pred).abs()
    thresh = torch.maximum(gt / (pred + 1e-6), pred / gt)
    a1, a2, a3 = ((thresh < 1.25 ** k).float().mean() for k in (1, 2, 3))
    d1 = 100.0 * ((diff >= 3) & (diff / gt >= 0.05)).sum() / mask.sum()
    rmse = (diff ** 2).mean().sqrt()
    rmse_log = ((gt.log() - (pred + 1e-6).log()) ** 2).mean().sqrt()
    return (diff / gt).mean(), (diff ** 2 / gt).mean(), rmse, rmse_log, d1, a1, a2, a3


def stock_warp(im_src, disp, delt):
    bn, _, h, w = disp.shape
    row = torch.linspace(-1, 1, w, device=disp.device)
    col = torch.linspace(-1, 1, h, device=disp.device)
    gx = row.view(1, 1, w) - disp[:, 0] * 2.0 / (w - 1)
    grid = torch.stack([gx, col.view(1, h, 1).expand(bn, h, w)], -1)
    return F.grid_sample(im_src + delt, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def stock_photometric(imL, imR, pred, delt):
    w = stock_warp(imR, pred, delt)
    diff = (imL - w).abs()
    pix = (w.sum(1, keepdim=True) > 0).expand_as(diff)
    tmp = diff[pix]
    tmp = tmp if len(tmp) > 0 else diff
    return tmp.mean() * 255, diff[w > 0].mean() * 255


def case(B, C, H, W, reps, warmup):
    g = torch.Generator().manual_seed(0)
    gt = (torch.rand(B, 1, H, W, generator=g) * 70 - 10).clamp(min=0).cuda()       # about 1/7 holes
    pred = (gt * (0.8 + 0.4 * torch.rand(B, 1, H, W, generator=g).cuda()) + 1.0)
    imL, imR = torch.rand(B, C, H, W, generator=g).cuda(), torch.rand(B, C, H, W, generator=g).cuda()

    def stock():
        return train.accuracy(pred, gt) + stock_compute_errors(gt, pred) + stock_photometric(imL, imR, pred, DELT)

    def fused():
        f = cv.stereo_metrics_finish(cv.stereo_metrics(pred, gt, imL, imR, delt=DELT))
        return (f["d1"], f["epe"], f["abs_rel"], f["sq_rel"], f["rmse"], f["rmse_log"], f["d1_kitti"], f["a1"],
                f["a2"], f["a3"], f["pixelerror"], f["pixelerror_elem"])

    vals = {"stock": [float(v) for v in stock()], "fused": [float(v) for v in fused()]}
    for _ in range(warmup):
        stock()
        fused()
    torch.cuda.synchronize()
    ts = {"stock": [], "fused": []}
    for _ in range(reps):
        ts["stock"].append(one(stock))                                   # alternate
        ts["fused"].append(one(fused))
    floor_bytes = 4.0 * (2 + 2 * C) * B * H * W
    return {"shape": [B, C, H, W], "values_stock": vals["stock"], "values_fused": vals["fused"],
            "stock": stats(ts["stock"]), "fused": stats(ts["fused"]),
            "hbm_floor_ms": floor_bytes / HBM_BYTES_PER_S * 1e3, "hbm_floor_bytes": floor_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU: none found")
    print(json.dumps({"reps": a.reps, "cases": [case(1, 3, 384, 1280, a.reps, a.warmup),
                                                case(4, 3, 540, 960, a.reps, a.warmup)]}))


if __name__ == "__main__":
    main()
