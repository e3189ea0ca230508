"""Fused stereo spatial augmentation (csrc/spatial.hip) at the recipe's shape: 4 frames of
540 x 960 x 7 (imL | imR | dispL) cropped to 384 x 768 (stereo_supervised.py:34), shift_max 32,
with scale_delt 0 (the recipes' setting) and 0.4 (the factory's default).  Prints one JSON line.

  kernel_us            device time per launch of stereo_spatial_kernel: back-to-back launches
                       queued behind a spin kernel (so host enqueue time is hidden), cycling over
                       ``--buffers`` frame batches (> 256 MiB in all, so the Infinity Cache holds
                       none of them)
  bytes_per_launch     algorithmic bytes: every source pixel of the windows once (4C B, the right
                       view's and the left view's columns counted once each) + 4C B written per
                       output pixel
  gbps / hbm_fraction  bytes_per_launch / kernel_us, against the 6.3 TB/s HBM peak
  call_ms              Stereo_Spatial(...)(frames): host planning, output allocation, the launch
                       (median of synchronised calls)
  torch_ms             the same records through stock torch ops on the device (slices, where,
                       cat, permute, F.interpolate), image by image, for comparison
  torch_max_diff       max |torch restatement - kernel| (interpolate is not bit-equal to the rule)

    python scripts/bench_spatial.py [--reps 200] [--buffers 6] [--delts 0,0.4]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import costvolume as cv         # noqa: E402
from dsmnet_amd import transforms as T          # noqa: E402

HBM_TBS = 6.3


def device_time_us(launch, xs, reps):
    """Per-launch device time: all launches enqueued while a spin kernel holds the stream."""
    for x in xs:
        launch(x)
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        launch(xs[i % len(xs)])
    b.record()
    torch.cuda.synchronize()
    return 1000.0 * a.elapsed_time(b) / reps


def call_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_restatement(x, records, hw, channels):
    C = x.shape[3]
    outs = []
    for b, (shift, ws, hs, w, h, resize, s) in enumerate(r[:7] for r in records):
        left = x[b, hs:hs + h, ws:ws + w]
        right = x[b, hs:hs + h, ws + shift:ws + shift + w]
        parts = [left[..., :3], right[..., 3:6]]
        for c in range(6, C):
            d = (right if c == 7 else left)[..., c:c + 1]
            parts.append(torch.where(d != 0, d + shift, d))
        win = torch.cat(parts, -1).permute(2, 0, 1)
        if resize:
            win = F.interpolate(win[None], size=hw, mode="bilinear", align_corners=False)[0]
            win[6:] *= s
        win = win.contiguous()
        win[:channels] /= 255.0
        outs.append(win)
    return torch.stack(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--buffers", type=int, default=6)
    ap.add_argument("--delts", default="0,0.4", help="scale_delt settings (one per kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spatial.py measures on the GPU"
    B, H0, W0, C = 4, 540, 960, 7
    g = torch.Generator().manual_seed(0)
    xs = []
    for _ in range(args.buffers):
        x = torch.rand(B, H0, W0, C, generator=g) * 255
        x[..., 6] = torch.where(x[..., 6] < 40, torch.zeros(()), x[..., 6])
        xs.append(x.cuda())
    out = {"frames": [B, H0, W0, C], "crop": [768, 384], "reps": args.reps, "buffers": args.buffers,
           "buffer_mib": round(args.buffers * xs[0].numel() * 4 / 2 ** 20, 1), "cases": {}}
    for delt in (float(d) for d in args.delts.split(",")):
        delt = 0 if delt == 0 else delt
        np.random.seed(0)
        t = T.Stereo_Spatial([768, 384], delt, 32)
        records, hw, channels = t.plan_spatial(B, H0, W0)
        nbytes = 4.0 * C * (sum(r[3] * r[4] for r in records) + B * hw[0] * hw[1])
        us = device_time_us(lambda x: cv.stereo_spatial(x, records, hw, channels), xs, args.reps)
        got = cv.stereo_spatial(xs[0], records, hw, channels)
        ref = torch_restatement(xs[0], records, hw, channels)
        out["cases"]["scale_delt=%s" % delt] = {
            "windows_wh": [[r[3], r[4]] for r in records], "scale_rand": [round(r[6], 4) for r in records],
            "bytes_per_launch": nbytes, "hbm_floor_us": nbytes / (HBM_TBS * 1e6), "kernel_us": us,
            "gbps": nbytes / (us * 1e3), "hbm_fraction": nbytes / (us * 1e3) / (HBM_TBS * 1e3),
            "call_ms": call_ms(lambda: t(xs[1]), args.reps),
            "torch_ms": call_ms(lambda: torch_restatement(xs[2], records, hw, channels), max(5, args.reps // 4)),
            "torch_max_diff": (got - ref).abs().max().item()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
