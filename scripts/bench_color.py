"""Fused stereo colour augmentation (csrc/color.hip) at the preset's shape: B = 4, 6 x 256 x 640
(DSMnet_train_kitti-raw.sh's 768 x 384 crop minus nedge = 64 on each side).  Prints one JSON line.

  kernel_us            device time per launch of stereo_color_kernel: back-to-back launches
                       queued behind a spin kernel (so host enqueue time is hidden), cycling over
                       ``--buffers`` batches (> 256 MiB in all, so the Infinity Cache holds none of
                       them), for the full Stereo_color records and for Normalize-only records
                       (same bytes, no powf)
  gbps                 algorithmic bytes (24 B read + 24 B written per pixel) / kernel_us,
                       against the 6.3 TB/s HBM peak
  call_ms              Stereo_color()(batch): host planning, 4 normal_ draws and the launch
                       (median of synchronised calls)
  torch_loop_ms        the reference's per-image loop with stock torch ops
                       (tests/color_oracle.stereo_color_batch_torch), for comparison

    python scripts/bench_color.py [--reps 50] [--buffers 20]
"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import _lib                     # noqa: E402
from dsmnet_amd import costvolume as cv         # noqa: E402
from dsmnet_amd import transforms as T          # noqa: E402
from tests import color_oracle as CO            # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--buffers", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_color.py measures on the GPU"
    B, C, H, W = 4, 6, 256, 640
    g = torch.Generator().manual_seed(0)
    xs = [torch.rand(B, C, H, W, generator=g).cuda() for _ in range(args.buffers)]
    random.seed(0)
    torch.manual_seed(0)
    recs, alpha, G = T.Stereo_color().plan(B, C, "cuda")[0]
    norm = [((0, 1, 2, 3), (1.0, 0.0, 0.0, 1.0), _lib.DSM_COLOR_NORMALIZE, 0)] * (B * G)
    nbytes = 8.0 * B * 3 * G * H * W
    out = {"shape": [B, C, H, W], "reps": args.reps, "buffers": args.buffers,
           "buffer_mib": round(args.buffers * xs[0].numel() * 4 / 2 ** 20, 1),
           "bytes_per_launch": nbytes, "hbm_floor_us": nbytes / (HBM_TBS * 1e6), "kernel_us": {}, "gbps": {}}
    for name, r, a in (("stereo_color", recs, alpha), ("normalize_only", norm, None)):
        us = device_time_us(lambda x: cv.stereo_color(x, r, a, G), xs, args.reps)
        out["kernel_us"][name] = us
        out["gbps"][name] = nbytes / (us * 1e3)
    out["hbm_fraction"] = out["gbps"]["stereo_color"] / (HBM_TBS * 1e3)
    t = T.Stereo_color()
    out["call_ms"] = call_ms(lambda: t(xs[0]), args.reps)
    out["torch_loop_ms"] = call_ms(lambda: CO.stereo_color_batch_torch(xs[1]), max(5, args.reps // 5))
    out["speedup_call_vs_torch_loop"] = out["torch_loop_ms"] / out["call_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
