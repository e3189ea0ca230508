"""From host memory to the spatially augmented batch, two ways, at KITTI's size: 4 samples of
375 x 1242, imL | imR | dispL (16-bit), Stereo_train([768, 384], 0.4, 32).  Prints one JSON line.

  raw    the decoded planes packed in one pinned buffer (datasets.loader.pack_layout), one
         non-blocking copy, costvolume.stereo_spatial_raw                     (csrc/frames.hip)
  fp32   the (B, H0, W0, C) fp32 frames, assembled on the host beforehand, in a pinned buffer, one
         non-blocking copy, costvolume.stereo_spatial                         (csrc/spatial.hip)

Both get the same records.  Each repeat is timed with a pair of events, the first recorded right
before the copy and the second right after the launch, so a time runs from the first byte of the
copy to the end of the spatial kernel; the host's packing / assembling is outside it.  The two
paths alternate in one process after a warm-up; median (min..max) over ``--reps``.  The outputs
are compared with torch.equal.

    python scripts/bench_frames.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import _lib                          # noqa: E402
from dsmnet_amd import costvolume as cv              # noqa: E402
from dsmnet_amd import transforms as T               # noqa: E402
from dsmnet_amd.datasets.loader import pack_layout   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames.py measures on the GPU"
    B, H0, W0, C = 4, 375, 1242, 7
    rng = np.random.RandomState(0)
    items = []
    for i in range(B):
        disp = rng.randint(0, 200 * 256, size=(H0, W0)).astype(np.uint16)
        disp[rng.rand(H0, W0) < 0.3] = 0
        planes = [rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8) for _ in range(2)] + [disp]
        items.append((planes, (0, 0), (H0, W0), "%d" % i))
    sources, total = pack_layout(items, [_lib.DSM_DISP_U16_256] * B)
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    frames = torch.empty(B, H0, W0, C, dtype=torch.float32, pin_memory=True)
    for b, ((planes, _, _, _), s) in enumerate(zip(items, sources)):
        for p, off in zip(planes, s[:4]):
            stage.numpy()[off:off + p.nbytes] = p.reshape(-1).view(np.uint8)
        frames.numpy()[b] = np.concatenate([np.float32(planes[0]), np.float32(planes[1]),
                                            (np.float32(planes[2]) / np.float32(256))[:, :, None]], axis=2)
    np.random.seed(0)
    t = T.Stereo_train([768, 384], 0.4, 32)
    hw = t.spatial.out_hw(H0, W0)
    records = [t.spatial.draw(H0, W0) for _ in range(B)]
    raw_dev = torch.empty(total, dtype=torch.uint8, device="cuda")
    frames_dev = torch.empty(B, H0, W0, C, dtype=torch.float32, device="cuda")

    def raw_path():
        raw_dev.copy_(stage, non_blocking=True)
        return cv.stereo_spatial_raw(raw_dev, sources, records, (H0, W0), C, hw, 6)

    def fp32_path():
        frames_dev.copy_(frames, non_blocking=True)
        return cv.stereo_spatial(frames_dev, records, hw, 6)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    for _ in range(args.warmup):
        timed(raw_path), timed(fp32_path)
    times = {"raw": [], "fp32": []}
    for _ in range(args.reps):
        ms, got = timed(raw_path)
        times["raw"].append(ms)
        ms, want = timed(fp32_path)
        times["fp32"].append(ms)
    out = {"samples": [B, H0, W0, C], "crop": [768, 384], "scale_delt": 0.4, "reps": args.reps,
           "windows_wh": [[r[3], r[4]] for r in records], "bit_identical": bool(torch.equal(got, want)),
           "bytes_copied": {"raw": int(total), "fp32": int(frames.numel() * 4)}}
    for k, ts in times.items():
        ts.sort()
        out[k + "_ms"] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
    out["ratio_fp32_over_raw"] = out["fp32_ms"]["median"] / out["raw_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
