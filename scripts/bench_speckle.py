"""Speckle filter of one batch (csrc/speckle.hip, costvolume.filter_speckles) against the least any host
implementation pays, in ONE process, alternating the two so that both see the same machine:

  (a) device      filter_speckles(disp, 200, 1.0, valid=mask, want=("out", "keep"))
  (b) round_trip  the map and a byte mask copied device -> host -> device with NOTHING done on the host: the
                  copies and the synchronisation a host labelling needs before and after its own work
  (c) host_label  where scipy imports: the labelling of the same graph on the host
                  (scipy.sparse.csgraph.connected_components over the edge list), one run on the wall clock,
                  for information; it comes on top of (b)

on the left-right benchmark's kind of input (scripts/bench_lrcheck.py): a smooth map with an occluding box
and the mask of its check, about 7 % valid, then with every pixel valid.  The device result is checked
against the host labelling (where scipy imports) before anything is timed.  Event-timed after warm-up;
median and min..max of the repeats.  Prints one JSON line.

    python scripts/bench_speckle.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import costvolume as cv          # noqa: E402

MAX_SIZE, MAX_DIFF = 200, 1.0


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


def host_keep(disp, valid):
    """keep of the filter from scipy's connected components; None without scipy."""
    try:
        from scipy import sparse
        from scipy.sparse import csgraph
    except ImportError:
        return None
    d = disp.reshape((disp.shape[0],) + disp.shape[-2:])
    node = np.isfinite(d) & valid.reshape(d.shape).astype(bool)
    z = np.where(node, d, np.float32(0))
    idx = np.arange(d.size).reshape(d.shape)
    md = np.float32(MAX_DIFF)
    right = node[:, :, 1:] & node[:, :, :-1] & (np.abs(z[:, :, 1:] - z[:, :, :-1]) <= md)
    down = node[:, 1:] & node[:, :-1] & (np.abs(z[:, 1:] - z[:, :-1]) <= md)
    p = np.concatenate([idx[:, :, 1:][right], idx[:, 1:][down]])
    q = np.concatenate([idx[:, :, :-1][right], idx[:, :-1][down]])
    g = sparse.coo_matrix((np.ones(len(p), np.int8), (p, q)), shape=(d.size, d.size))
    comp = csgraph.connected_components(g, directed=False)[1].reshape(d.shape)
    cnt = np.bincount(comp[node], minlength=d.size)
    return (node & (cnt[comp] > MAX_SIZE)).reshape(disp.shape)


def case(B, H, W, all_valid, reps, warmup):
    g = torch.Generator().manual_seed(0)
    base = F.interpolate(torch.rand(B, 1, H // 32 + 2, W // 32 + 2, generator=g) * 60, size=(H, W), mode="bilinear",
                         align_corners=True)
    disp = base.clone()
    disp[:, :, H // 4: H // 2, W // 3: W // 2] += 20.0                 # an occluding box
    other = (base.flip(-1) + torch.rand(B, 1, H, W, generator=g)).contiguous()
    disp, other = disp.cuda(), other.cuda()
    mask = torch.ones_like(disp, dtype=torch.bool) if all_valid else cv.lr_check(disp, other, want=("mask",)).mask
    mask8 = mask.view(torch.uint8)
    pin_d = torch.empty(disp.shape, dtype=torch.float32).pin_memory()
    pin_m = torch.empty(mask.shape, dtype=torch.uint8).pin_memory()
    back_d, back_m = torch.empty_like(disp), torch.empty_like(mask8)

    def device():
        return cv.filter_speckles(disp, MAX_SIZE, MAX_DIFF, valid=mask, want=("out", "keep"))

    def round_trip():
        pin_d.copy_(disp, non_blocking=True)
        pin_m.copy_(mask8, non_blocking=True)
        torch.cuda.current_stream().synchronize()                    # the host would label here
        back_d.copy_(pin_d, non_blocking=True)
        back_m.copy_(pin_m, non_blocking=True)

    got = device()
    t0 = time.time()
    want = host_keep(disp.cpu().numpy(), mask.cpu().numpy())
    host_ms = (time.time() - t0) * 1e3
    runs = {"device": device, "round_trip": round_trip}
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():                                       # alternate
            ts[k].append(one(fn))
    out = {"shape": [B, H, W], "valid_fraction": float(mask.float().mean()), "kept_fraction": float(got.keep.float().mean()),
           "equals_host_labelling": None if want is None else bool(np.array_equal(got.keep.cpu().numpy(), want)),
           "host_label_ms_one_run": None if want is None else host_ms}
    out.update({k: stats(v) for k, v in ts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speckle.py measures on the GPU: none found")
    cases = [case(B, H, W, all_valid, a.reps, a.warmup)
             for (B, H, W) in ((1, 384, 1280), (4, 540, 960)) for all_valid in (False, True)]
    print(json.dumps({"reps": a.reps, "max_size": MAX_SIZE, "max_diff": MAX_DIFF, "cases": cases}))


if __name__ == "__main__":
    main()
