"""Confidence heads at the benchmark head shape, (1,48,96,320) -> (192,384,1280): the fused op
(dsm_disp_confidence_fwd), soft_argmin_up4_kernel and the torch composition in one process, device events
around back-to-back launches, alternating rounds (profiles/headconf.md).

    python scripts/bench_headconf.py [--radius 4] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsmnet_amd import _lib  # noqa: E402

B, Dc, Hc, Wc, D, H, W = 1, 48, 96, 320, 192, 384, 1280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    R = args.radius
    lib = _lib.load()
    cost = (4.0 * torch.randn(B, Dc, Hc, Wc, generator=torch.Generator().manual_seed(7))).cuda()
    outs = [torch.empty(B, H, W, device="cuda") for _ in range(5)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused(want):
        ptrs = [p(outs[0])] + [p(o) if w else None for o, w in zip(outs[1:], want)]
        rc = lib.dsm_disp_confidence_fwd(p(cost), *ptrs, B, Dc, Hc, Wc, D, H, W, 0, 0, R, _lib.DSM_F32, stream())
        assert rc == 0, rc

    def soft_argmin():
        rc = lib.dsm_soft_argmin_fwd(p(cost), p(outs[0]), None, B, Dc, Hc, Wc, D, H, W, 0, 0, _lib.DSM_F32, stream())
        assert rc == 0, rc

    def composition():
        v = F.interpolate(cost.unsqueeze(1), size=(D, H, W), mode="trilinear", align_corners=False)[:, 0]
        pr = torch.softmax(v, dim=1)
        d = torch.arange(D, device="cuda", dtype=torch.float32).view(1, D, 1, 1)
        dstar = v.argmax(dim=1, keepdim=True)
        win = ((d >= dstar - R) & (d <= dstar + R)).float()
        pwin = (pr * win).sum(1)
        return ((d * pr).sum(1), (d * pr * win).sum(1) / pwin, pr.gather(1, dstar)[:, 0], pwin,
                -(pr * torch.log(pr.clamp_min(1e-38))).sum(1))

    variants = {
        "disp_confidence_up4_kernel, five maps": (lambda: fused((1, 1, 1, 1)), 100),
        "disp_confidence_up4_kernel, no window pass": (lambda: fused((0, 1, 0, 1)), 100),
        "soft_argmin_up4_kernel": (soft_argmin, 100),
        "torch composition": (composition, 3),
    }
    for fn, _ in variants.values():              # warm-up: every shape, every code object
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, n) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / n)
    res = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
    fused((1, 1, 1, 1))
    torch.cuda.synchronize()
    res["max_abs_fused_minus_torch"] = dict(zip(("disp", "peak", "pmax", "pwin", "entropy"),
                                                ((a - b).abs().max().item() for a, b in zip(outs, composition()))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
