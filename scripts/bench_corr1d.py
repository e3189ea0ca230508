"""Corr1d alone at the three model shapes of DESIGN.md 3.4, through the C ABI on preallocated buffers, ONE
process, the sides of every comparison alternating window by window so that all see the same machine:

  (a) the dot-product data gradient: the naive kernel (``dsm_corr1d_sim_bwd`` with DSM_CORR_BWD_NAIVE: the
      kernel of ``dsm_corr1d_bwd``) against the LDS-tiled kernel; their outputs are compared first at the
      suite's 3e-4 absolute bound;
  (b) the cosine similarity beside the dot product, forward and backward: what the norm pre-pass, the epilogue
      and the backward pre-pass cost.

Event-timed windows of ``--window`` launches (>= 50) after warm-up; per launch: median and min..max over
``--reps`` windows.  Beside each time the algorithmic bytes of the call (every tensor read or written once per
launch that touches it) and the rate they imply.  Prints one JSON line.

    python scripts/bench_corr1d.py [--reps 9] [--window 50] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import _lib                      # noqa: E402
from dsmnet_amd import costvolume as cv          # noqa: E402

SHAPES = [  # (B, C, H, W), D, stride, ksize
    ((1, 128, 96, 320), 41, 1, 1),               # DispNetC, iResNet's first correlation
    ((1, 128, 96, 320), 81, 1, 1),               # iResNet
    ((1, 64, 192, 640), 41, 2, 3),               # iResNet's refinement correlation
]


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stats(ts, nbytes):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"median_us": med * 1e3, "min_us": ts[0] * 1e3, "max_us": ts[-1] * 1e3, "bytes": nbytes,
            "GBps_at_median": nbytes / (med * 1e-3) / 1e9}


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def bench_shape(shape, D, s, k, reps, win, warmup):
    lib = _lib.load()
    B, C, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(0)
    fL = torch.randn(*shape, device="cuda", generator=g)
    fR = torch.randn(*shape, device="cuda", generator=g)
    cot = torch.randn(B, D, H, W, device="cuda", generator=g)
    new = lambda *sh: torch.empty(*sh, device="cuda")
    out, raw, inv = new(B, D, H, W), (new(B, D, H, W) if k > 1 else None), new(2, B, H, W)
    out_d, tmp_d = new(B, D, H, W), (new(B, D, H, W) if k > 1 else None)
    ws = new(max(1, lib.dsm_corr1d_sim_workspace_bytes(B, C, H, W, D, k, _lib.DSM_SIM_COSINE) // 4))
    grads = {name: (torch.empty_like(fL), torch.empty_like(fR)) for name in ("naive", "tiled", "cos", "cos_naive")}
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (B, C, H, W, D, s, k)

    def chk(rc):
        if rc != 0:
            raise SystemExit("launch refused: %d" % rc)

    def fwd_dot():
        chk(lib.dsm_corr1d_fwd(p(fL), p(fR), p(out_d), p(tmp_d), *dims, _lib.DSM_F32, st()))

    def fwd_cos():
        chk(lib.dsm_corr1d_sim_fwd(p(fL), p(fR), p(out), p(raw), p(inv), *dims, _lib.DSM_SIM_COSINE, 1e-8, _lib.DSM_F32, st()))

    def bwd(name, sim, flags):
        dl, dr = grads[name]
        cos = sim == _lib.DSM_SIM_COSINE
        chk(lib.dsm_corr1d_sim_bwd(p(cot), p(fL), p(fR), p(raw if k > 1 else out) if cos else None, p(inv) if cos else None,
                                   p(dl), p(dr), p(ws), *dims, sim, 1e-8, flags, _lib.DSM_F32, st()))

    sides = {
        "fwd_dot": fwd_dot, "fwd_cosine": fwd_cos,
        "bwd_dot_naive": lambda: bwd("naive", _lib.DSM_SIM_DOT, _lib.DSM_CORR_BWD_NAIVE),
        "bwd_dot_tiled": lambda: bwd("tiled", _lib.DSM_SIM_DOT, 0),
        "bwd_cosine": lambda: bwd("cos", _lib.DSM_SIM_COSINE, 0),
        "bwd_cosine_naive": lambda: bwd("cos_naive", _lib.DSM_SIM_COSINE, _lib.DSM_CORR_BWD_NAIVE),
    }
    for fn in sides.values():                    # (the cosine forward first fills raw / inv for its backward)
        fn()
    torch.cuda.synchronize()
    diff = max((grads["naive"][i] - grads["tiled"][i]).abs().max().item() for i in (0, 1))
    diff_cos = max((grads["cos"][i] - grads["cos_naive"][i]).abs().max().item() for i in (0, 1))
    if not diff <= 3e-4:
        raise SystemExit("tiled and naive dot-product gradients differ by %.3e > 3e-4" % diff)
    sc = torch.empty(4, device="cuda")
    plans = {"fwd_dot": cv.corr1d_plan_name(fL, fR, sc, sc if k > 1 else None, *dims),
             "fwd_cosine": cv.corr1d_sim_fwd_plan_name(fL, fR, sc, sc if k > 1 else None, sc, *dims, "cosine"),
             "bwd_dot_tiled": cv.corr1d_sim_bwd_plan_name(cot, fL, fR, None, None, sc, sc, sc if k > 1 else None, *dims, "dot"),
             "bwd_cosine": cv.corr1d_sim_bwd_plan_name(cot, fL, fR, sc, sc, sc, sc, sc, *dims, "cosine")}
    feat, vol, pix = 4.0 * B * C * H * W, 4.0 * B * D * H * W, 4.0 * B * H * W
    box = 2 * vol if k > 1 else 0.0              # the filter reads one map and writes another
    nbytes = {"fwd_dot": 2 * feat + vol + box,
              "fwd_cosine": 2 * feat + 2 * pix + 2 * feat + 2 * pix + vol + box,       # norm pass; correlation + inv
              "bwd_dot_naive": vol + 4 * feat + box, "bwd_dot_tiled": vol + 4 * feat + box,
              "bwd_cosine": 3 * vol + 4 * pix + vol + 4 * feat + 2 * pix + box}        # pre-pass; data gradient + coef
    nbytes["bwd_cosine_naive"] = nbytes["bwd_cosine"]
    for _ in range(warmup):
        for fn in sides.values():
            window(fn, win)
    ts = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():           # alternate
            ts[name].append(window(fn, win))
    res = {"shape": list(shape), "D": D, "stride": s, "ksize": k, "window": win, "reps": reps, "plans": plans,
           "max_abs_diff_tiled_vs_naive": diff, "max_abs_diff_cosine_tiled_vs_naive": diff_cos}
    for name in sides:
        res[name] = stats(ts[name], nbytes[name])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corr1d.py measures on the GPU: none found")
    if a.window < 50:
        raise SystemExit("--window must be at least 50 launches")
    print(json.dumps({"cases": [bench_shape(sh, D, s, k, a.reps, a.window, a.warmup) for sh, D, s, k in SHAPES]}))


if __name__ == "__main__":
    main()
