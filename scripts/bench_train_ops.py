"""profiles/train_ops.md: training through the fused iResNet warp (``costvolume.warp_abs_error``, option
``warp_train``) and the fused decoder levels (``costvolume.decoder_level``, option ``decoder_train``) against the
stock ops under autograd, on one GPU, in one process, the two alternating.

    python scripts/bench_train_ops.py [--out profiles/train_ops.md] [--reps 20]

Per op, at 4 pairs of 256 x 640 and at 1 pair of 384 x 1280: CALLS calls captured into one hipGraph per variant,
the graphs replayed alternately; the figure is the median over the rounds of (replay time / CALLS).
  warp, stock:   |L - grid_sample(R + delt, grid)| with the grids built by linspace / stack as imwrap_BCHW builds
                 them, but on the device (imwrap_BCHW's own host linspace and host epsilon cannot be captured: the
                 stock figure leaves out two host-to-device copies per call); autograd.grad for L, R and disp;
  warp, new:     the same through ``warp_abs_error``; its forward and backward launches also each alone, with the
                 bytes they have to move (every map read once, every gradient written once, gR zeroed and summed);
  level, stock:  ``decoder_level`` with ``decoder_train`` off (transposed convolution with bias, in-place ReLU,
                 interpolate, three crops, cat) and autograd.grad for x, weight, bias, pr and skip;
  level, new:    the same with the option on; the two launches of ``DecoderCatFunction`` also each alone.
Whole step: ``train.train_step`` (supervised) of iResNet and DispNetC at 4 pairs of 256 x 640, both options off /
on alternating, eager, host clock around a synchronise.  Needs the GPU: there is no CPU fallback."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsmnet_amd import costvolume as cv                      # noqa: E402
from dsmnet_amd import train                                 # noqa: E402
from dsmnet_amd.models import model_create_by_name           # noqa: E402

SETTINGS = [(4, 256, 640), (1, 384, 1280)]
# iResNet's decoder: name, deconv Cin, width, skip channels, output size as a divisor of the image
LEVELS = [("deconv5", 1024, 512, 512, 32), ("deconv4", 512, 256, 512, 16), ("deconv3", 256, 128, 256, 8),
          ("deconv2", 128, 64, 128, 4), ("deconv1", 64, 32, 64, 2), ("deconv0", 32, 32, 32, 1),
          ("r_deconv1", 128, 64, 64, 2), ("r_deconv0", 64, 32, 32, 1)]
CALLS = 10


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(CALLS)]
    return g, keep


def replay_us(graphs, reps):
    times = [[] for _ in graphs]
    for _ in range(reps):
        for i, (g, _) in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3 / CALLS)
    return [statistics.median(t) for t in times]


def stock_warp_abs(L, R, disp, delt):
    bn, _, h0, w0 = R.shape
    _, _, h, w = disp.shape
    x1 = -1.0 + (w - 1) * 2.0 / (w0 - 1)
    y1 = -1.0 + (h - 1) * 2.0 / (h0 - 1)
    gx = torch.linspace(-1.0, x1, w, device=R.device).view(1, 1, w).expand(bn, h, w)
    gy = torch.linspace(-1.0, y1, h, device=R.device).view(1, h, 1).expand(bn, h, w)
    grid = torch.stack([gx - disp.squeeze(1) * 2.0 / (w0 - 1), gy], dim=3)
    return torch.abs(L - F.grid_sample(R + delt, grid, mode="bilinear", padding_mode="zeros", align_corners=False))


def warp_row(B, H, W, reps, C=32):
    gen = torch.Generator().manual_seed(1)
    L, R = (torch.randn(B, C, H, W, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = 20.0 + 10.0 * torch.sin(xx / 50.0) * torch.cos(yy / 30.0)            # a disparity map, not noise
    disp = (smooth + 0.5 * torch.rand(B, 1, H, W, generator=gen)).cuda().requires_grad_(True)
    cot = torch.randn(B, C, H, W, generator=gen).cuda()
    delt_t, delt = torch.tensor(6e-5, device="cuda"), 6e-5
    lib = cv._lib.load()

    def stock():
        return torch.autograd.grad(stock_warp_abs(L, R, disp, delt_t), [L, R, disp], cot)

    def new():
        return torch.autograd.grad(cv.warp_abs_error(L, R, disp, delt), [L, R, disp], cot)
    ref, got = stock(), new()
    # a sample position within rounding of an integer takes the other pair of taps in one of the two fp32 paths:
    # such elements differ by O(1), so the figure is the share of elements further apart than 1e-4 of the maximum
    errs = [((a - r).abs() > 1e-4 * r.abs().max()).float().mean().item() for a, r in zip(got, ref)]
    Ld, Rd, dd = L.detach(), R.detach(), disp.detach()
    out, gL, gR, gd = torch.empty_like(Ld), torch.empty_like(Ld), torch.empty_like(Rd), torch.empty_like(dd)

    def fwd():
        cv._lib.check(lib.dsm_warp_abs_error(cv._p(Ld), cv._p(Rd), cv._p(dd), cv._p(out), B, C, H, W, H, W, delt,
                                             cv._stream()), "fwd")

    def bwd():
        cv._lib.check(lib.dsm_warp_abs_error_bwd(cv._p(cot), cv._p(Ld), cv._p(Rd), cv._p(dd), cv._p(gL), cv._p(gR),
                                                 cv._p(gd), B, C, H, W, H, W, delt, cv._stream()), "bwd")
    t = replay_us([graph_of(f) for f in (stock, new, fwd, bwd)], reps)
    n, px = B * C * H * W, B * H * W
    fwd_bytes, bwd_bytes = 4.0 * (3 * n + px), 4.0 * (6 * n + 2 * px)      # gR counted twice: zeroed, then summed
    return ("%dx%dx%dx%d" % (B, C, H, W),) + tuple(t) + (fwd_bytes, bwd_bytes, max(errs))


def level_row(name, cin, width, cskip, div, B, H, W, reps):
    torch.manual_seed(2)
    h, w = H // div, W // div
    deconv = nn.Sequential(nn.ConvTranspose2d(cin, width, 4, 2, 1, bias=True), nn.ReLU(inplace=True)).cuda()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, h // 2, w // 2, generator=gen).cuda().requires_grad_(True)
    pr = torch.randn(B, 1, h // 2, w // 2, generator=gen).cuda().requires_grad_(True)
    skip = torch.randn(B, cskip, h, w, generator=gen).cuda().requires_grad_(True)
    cot = torch.randn(B, width + 1 + cskip, h, w, generator=gen).cuda()
    wants = [x, deconv[0].weight, deconv[0].bias, pr, skip]
    lib = cv._lib.load()

    def level(on):
        def fn():
            old = cv.set_option("decoder_train", on)
            try:
                return torch.autograd.grad(cv.decoder_level(deconv, x, pr, skip), wants, cot)
            finally:
                cv.set_option("decoder_train", old)
        return fn
    ref, got = level(False)(), level(True)()
    errs = [((a - r).abs().max() / r.abs().max()).item() for a, r in zip(got, ref)]
    with torch.no_grad():
        up = F.conv_transpose2d(x, deconv[0].weight, None, 2, 1).contiguous()
    bias, prd, sd = deconv[0].bias.detach(), pr.detach(), skip.detach()
    out, g_up, g_b = torch.empty_like(cot), torch.empty_like(up), torch.empty_like(bias)
    g_pr, g_skip = torch.empty_like(prd), torch.empty_like(sd)
    dims = (B, width, 1, cskip, h, w, h // 2, w // 2, h, w, 1)

    def fwd():
        cv._lib.check(lib.dsm_decoder_cat(cv._p(up), cv._p(bias), cv._p(prd), cv._p(sd), cv._p(out), *dims,
                                          cv._stream()), "fwd")

    def bwd():
        cv._lib.check(lib.dsm_decoder_cat_bwd(cv._p(cot), cv._p(out), cv._p(g_up), cv._p(g_b), cv._p(g_pr),
                                              cv._p(g_skip), *dims, cv._stream()), "bwd")
    fwd()
    t = replay_us([graph_of(f) for f in (level(False), level(True), fwd, bwd)], reps)
    fwd_bytes = 4.0 * (up.numel() + prd.numel() + sd.numel() + out.numel())
    bwd_bytes = 4.0 * (cot.numel() + up.numel() + g_up.numel() + g_pr.numel() + g_skip.numel())    # + the mask channels
    return (name, "%d->%d+1+%d" % (cin, width, cskip), "%dx%dx%d" % (B, h, w)) + tuple(t) + (fwd_bytes, bwd_bytes,
                                                                                             max(errs))


def _batch(B, H, W, shift, seed):
    g = torch.Generator().manual_seed(seed)
    left = torch.rand(B, 3, H, W, generator=g)
    disp = torch.full((B, 1, H, W), float(shift))
    disp[:, :, :, :shift] = 0
    return torch.cat([left, torch.roll(left, -shift, dims=3), disp], 1).cuda()


def step_row(name, reps, B=4, H=256, W=640):
    torch.manual_seed(3)
    models = {False: model_create_by_name(name, 192).cuda()}
    models[True] = copy.deepcopy(models[False])
    batch = _batch(B, H, W, 6, 2)
    state, times = {}, {False: [], True: []}
    for on, m in models.items():
        lossfun = train.losses("supervised", m.count_levels, maxepoch_weight_adjust=37)
        lossfun.Weight_Adjust_levels(10)
        state[on] = (lossfun, train.make_optimizer(m, lr=1e-5))

    def step(on, timer=None):
        old = (cv.set_option("warp_train", on), cv.set_option("decoder_train", on))
        cv.set_timer(timer)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = train.train_step(models[on], state[on][1], state[on][0], batch)[0]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, loss
        finally:
            cv.set_timer(None)
            cv.set_option("warp_train", old[0])
            cv.set_option("decoder_train", old[1])
    first = {}
    for on in (False, True):
        first[on] = step(on)[1]
        step(on)                                       # warm-up (solver search of the stock layers)
    for _ in range(reps):
        for on in (False, True):
            times[on].append(step(on)[0])
    timer = cv.LaunchTimer()
    step(True, timer)
    ms = {k: e["ms"] for k, e in timer.summary().items() if k.startswith(("warp_abs_error", "decoder_cat"))}
    return statistics.median(times[False]), statistics.median(times[True]), ms, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_ops needs the GPU")
    lines = ["# Training through the fused warp and decoder levels against the stock ops", "",
             "`python scripts/bench_train_ops.py`: one process, stock and new alternating, replayed graphs of %d calls,"
             % CALLS, "median of %d rounds, microseconds per call; GB/s = algorithmic bytes / time." % args.reps, ""]
    lines += ["## iResNet warp + abs error, forward + backward (gradients of L, R and disp)", "",
              "| maps | stock fwd+bwd | new fwd+bwd | stock/new | new: forward alone | GB/s | backward alone | GB/s | share of gradient elements > 1e-4 of the max apart |",
              "|---|---|---|---|---|---|---|---|---|"]
    for B, H, W in SETTINGS:
        r = warp_row(B, H, W, args.reps)
        lines.append("| %s | %.1f | %.1f | %.2f | %.1f | %.0f | %.1f | %.0f | %.1e |"
                     % (r[0], r[1], r[2], r[1] / r[2], r[3], r[5] / r[3] * 1e-3, r[4], r[6] / r[4] * 1e-3, r[7]))
        print(lines[-1], flush=True)
    lines.append("")
    for B, H, W in SETTINGS:
        lines += ["## iResNet decoder levels, forward + backward, %d pair(s) of %d x %d" % (B, H, W), "",
                  "| level | Cin->channels | out | stock fwd+bwd | new fwd+bwd | stock/new | new: `decoder_cat` alone | GB/s | `decoder_cat_bwd` alone | GB/s | worst grad diff / max |",
                  "|---|---|---|---|---|---|---|---|---|---|---|"]
        for lv in LEVELS:
            r = level_row(*lv, B, H, W, args.reps)
            lines.append("| %s | %s | %s | %.1f | %.1f | %.2f | %.1f | %.0f | %.1f | %.0f | %.1e |"
                         % (r[0], r[1], r[2], r[3], r[4], r[3] / r[4], r[5], r[7] / r[5] * 1e-3, r[6], r[8] / r[6] * 1e-3,
                            r[9]))
            print(lines[-1], flush=True)
        lines.append("")
    if not args.skip_step:
        lines += ["## Whole supervised `train_step`, 4 pairs of 256 x 640, eager, milliseconds (median)", "",
                  "| model | options off | options on | off/on | on: ms inside the four fused launches | first loss off / on |",
                  "|---|---|---|---|---|---|"]
        for name in ("iresnet", "dispnetcorr"):
            off, on, ms, first = step_row(name, max(4, args.reps // 2))
            parts = ", ".join("%s %.2f" % (k, v) for k, v in sorted(ms.items()))
            lines.append("| %s | %.2f | %.2f | %.3f | %s | %.6f / %.6f |"
                         % (name, off, on, off / on, parts, first[False], first[True]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
