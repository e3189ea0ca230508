"""profiles/wide2d_train.md: training through the wide 3x3 layers of the DispNetC / iResNet encoder
(``costvolume.wide_conv2d_relu``, option ``wide_conv2d_train``) against the stock layers under autograd, on
one GPU, in one process, the two alternating.

    python scripts/wide2d_train_bench.py [--out profiles/wide2d_train.md] [--reps 20]

Per layer, at 4 pairs of 256 x 640 and at 1 pair of 384 x 1280: CALLS calls captured into one hipGraph per
variant, the graphs replayed alternately; the figure is the median over the rounds of (replay time / CALLS).
  stock:      y = relu(conv2d(x, w, b)); autograd.grad(y, [x, w, b], cot) on NCHW maps, as
              Sequential(Conv2d, ReLU) trains;
  new:        the same through wide_conv2d_relu on NHWC maps (packs cached, as inside a training step);
  its parts:  forward launch, dsm_bias_relu_bwd, backward-data launch, dsm_conv2d_wgrad, each alone;
  stock dX:   aten.convolution_backward asked for the data gradient only (stride-2 layers: what the transposed
              launch replaces).
Whole step: ``train.train_step_selfsup`` of DispNetC (depthmono-mask, Stereo_color) at 4 pairs of 256 x 640,
option off / on alternating, eager, host clock around a synchronise.  Needs the GPU: there is no CPU fallback."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsmnet_amd import costvolume as cv                      # noqa: E402
from dsmnet_amd import train, transforms                     # noqa: E402
from dsmnet_amd.models import model_create_by_name           # noqa: E402

# name, Cin, Cout, stride, input size as a divisor of the image
LAYERS = [("conv3b", 256, 256, 1, 8), ("conv4a", 256, 512, 2, 8), ("conv4b", 512, 512, 1, 16),
          ("conv5a", 512, 512, 2, 16), ("conv5b", 512, 512, 1, 32), ("conv6a", 512, 1024, 2, 32),
          ("conv6b", 1024, 1024, 1, 64)]
SETTINGS = [(4, 256, 640), (1, 384, 1280)]
CALLS = 10
CL = torch.channels_last


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


def layer_row(name, cin, cout, s, B, H, W, reps):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, cin, H, W, generator=gen).relu().cuda().requires_grad_(True)
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).cuda().requires_grad_(True)
    b = (torch.randn(cout, generator=gen) * 0.1).cuda().requires_grad_(True)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    cot = torch.randn(B, cout, Ho, Wo, generator=gen).cuda()
    xcl = x.detach().contiguous(memory_format=CL).requires_grad_(True)
    cotcl = cot.contiguous(memory_format=CL)

    def stock():
        y = F.relu(F.conv2d(x, w, b, s, 1))
        return torch.autograd.grad(y, [x, w, b], cot)

    def new():
        with cv.amax_scope(x.device):
            y = cv.wide_conv2d_relu(xcl, w, b, s)
            return torch.autograd.grad(y, [xcl, w, b], cotcl)

    ref, got = stock(), new()
    errs = [((a.float() - r).abs().max() / r.abs().max()).item() for a, r in zip(got, ref)]
    # the parts of the new path, each alone, on tensors that carry their maxima
    with torch.no_grad(), cv.amax_scope(x.device):
        xd = xcl.detach()
        cv.absmax(xd)
        ent = cv._wide_pack_entry(w)
        pf, pg = cv._wide_pack(ent, w, "forward"), cv._wide_pack(ent, w, "gradient")
        y = cv.conv2d_block(xd, pf, cout, None, b.detach(), stride=s, relu=1)
        g, _ = cv.bias_relu_bwd(cotcl, y)
        g._dsm_amax = cv.absmax(g)                     # slots of their own: the graphs below outlive this scope
    xd._dsm_amax = xd._dsm_amax.clone()
    g._dsm_amax = g._dsm_amax.clone()
    nograd = torch.no_grad()

    def fwd():
        with nograd:
            return cv.conv2d_block(xd, pf, cout, None, b.detach(), stride=s, relu=1)

    def relu_bwd():
        with nograd:
            return cv.bias_relu_bwd(cotcl, y)

    def dx():
        with nograd:
            return cv.conv2d_block(g, pg, cin, stride=1) if s == 1 else cv.conv2d_transposed_block(g, pg, cin, (H, W))

    def dw():
        with nograd:
            return cv._wgrad2d(xd, g, s, 1)

    gd, wd, xs = g.detach().contiguous(), w.detach(), x.detach()

    def stock_dx():
        with nograd:
            return torch.ops.aten.convolution_backward(gd, xs, wd, None, [s, s], [1, 1], [1, 1], False, [0, 0], 1,
                                                       [True, False, False])[0]

    t = replay_us([graph_of(f) for f in (stock, new, fwd, relu_bwd, dx, dw, stock_dx)], reps)
    return (name, cin, cout, s, "%dx%dx%d" % (B, Ho, Wo)) + tuple(t) + (max(errs),)


def step_rows(reps, nedge):
    torch.manual_seed(3)
    models = {False: model_create_by_name("dispnetcorr", 192).cuda()}
    models[True] = copy.deepcopy(models[False])
    gen = torch.Generator().manual_seed(2)
    left = torch.rand(4, 3, 256, 640, generator=gen)
    batch = torch.cat([left, torch.roll(left, -5, dims=3)], 1).cuda()
    state, times, shares = {}, {False: [], True: []}, {}
    for on, m in models.items():
        lossfun = train.losses("depthmono-mask", m.count_levels, 10)
        lossfun.Weight_Adjust_levels(2)
        state[on] = (lossfun, train.make_optimizer(m, lr=1e-5))
    aug = transforms.Stereo_color()

    def step(on, timer=None):
        old = cv.set_option("wide_conv2d_train", on)
        cv.set_timer(timer)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train.train_step_selfsup(models[on], state[on][1], state[on][0], batch, augment=aug, nedge=nedge)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        finally:
            cv.set_timer(None)
            cv.set_option("wide_conv2d_train", old)
    for on in (False, True):
        step(on), step(on)                             # warm-up (solver search of the stock layers)
    for _ in range(reps):
        for on in (False, True):
            times[on].append(step(on))
    timer = cv.LaunchTimer()
    step(True, timer)
    for key, e in timer.summary().items():
        for tag, pre in (("forward + dX s1", "conv2d_wide_"), ("dX s2", "deconv2d_wide_"), ("relu-bwd", "dsm_bias_relu_bwd"),
                         ("dW", "conv2d_wgrad_kernel<")):
            if key.startswith(pre):
                shares[tag] = shares.get(tag, 0.0) + e["ms"]
    return statistics.median(times[False]), statistics.median(times[True]), shares


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide2d_train_bench needs the GPU")
    cv.set_option("conv_precision", "f16x2")
    lines = ["# Training through the wide 3x3 layers (`costvolume.wide_conv2d_relu`) against the stock layers", "",
             "`python scripts/wide2d_train_bench.py`: f16x2, one process, stock and new alternating, replayed graphs of",
             "%d calls, median of %d rounds, microseconds per call." % (CALLS, args.reps), ""]
    for B, H, W in SETTINGS:
        lines += ["## Per layer, %d pair(s) of %d x %d" % (B, H, W), "",
                  "| layer | Cin->Cout, s | out | stock fwd+bwd | new fwd+bwd | stock/new | new: forward | relu-bwd | dX | dW | stock dX alone | stock dX / new dX | worst grad diff / max |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for name, cin, cout, s, div in LAYERS:
            r = layer_row(name, cin, cout, s, B, H // div, W // div, args.reps)
            lines.append("| %s | %d->%d, %d | %s | %.1f | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1e |"
                         % (r[:5] + (r[5], r[6], r[5] / r[6], r[7], r[8], r[9], r[10], r[11], r[11] / r[9], r[12])))
            print(lines[-1], flush=True)
        lines.append("")
    if not args.skip_step:
        lines += ["## Whole `train_step_selfsup` of DispNetC, 4 pairs of 256 x 640, eager, milliseconds (median)", "",
                  "| crop (nedge) | option off | option on | off/on | on: wide launches ms (forward + dX s1 / dX s2 / relu-bwd / dW) | share of the step |",
                  "|---|---|---|---|---|---|"]
        for nedge in (64, 0):
            off, on, sh = step_rows(max(4, args.reps // 2), nedge)
            parts = [sh.get(k, 0.0) for k in ("forward + dX s1", "dX s2", "relu-bwd", "dW")]
            lines.append("| %d | %.2f | %.2f | %.3f | %.2f / %.2f / %.2f / %.2f | %.1f %% |"
                         % ((nedge, off, on, off / on) + tuple(parts) + (100.0 * sum(parts) / on,)))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
