"""profiles/wide2d.md: the wide 3x3 layers of the DispNetC / iResNet encoder (csrc/conv_wide2d.hpp) against
the stock layer, on one GPU, in one process, the two alternating.

    python scripts/wide2d_bench.py [--out profiles/wide2d.md] [--reps 30]

Per layer: 20 calls captured into one hipGraph per variant (device time without the Python launch path),
the graphs replayed alternately; the figure is the median over the rounds of (replay time / 20).
  stock: F.relu(F.conv2d(x, w, b, stride, 1)) on the NCHW map, as Sequential(Conv2d, ReLU) runs it;
  wide:  costvolume.conv2d_block on the NHWC map that carries its absolute maximum (both launches of a
         K-split layer and the amax slot's fill included).
Whole forwards: ``wide_conv2d`` off / on alternating, eager (host clock around a synchronise) and replayed
from a captured graph (dsmnet_amd.graphs.GraphedForward).  Needs the GPU: there is no CPU fallback."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsmnet_amd import costvolume as cv                      # noqa: E402
from dsmnet_amd.graphs import GraphedForward                 # noqa: E402
from dsmnet_amd.models import model_create_by_name           # noqa: E402

# name, Cin, Cout, stride, input (H, W) at 384 x 1280
LAYERS = [("conv3b", 256, 256, 1, (48, 160)), ("conv4a", 256, 512, 2, (48, 160)), ("conv4b", 512, 512, 1, (24, 80)),
          ("conv5a", 512, 512, 2, (24, 80)), ("conv5b", 512, 512, 1, (12, 40)), ("conv6a", 512, 1024, 2, (12, 40)),
          ("conv6b", 1024, 1024, 1, (6, 20))]
CALLS = 20


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        keep = [fn() for _ in range(CALLS)]
    return g, keep


def replay_us(graphs, reps):
    """Median microseconds per call of each graph, the graphs replayed in turn ``reps`` times."""
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


def layer_rows(reps):
    rows = []
    for name, cin, cout, s, (H, W) in LAYERS:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(1, cin, H, W, generator=g).relu().cuda()
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda()
        b = (torch.randn(cout, generator=g) * 0.1).cuda()
        xcl = x.contiguous(memory_format=torch.channels_last)
        cv.absmax(xcl)
        packed, ones = cv.pack_conv2d_weight(w), torch.ones(cout, device="cuda")

        def stock():
            return F.relu(F.conv2d(x, w, b, s, 1))

        def wide():
            with cv.amax_scope(x.device):
                return cv.conv2d_block(xcl, packed, cout, ones, b, stride=s, relu=1)

        err = (wide().float() - stock()).abs().max().item() / stock().abs().max().item()
        t_stock, t_wide = replay_us([graph_of(stock), graph_of(wide)], reps)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        gflop = 2.0 * 9 * cin * cout * Ho * Wo / 1e9
        wbytes = 4.0 * 9 * cin * cout                       # the two fp16 planes the kernel streams
        a = cv._lib.Conv3dArgs()
        a.x = a.w_packed = a.y = a.x_amax = 16
        a.B, a.Cin, a.Cout, a.Di, a.Hi, a.Wi, a.Do, a.Ho, a.Wo = 1, cin, cout, 1, H, W, 1, Ho, Wo
        a.stride, a.kd, a.k, a.dil, a.precision = s, 1, 3, 1, cv._lib.DSM_PREC_F16X2
        rows.append((name, cin, cout, s, "%dx%d" % (Ho, Wo), gflop, t_stock, t_wide, gflop / t_wide * 1e3,
                     gflop / t_wide * 1e3 / (2500.0 / 3), wbytes / t_wide * 1e-6, wbytes / t_wide * 1e-6 / 6.3,
                     err, cv.conv3d_plan_name(a)))
    return rows


def forward_rows(reps):
    rows = []
    for name in ("dispnetcorr", "iresnet"):
        torch.manual_seed(3)
        m = model_create_by_name(name, 192).cuda().eval()
        for H, W in ((384, 1280), (256, 512)):
            imL, imR = torch.randn(1, 3, H, W).cuda(), torch.randn(1, 3, H, W).cuda()
            graphs = {}
            for on in (False, True):
                old = cv.set_option("wide_conv2d", on)
                graphs[on] = GraphedForward(m, imL, imR)
                cv.set_option("wide_conv2d", old)
            eager, replay = {False: [], True: []}, {False: [], True: []}
            for _ in range(reps):
                for on in (False, True):
                    old = cv.set_option("wide_conv2d", on)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.no_grad():
                        m(imL, imR)
                    torch.cuda.synchronize()
                    eager[on].append((time.perf_counter() - t0) * 1e3)
                    cv.set_option("wide_conv2d", old)
                    t0 = time.perf_counter()
                    graphs[on].replay()
                    torch.cuda.synchronize()
                    replay[on].append((time.perf_counter() - t0) * 1e3)
            rows.append((name, "%dx%d" % (H, W), statistics.median(eager[False]), statistics.median(eager[True]),
                         statistics.median(replay[False]), statistics.median(replay[True])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide2d_bench needs the GPU")
    cv.set_option("conv_precision", "f16x2")
    lines = ["## Per layer (1 pair, 384 x 1280), stock against wide, microseconds per call from replayed graphs", "",
             "| layer | Cin->Cout, s | out | GFLOP | stock us | wide us | stock/wide | eff. TF/s | of 2500/3 | weight TB/s | of 6.3 | max diff / max | plan |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in layer_rows(args.reps):
        lines.append("| %s | %d->%d, %d | %s | %.2f | %.1f | %.1f | %.2f | %.1f | %.1f %% | %.2f | %.1f %% | %.1e | `%s` |"
                     % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[6] / r[7], r[8], 100 * r[9], r[10], 100 * r[11], r[12], r[13]))
    lines += ["", "## Whole forward, batch 1, ``wide_conv2d`` off / on alternating, milliseconds (median)", "",
              "| model | size | eager off | eager on | graph off | graph on | graph off/on |", "|---|---|---|---|---|---|---|"]
    for r in forward_rows(max(5, args.reps // 2)):
        lines.append("| %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (r + (r[4] / r[5],)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
