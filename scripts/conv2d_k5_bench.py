"""profiles/conv2d_k5.md: the 5x5 stride-2 layers (csrc/conv_wide2d.hpp with a 5x5 window, plan kind 10) against
the stock layer, on one GPU, in one process, the two alternating.

    python scripts/conv2d_k5_bench.py [--out profiles/conv2d_k5.md] [--reps 10] [--resources remarks.txt]

Per layer (DispNet's conv2 and conv3a at 384 x 1280 and 256 x 512): 20 calls captured into one hipGraph per
variant (device time without the Python launch path), the graphs replayed alternately; the figure is the
median over the rounds of (replay time / 20).
  stock: F.relu(F.conv2d(x, w, b, 2, 2)) on the NCHW map, as Sequential(Conv2d, ReLU) runs it;
  k5:    costvolume.conv2d_block(k=5) on the NHWC map that carries its absolute maximum (both launches of a
         K-split layer and the amax slot's fill included).
Whole forwards: DispNet and DispNetC, ``conv2d_k5`` off / on alternating with ``wide_conv2d`` on in both, eager
(host clock around a synchronise) and replayed from a captured graph (dsmnet_amd.graphs.GraphedForward); the
layout conversion and the absmax pass in front of conv2 are inside these figures.
Compiler figures: ``--resources`` names a file with the remarks of
``hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c dsmnet_amd/csrc/conv_f16.hip``
(standard error); without it the script runs that command itself.  Needs the GPU: there is no CPU fallback."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsmnet_amd import costvolume as cv                      # noqa: E402
from dsmnet_amd.graphs import GraphedForward                 # noqa: E402
from dsmnet_amd.models import model_create_by_name           # noqa: E402

# name, Cin, Cout, image size, input (H, W) of the layer
LAYERS = [("conv2", 64, 128, "384x1280", (192, 640)), ("conv3a", 128, 256, "384x1280", (96, 320)),
          ("conv2", 64, 128, "256x512", (128, 256)), ("conv3a", 128, 256, "256x512", (64, 128))]
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
    for name, cin, cout, size, (H, W) in LAYERS:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(1, cin, H, W, generator=g).relu().cuda()
        w = (torch.randn(cout, cin, 5, 5, generator=g) * (2.0 / (25 * cin)) ** 0.5).cuda()
        b = (torch.randn(cout, generator=g) * 0.1).cuda()
        xcl = x.contiguous(memory_format=torch.channels_last)
        cv.absmax(xcl)
        packed, ones = cv.pack_conv2d_weight(w), torch.ones(cout, device="cuda")

        def stock():
            return F.relu(F.conv2d(x, w, b, 2, 2))

        def k5():
            with cv.amax_scope(x.device):
                return cv.conv2d_block(xcl, packed, cout, ones, b, stride=2, relu=1, k=5)

        err = (k5().float() - stock()).abs().max().item() / stock().abs().max().item()
        t_stock, t_k5 = replay_us([graph_of(stock), graph_of(k5)], reps)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        gflop = 2.0 * 25 * cin * cout * Ho * Wo / 1e9
        a = cv._lib.Conv3dArgs()
        a.x = a.w_packed = a.y = a.x_amax = 16
        a.B, a.Cin, a.Cout, a.Di, a.Hi, a.Wi, a.Do, a.Ho, a.Wo = 1, cin, cout, 1, H, W, 1, Ho, Wo
        a.stride, a.kd, a.k, a.dil, a.precision = 2, 1, 5, 1, cv._lib.DSM_PREC_F16X2
        rows.append((name, size, cin, cout, "%dx%d" % (Ho, Wo), gflop, t_stock, t_k5, t_stock / t_k5,
                     gflop / t_stock * 1e3, gflop / t_k5 * 1e3, err, cv.conv3d_plan_name(a)))
    return rows


def forward_rows(reps):
    rows = []
    for name in ("dispnet", "dispnetcorr"):
        torch.manual_seed(3)
        m = model_create_by_name(name, 192).cuda().eval()
        for H, W in ((384, 1280), (256, 512)):
            imL, imR = torch.randn(1, 3, H, W).cuda(), torch.randn(1, 3, H, W).cuda()
            graphs = {}
            for on in (False, True):
                old = cv.set_option("conv2d_k5", on)
                graphs[on] = GraphedForward(m, imL, imR)
                cv.set_option("conv2d_k5", old)
            eager, replay = {False: [], True: []}, {False: [], True: []}
            for _ in range(reps):
                for on in (False, True):
                    old = cv.set_option("conv2d_k5", on)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.no_grad():
                        m(imL, imR)
                    torch.cuda.synchronize()
                    eager[on].append((time.perf_counter() - t0) * 1e3)
                    cv.set_option("conv2d_k5", old)
                    t0 = time.perf_counter()
                    graphs[on].replay()
                    torch.cuda.synchronize()
                    replay[on].append((time.perf_counter() - t0) * 1e3)
            rows.append((name, "%dx%d" % (H, W), statistics.median(eager[False]), statistics.median(eager[True]),
                         statistics.median(replay[False]), statistics.median(replay[True])))
    return rows


def resource_rows(path):
    """(kernel, SGPRs, SGPR spills, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD) of every instantiation of
    the kernel in the compiler's remarks; the 5x5 ones are <PM, false, 5>."""
    if path is None:
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3",
                                "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                os.path.join(ROOT, "dsmnet_amd", "csrc", "conv_f16.hip"), "-o",
                                os.path.join(tmp, "conv_f16.o")], capture_output=True, text=True, check=True)
        text = r.stderr
    else:
        with open(path) as f:
            text = f.read()
    rows, cur = [], None
    keys = ("TotalSGPRs", "SGPRs Spill", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)} if "conv_wide2d_kernel" in m.group(1) else None
            if cur is not None:
                rows.append(cur)
            continue
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in keys:
            cur[m.group(1)] = m.group(2)
    out = []
    for r in rows:
        m = re.search(r"conv_wide2d_kernelILi(\d)ELb(\d)(?:ELi(\d))?E", r["name"])
        pm, tr, k = int(m.group(1)), int(m.group(2)), int(m.group(3) or 3)
        label = "conv_wide2d_kernel<%s, %s, K=%d>" % ("f16x2" if pm == 2 else "f16", "transposed" if tr else "forward", k)
        out.append((label,) + tuple(r.get(key, "?") for key in keys))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv2d_k5_bench needs the GPU")
    cv.set_option("conv_precision", "f16x2")
    cv.set_option("wide_conv2d", True)
    lines = ["# 5x5 stride-2 layers on the MFMA kernel (`conv2d_k5`) against the stock layer", "",
             "Written by `scripts/conv2d_k5_bench.py` (%s, torch %s), precision f16x2." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "## Per layer (1 pair), microseconds per call from replayed graphs of %d calls, median of %d rounds" % (CALLS, args.reps), "",
             "| layer | image | Cin->Cout | out | GFLOP | stock us | k5 us | stock/k5 | stock eff. TF/s | k5 eff. TF/s | max diff / max | plan |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for r in layer_rows(args.reps):
        lines.append("| %s | %s | %d->%d | %s | %.2f | %.1f | %.1f | %.2f | %.1f | %.1f | %.1e | `%s` |" % r)
        if r[8] < 1.0:
            slower.append("%s at %s (%d->%d): %.2fx" % (r[0], r[1], r[2], r[3], r[8]))
    lines += ["", "Layers slower than the stock layer: %s." % ("; ".join(slower) if slower else "none")]
    lines += ["", "## Whole forward, batch 1, `wide_conv2d` on, `conv2d_k5` off / on alternating, milliseconds (median of %d)" % max(5, args.reps // 2), "",
              "| model | size | eager off | eager on | graph off | graph on | graph off/on |", "|---|---|---|---|---|---|---|"]
    for r in forward_rows(max(5, args.reps // 2)):
        lines.append("| %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (r + (r[4] / r[5],)))
    lines += ["", "## Compiler resource figures (`-Rpass-analysis=kernel-resource-usage`, gfx950), `__launch_bounds__(512, 2)`", "",
              "Dynamic LDS: 122,944 B (f16x2), 73,792 B (f16): two staged images of 768 slots and the reduction words.", "",
              "| kernel | SGPRs | SGPR spills (to VGPR lanes) | VGPRs | AGPRs | scratch B/lane | waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for r in resource_rows(args.resources):
        lines.append("| `%s` | %s | %s | %s | %s | %s | %s |" % r)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
