"""The self-supervised training step eager and from a hipGraph, at the preset shape (DispNetC, B = 4,
384x768 source, -mask: 256x640 crop; ``depthmono-mask`` of DSMnet_train_kitti-raw.sh and
``Cap_ds-mask`` of DSMnet_train_kitti.sh; default precision).  Writes profiles/selfsup_graph.md.

    python scripts/bench_selfsup_graph.py [--rounds 20] [--warmup 5] [--out profiles/selfsup_graph.md]

(a) Whole step: ``train.train_step_selfsup`` (stock Adam, and fused capturable Adam) against
    ``graphs.GraphedSelfsupStep`` in its single-process and its flat-gradient (multi-rank) form.  One
    process, every variant warmed up, the variants alternating inside every round; a round times ONE
    step of each with device events around work that ends in a synchronise, and the wall time the
    host spends inside the call (for the graphed forms: before any synchronise).  Median and spread
    over the rounds.  The eager step's kernel launches are counted once with torch's profiler.
(b) Loss alone: forward + backward of the fused pyramid loss through the host-argument and the
    device-array entry points, alternating the same way.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import train                         # noqa: E402
from dsmnet_amd.graphs import GraphedSelfsupStep     # noqa: E402
from dsmnet_amd.models import model_create_by_name   # noqa: E402

B, H, W, NEDGE = 4, 384, 768, 64


def once(fn):
    """(device ms between two events around fn + synchronise, host ms inside fn)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * (t1 - t0)


def spread(v):
    s = sorted(v)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9), "min": s[0], "max": s[-1]}


def alternate(variants, rounds, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            d, h = once(fn)
            dev[k].append(d)
            host[k].append(h)
    return {k: {"device_ms": spread(dev[k]), "host_ms": spread(host[k])} for k in variants}


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as e:                               # no profiler in this build: the table says so
        return "not counted (%s)" % type(e).__name__


def whole_step(name, rounds, warmup, batches):
    def fresh(capturable):
        torch.manual_seed(0)
        model = model_create_by_name("dispnetcorr", 192).cuda()
        lossfun = train.selfsup_losses(name, model.count_levels, 10)
        lossfun.Weight_Adjust_levels(3)                  # every level weighted
        return model, train.make_optimizer(model, capturable=capturable), lossfun
    m0, o0, l0 = fresh(False)
    m1, o1, l1 = fresh(True)
    m2, o2, l2 = fresh(True)
    m3, o3, l3 = fresh(True)
    g2 = GraphedSelfsupStep(m2, o2, l2, batches[0])
    g3 = GraphedSelfsupStep(m3, o3, l3, batches[0], flat_gradients=True)
    it = {"i": 0}

    def nxt():
        it["i"] += 1
        return batches[it["i"] % len(batches)]
    variants = {
        "eager, stock Adam": lambda: train.train_step_selfsup(m0, o0, l0, nxt()),
        "eager, fused capturable Adam": lambda: train.train_step_selfsup(m1, o1, l1, nxt()),
        "graph, single process": lambda: g2(nxt()),
        "graph, flat gradients + eager Adam": lambda: g3(nxt()),
    }
    out = alternate(variants, rounds, warmup)
    out["eager launches"] = count_launches(variants["eager, stock Adam"])
    return out


def loss_alone(name, rounds, warmup, batch):
    g = torch.Generator().manual_seed(0)
    h, w = H - 2 * NEDGE, W - 2 * NEDGE
    batch1 = torch.flip(batch, dims=[-1])
    dLs = [(torch.rand(B, 1, h >> k, w >> k, generator=g) * 40 / 2 ** k).cuda().requires_grad_() for k in range(7)]
    dL1s = [(torch.rand(B, 1, h >> k, w >> k, generator=g) * 40 / 2 ** k).cuda().requires_grad_() for k in range(7)]
    a = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, NEDGE:H - NEDGE, NEDGE:W - NEDGE], "dispLs": dLs,
         "scale_dispLs": list(range(7)), "LeftTop": [NEDGE, NEDGE], "imR1_src": batch1[:, :3],
         "imL1": batch1[:, 3:6, NEDGE:H - NEDGE, NEDGE:W - NEDGE], "dispL1s": dL1s,
         "scale_dispL1s": list(range(7)), "LeftTop1": [NEDGE, NEDGE]}
    host_args = train.selfsup_losses(name, 7, 10)
    host_args.Weight_Adjust_levels(3)
    dev_array = train.selfsup_losses(name, 7, 10)
    dev_array.Weight_Adjust_levels(3)
    dev_array.step_params = dev_array.draw_step_params(a["scale_dispLs"]).cuda()
    return alternate({"host arguments": lambda: host_args(a).backward(),
                      "device array": lambda: dev_array(a).backward()}, rounds, warmup)


def fmt(s):
    return "%.3f [%.3f – %.3f] (%.3f / %.3f)" % (s["median"], s["p10"], s["p90"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfsup_graph.md"))
    ap.add_argument("--notes", default=None, help="a markdown file appended to the tables (findings, resources)")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(3):
        left = torch.rand(B, 3, H, W, generator=g)
        batches.append(torch.cat([left, torch.roll(left, -7, dims=3)], 1).cuda())
    res = {}
    for name in ("depthmono-mask", "Cap_ds-mask"):
        res[name] = {"step": whole_step(name, args.rounds, args.warmup, batches),
                     "loss": loss_alone(name, args.rounds, args.warmup, batches[0])}
        torch.cuda.empty_cache()
    lines = ["# Self-supervised step: eager and from a hipGraph", "",
             "`python scripts/bench_selfsup_graph.py --rounds %d --warmup %d` on %s, torch %s.  DispNetC, B = %d, "
             "%dx%d source, nedge %d (%dx%d crop), every level weighted, default precision.  One process; the "
             "variants alternate inside each of the %d rounds, one step of each per round.  Cells: median "
             "[p10 – p90] (min / max), milliseconds." % (
                 args.rounds, args.warmup, torch.cuda.get_device_name(0), torch.__version__, B, H, W, NEDGE,
                 H - 2 * NEDGE, W - 2 * NEDGE, args.rounds), ""]
    for name, r in res.items():
        lines += ["## %s" % name, "", "(a) Whole step.  Device: events around the call and the synchronise that ends "
                  "it.  Host: wall time inside the call (the eager step ends in a host read of the loss; the graphed "
                  "call returns before the device is done).  Eager kernel launches per step (torch profiler): %s."
                  % r["step"]["eager launches"], "",
                  "| variant | device ms | host ms inside the call |", "|---|---|---|"]
        for k, v in r["step"].items():
            if k != "eager launches":
                lines.append("| %s | %s | %s |" % (k, fmt(v["device_ms"]), fmt(v["host_ms"])))
        lines += ["", "(b) Loss alone, forward + backward over the 7-level pyramid.", "",
                  "| entry points | device ms | host ms inside the call |", "|---|---|---|"]
        for k, v in r["loss"].items():
            lines.append("| %s | %s | %s |" % (k, fmt(v["device_ms"]), fmt(v["host_ms"])))
        lines.append("")
    if args.notes:
        lines += open(args.notes).read().rstrip("\n").split("\n") + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
