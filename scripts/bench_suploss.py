"""Supervised pyramid loss alone, forward + backward, stock torch ops (option off) against the
fused op (csrc/suploss.hip, option on) in ONE process, alternating the two so that both see the
same machine; then one hipGraph-replayed PSMNet training step (graphs.GraphedTrainStep, 256x512,
batch 1) with the option off and on.  Event-timed after warm-up; median and min..max of the
repeats.  Also the HBM floor of the fused form: gt once per pass and item, the coarse maps (and
their gradients), 4 B per pixel per item of saved state each way.  Prints one JSON line.

    python scripts/bench_suploss.py [--reps 30] [--warmup 5] [--skip-train]
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import costvolume as cv          # noqa: E402
from dsmnet_amd import train                     # noqa: E402

HBM_BYTES_PER_S = 8.0e12                         # MI355X peak


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


def loss_case(name, gt_shape, pred_shapes, levels, count_levels, epoch, reps, warmup):
    g = torch.Generator().manual_seed(0)
    gt = (torch.rand(*gt_shape, generator=g) * 60 - 10).cuda()            # about 1/6 without ground truth
    preds = [(torch.rand(*s, generator=g) * 50).cuda().requires_grad_() for s in pred_shapes]
    lf = train.losses("supervised", count_levels, 37)
    lf.Weight_Adjust_levels(epoch)
    args = {"disp_gt": gt, "disps": preds, "scale_disps": levels, "flag_smooth": True}

    def run(on):
        old = cv.set_option("fused_supervised_loss", on)
        try:
            loss = lf(args)
            loss.backward()
        finally:
            cv.set_option("fused_supervised_loss", old)
        return loss

    vals = {on: float(run(on)) for on in (False, True)}
    for _ in range(warmup):
        run(False)
        run(True)
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):                                       # alternate
            for p in preds:
                p.grad = None
            ts[on].append(one(lambda: run(on)))
    n_items = len(preds)
    coarse = sum(p.numel() for p in preds)
    floor_bytes = 4.0 * (n_items * gt.numel() + coarse + n_items * gt.numel()      # forward: gt, maps, saved state
                         + n_items * gt.numel() + coarse)                          # backward: saved state, gradients
    return {"case": name, "gt": list(gt_shape), "items": n_items, "levels": levels,
            "loss_stock": vals[False], "loss_fused": vals[True],
            "stock": stats(ts[False]), "fused": stats(ts[True]),
            "hbm_floor_ms": floor_bytes / HBM_BYTES_PER_S * 1e3, "hbm_floor_bytes": floor_bytes}


def graphed_step(reps, warmup):
    from dsmnet_amd.graphs import GraphedTrainStep
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    base = model_create_by_name("psmnet", 192).cuda()
    for i in (1, 2, 3):
        with torch.no_grad():
            getattr(base, "classif%d" % i)[2].weight.mul_(1e-3)
    left = torch.rand(1, 3, 256, 512, device="cuda")
    disp = torch.full((1, 1, 256, 512), 6.0, device="cuda")
    batch = torch.cat([left, torch.roll(left, -6, dims=3), disp], 1)
    steps = {}
    for on in (False, True):
        old = cv.set_option("fused_supervised_loss", on)
        try:
            m = copy.deepcopy(base)
            lf = train.losses("supervised", 1, 0)
            lf.Weight_Adjust_levels(0)
            opt = torch.optim.Adam(m.parameters(), lr=1e-4, capturable=True, fused=True)
            steps[on] = GraphedTrainStep(m, opt, lf, batch, warmup=2)
        finally:
            cv.set_option("fused_supervised_loss", old)
    for _ in range(warmup):
        for on in (False, True):
            steps[on](batch)
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            ts[on].append(one(lambda: steps[on](batch)))
    return {"shape": [1, 256, 512], "model": "psmnet", "stock": stats(ts[False]), "fused": stats(ts[True])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_suploss.py measures on the GPU: none found")
    out = {"reps": a.reps, "cases": [
        loss_case("psmnet 3 x (4,540,960)", (4, 1, 540, 960), [(4, 540, 960)] * 3, [0, 0, 0], 1, 0, a.reps, a.warmup),
        loss_case("dispnetc 7 levels (4,1,256,640)", (4, 1, 256, 640),
                  [(4, 1, 256 >> k, 640 >> k) for k in range(7)], list(range(7)), 7, 10, a.reps, a.warmup),
        loss_case("psmnet 3 x (1,256,512)", (1, 1, 256, 512), [(1, 256, 512)] * 3, [0, 0, 0], 1, 0, a.reps, a.warmup)]}
    if not a.skip_train:
        out["graphed_train_step"] = graphed_step(max(5, a.reps // 3), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
