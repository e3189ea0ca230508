"""Self-supervised depthmono-mask loss at the preset shape (DSMnet_train_kitti-raw.sh: B = 4,
384x768 source, nedge 64 -> 256x640 loss crop, dispnetcorr's 7 outputs): loss forward + backward,
fused (csrc/selfsup.hip) versus the stock float32 restatement on the GPU (median of event-timed
reps after warm-up), and the whole train_step_selfsup.  Prints one JSON line.

    python scripts/bench_selfsup.py [--reps 20] [--warmup 5] [--rounds 1] [--skip-train] [--loss-name NAME]

``--loss-name Cap_ds-mask`` (or any other built Cap name) times the Cap objective of the same
kernels against its restatement (tests/cap_oracle.py): the preset of DSMnet_train_kitti.sh.
``--loss-name SsSMnet[-mask]`` or ``common[-mask]`` times those objectives
(``train.selfsup_losses``) against tests/sssmnet_oracle.py.  ``--rounds N`` alternates fused and stock N times in the one process
and reports every round's medians next to their median (profiles/sssmnet.md).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import train                    # noqa: E402
from dsmnet_amd.models import model_create_by_name   # noqa: E402
from tests import cap_oracle as CO              # noqa: E402
from tests import selfsup_oracle as SO          # noqa: E402
from tests import sssmnet_oracle as XO          # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--loss-name", default="depthmono-mask")
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    B, H, W, nedge = 4, 384, 768, 64
    h, w = H - 2 * nedge, W - 2 * nedge
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(B, 6, H, W, generator=g).cuda()
    batch1 = torch.flip(batch, dims=[-1])
    dLs = [(torch.rand(B, 1, h >> k, w >> k, generator=g) * 40 / 2 ** k).cuda().requires_grad_() for k in range(7)]
    dL1s = [(torch.rand(B, 1, h >> k, w >> k, generator=g) * 40 / 2 ** k).cuda().requires_grad_() for k in range(7)]
    try:
        lossfun = train.losses(args.loss_name, 7, 10)
    except NotImplementedError:                     # the names only the subclass opens
        lossfun = train.selfsup_losses(args.loss_name, 7, 10)
    lossfun.Weight_Adjust_levels(3)                 # every level weighted (0.01 or more)
    a = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:H - nedge, nedge:W - nedge], "dispLs": dLs,
         "scale_dispLs": list(range(7)), "LeftTop": [nedge, nedge], "imR1_src": batch1[:, :3],
         "imL1": batch1[:, 3:6, nedge:H - nedge, nedge:W - nedge], "dispL1s": dL1s,
         "scale_dispL1s": list(range(7)), "LeftTop1": [nedge, nedge]}

    def fused():
        lossfun(a).backward()

    def stock():
        rest = (a["imR_src"], a["imL"], dLs, a["scale_dispLs"], a["LeftTop"], a["imR1_src"], a["imL1"], dL1s,
                a["LeftTop1"])
        if "depthmono" in args.loss_name:
            loss, _ = SO.losses_pyramid1(lossfun.weight_levels, lossfun.flag_mask, *rest, dtype=torch.float32)
        elif "sssmnet" in args.loss_name.lower() or "common" in args.loss_name.lower():
            loss, _ = XO.losses_pyramid("sssmnet" if "sssmnet" in args.loss_name.lower() else "common",
                                        lossfun.weight_levels, lossfun.flag_mask, *rest, dtype=torch.float32)
        else:
            loss, _ = CO.losses_pyramid1(lossfun.weight_levels, lossfun.flag_mask, CO.terms_of(args.loss_name),
                                         *rest, dtype=torch.float32)
        loss.backward()

    rounds = [(timed(fused, args.reps, args.warmup), timed(stock, args.reps, args.warmup))
              for _ in range(max(1, args.rounds))]
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"loss_name": args.loss_name, "shape": [B, H, W], "nedge": nedge, "levels": 7, "reps": args.reps,
           "loss_fwd_bwd_ms": {"fused": med([r[0] for r in rounds]), "stock_fp32": med([r[1] for r in rounds])}}
    out["loss_fwd_bwd_ms"]["speedup"] = out["loss_fwd_bwd_ms"]["stock_fp32"] / out["loss_fwd_bwd_ms"]["fused"]
    if args.rounds > 1:
        out["loss_fwd_bwd_ms"]["rounds"] = {"fused": [r[0] for r in rounds], "stock_fp32": [r[1] for r in rounds]}
    if not args.skip_train:
        torch.manual_seed(0)
        model = model_create_by_name("dispnetcorr", 192).cuda()
        opt = train.make_optimizer(model)
        out["train_step_selfsup_ms"] = timed(lambda: train.train_step_selfsup(model, opt, lossfun, batch),
                                             max(5, args.reps // 2), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
