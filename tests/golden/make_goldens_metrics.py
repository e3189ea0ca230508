#!/usr/bin/env python3
"""Generate tests/golden/golden_metrics.npz from the REFERENCE's utils/evaluate.py itself.

Runs only where the reference tree exists (never on the GPU box).  As make_goldens_cap.py does:
``utils/imwrap.py`` is executed from its text as a module, and the lines of ``utils/evaluate.py``
that still run on today's torch and numpy are executed from the file text (``ref_lines`` of
make_goldens.py): :14-20 the D1 / EPE head of ``evaluate``, :36-44 ``imwrap_pixel_errors`` and
:46-73 ``compute_errors``.  The textual shims are the generators' usual ones: ``.data[0]`` ->
``.item()`` and a one-argument ``to_tensor`` (the file's own import of ``util`` is broken).
evaluate.py:26-32, the photometric tail of ``evaluate``, indexes a (B,C,H,W) tensor with a
(B,1,H,W) mask and cannot run; its number is the restatement's alone (tests/metrics_oracle.py).

The numpy lines get float32 arrays (what the reference's loaders hand them), the warp lines
float64 tensors; torch's CPU generator is seeded before each warp, so the reference's own
``torch.rand(1)`` epsilon is reproducible.  Inputs: tests/metrics_oracle.py ``make_inputs`` at
2x3x37x300 -- ground truth in [1,60] with 30 % holes, predictions gt * (0.5 .. 2.4) +- 0.2 moved
away from every counted threshold (the precondition is asserted here in float64), independent
smooth-noise images.

The script REFUSES to write if the restatement disagrees with the reference by more than 1e-6
relative on any number.

Usage:  python tests/golden/make_goldens_metrics.py
"""
import json
import os
import sys
import textwrap
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL       # noqa: E402
from tests import metrics_oracle as MO          # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402

warnings.filterwarnings("ignore")

SEED, B, C, H, W = 401, 2, 3, 37, 300


def load_reference():
    imwrap_mod = RL._exec_text("ref_imwrap", os.path.join(RL.REFERENCE_ROOT, "utils", "imwrap.py"))
    ns = {"np": np, "torch": torch, "imwrap_BCHW": imwrap_mod.imwrap_BCHW,
          "to_tensor": lambda x: torch.as_tensor(x)}
    head = "def evaluate_head(dispL, dispL_gt):\n" + textwrap.indent(ref_lines("utils/evaluate.py", 14, 20), "    ") \
        + "    return d1, epe\n"
    exec(head, ns)
    exec(ref_lines("utils/evaluate.py", 36, 44).replace(".data[0]", ".item()"), ns)
    exec(ref_lines("utils/evaluate.py", 46, 73), ns)
    return ns


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    ref = load_reference()
    imgs, gt, pred = MO.make_inputs(SEED, B, C, H, W)
    raw, _ = MO.condition(pred, gt)
    assert MO.precondition_holds(pred, gt) and torch.equal(raw, pred)
    assert float(pred.min()) > 0 and 0.2 < float((gt > 0).double().mean()) < 0.8
    imL, imR = MO.images_of(imgs)

    # the reference's numbers
    want = {}
    d1, epe = ref["evaluate_head"](pred.numpy(), gt.numpy())
    want["d1"], want["epe"] = float(d1), float(epe)
    names = ("abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3")
    for k, v in zip(names, ref["compute_errors"](gt.numpy(), pred.numpy())):
        want[k] = float(v)
    torch.manual_seed(SEED)
    want["pixelerror_elem"] = float(ref["imwrap_pixel_errors"](imL.double(), imR.double(), pred.double()))

    # the restatement
    torch.manual_seed(SEED)
    delt = MO.SO.draw_delt()
    sums = MO.sums(pred, gt, imL, imR, delt, negate_warp=True)
    mine = {k: float(v) for k, v in MO.finish(sums, (C, H, W)).items()}
    print("metrics goldens (reference lines executed from the file text)")
    for k in sorted(want):
        e = rel(mine[k], want[k])
        print("  %-16s reference %.10g  restatement %.10g  rel %.2e" % (k, want[k], mine[k], e))
        if not e <= 1e-6:
            raise SystemExit("restatement disagrees with the reference on %s" % k)
    if not mine["pixelerror"] / 255.0 >= 0.1:
        raise SystemExit("the images are meant to differ: mean |imL - w| = %g" % (mine["pixelerror"] / 255.0))
    print("  %-16s (restatement only) %.10g" % ("pixelerror", mine["pixelerror"]))

    store = {"imgs": imgs.numpy(), "gt": gt.numpy(), "pred": pred.numpy(), "delt": np.float64(delt),
             "sums": sums.numpy(), "keys": np.frombuffer(json.dumps(sorted(want)).encode(), dtype=np.uint8),
             "reference": np.array([want[k] for k in sorted(want)], dtype=np.float64),
             "pixelerror": np.float64(mine["pixelerror"])}
    meta = {"torch": torch.__version__, "numpy": np.__version__, "seed": SEED, "shape": [B, C, H, W],
            "negate_warp": True, "reference": "sunshinnnn/DSMnet utils/evaluate.py, utils/imwrap.py"}
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_metrics.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
