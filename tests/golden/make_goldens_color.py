#!/usr/bin/env python3
"""Generate tests/golden/golden_color.npz from the REFERENCE's colour transforms themselves.

Runs only where the reference tree exists (never on the GPU box).  ``myTransforms/aug_color.py`` is
executed from its text as a module; the lines of ``myTransforms/__init__.py`` that build the stereo
transforms (:8 the ImageNet mean / std, :11-14 Normalize_Imagenet, :109-114 Stereo_color, :121-124
Stereo_normalize, :131-137 Stereo_color_batch) are executed from the file text, with a
``transforms.Compose`` that applies its list in turn (torchvision's, which is all the reference
uses of it).  torch 2.x only warns at aug_color.py's ``add_(Number, Tensor)`` form.

Everything runs on the CPU in float32, the training dtype, with ``random.seed`` and
``torch.manual_seed`` fixed before each batch: Lighting's ``normal_`` then draws from the CPU
generator in float32, as the product's planner does when handed a CPU device.  The cases include a
dark region, where Contrast (u < 0) or Saturation before Gamma leaves negative values and the
reference's ``x ** (1 + u)`` yields NaN; the fixture keeps those NaNs.

The script REFUSES to write if the restatement (tests/color_oracle.py, with its reference-NaN
switch), fed by the planner seeded the same way, disagrees with the reference by more than 2e-6
absolute or puts NaN anywhere else.

Usage:  python tests/golden/make_goldens_color.py
"""
import json
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL       # noqa: E402
from tests import color_oracle as CO            # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402

warnings.filterwarnings("ignore")


class _Compose(object):
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, img):
        for t in self.ts:
            img = t(img)
        return img


def load_reference():
    aug = RL._exec_text("ref_aug_color", os.path.join(RL.REFERENCE_ROOT, "myTransforms", "aug_color.py"))
    ns = {"torch": torch, "transforms": types.SimpleNamespace(Compose=_Compose),
          "Normalize": aug.Normalize, "Lighting": aug.Lighting, "ColorJitter": aug.ColorJitter}
    for a, b in ((8, 8), (11, 14), (109, 114), (121, 124), (131, 137)):
        exec(ref_lines("myTransforms/__init__.py", a, b), ns)
    return ns


def inputs(seed, B, C, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g)
    x[:, :6, : H // 2, : W // 3] *= 0.08                     # dark region: Gamma after a negative shift
    x[:, :6, -1, :4] = 0.0                                   # exact 0 and 1
    x[:, :6, -1, 4:8] = 1.0
    if C > 6:
        x[:, 6:] = torch.rand(B, C - 6, H, W, generator=g) * 50   # a disparity channel
    return x


def check(name, x, want, planned):
    """planned: the product's launches for this batch, drawn with the same seeds."""
    got = x.double()
    for recs, alpha, G in planned:
        got = CO.restate(got, recs, alpha, G, reference_nan=True)
    w = want.double()
    nan_w, nan_g = torch.isnan(w), torch.isnan(got)
    if not torch.equal(nan_w, nan_g):
        raise SystemExit("%s: NaN pattern differs (%d reference vs %d restatement)"
                         % (name, int(nan_w.sum()), int(nan_g.sum())))
    err = (got[~nan_w] - w[~nan_w]).abs().max().item()
    print("  %-16s max |restatement - reference| %.2e, %d NaN" % (name, err, int(nan_w.sum())))
    if err > 2e-6:
        raise SystemExit("restatement disagrees with the reference on %s" % name)
    return int(nan_w.sum())


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    from dsmnet_amd import transforms as T
    ref = load_reference()
    store, meta = {}, {"torch": torch.__version__, "cases": {},
                       "reference": "sunshinnnn/DSMnet myTransforms/aug_color.py, myTransforms/__init__.py"}
    print("colour goldens (float32 CPU, reference lines executed from the file text)")
    nans = 0
    for case, shape, seed, kind in (("same", (3, 7, 24, 40), 11, "color_same"),
                                    ("split", (3, 6, 20, 37), 12, "color_split"),
                                    ("normalize", (2, 7, 16, 24), 13, "normalize")):
        x = inputs(seed, *shape)
        if kind == "normalize":
            ref_t, mine = ref["Stereo_normalize"](), T.Stereo_normalize()
        else:
            same = kind == "color_same"
            ref_t, mine = ref["Stereo_color"](same_group=same), T.Stereo_color(same_group=same)
        random.seed(seed)
        torch.manual_seed(seed)
        want = ref["Stereo_color_batch"](x.clone(), ref_t)
        random.seed(seed)
        torch.manual_seed(seed)
        planned = mine.plan(shape[0], shape[1], "cpu")
        nans += check(case, x, want, planned)
        store[case + ".x"] = x.numpy()
        store[case + ".out"] = want.numpy()
        meta["cases"][case] = {"seed": seed, "kind": kind, "shape": list(shape)}
    if nans == 0:
        raise SystemExit("no case reached the reference's NaN: the dark region no longer tests the drift")
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_color.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
