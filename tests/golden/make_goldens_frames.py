#!/usr/bin/env python3
"""Generate tests/golden/golden_frames.npz from the REFERENCE's dataset class itself.

Runs only where the reference tree exists (never on the GPU box).
``myDatasets_stereo/Dataset_stereo.py`` is executed from its text as a module.  Its
``from img_rw import imread, load_disp`` gets a stub module: the reference's img_rw imports cv2,
which is not installed here, and the samples are in memory anyway -- a "path" is a key into a
dict of seeded arrays of unequal sizes (8-bit RGB, 16-bit and float32 disparities).  So the crop,
the float conversion, the concatenation and the flip are the reference's own; the decoding is not
exercised.

The script REFUSES to write unless
  * ``tests/frames_oracle.getitem``, seeded alike, equals the reference bit for bit on every
    sample and leaves ``np.random`` in the same state;
  * the Train cases contain a flipped and an unflipped 8-channel sample, and the 7-channel case
    draws nothing.

Only numbers are stored.  Usage:  python tests/golden/make_goldens_frames.py
"""
import json
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL       # noqa: E402
from tests import frames_oracle as FO           # noqa: E402

SIZES = ((13, 41), (12, 44), (14, 40))           # size_min = [12, 40]; crop origins (1,0), (0,2), (2,0)
SIZE_MIN = [12, 40]
# name, planes per sample, Train, seed
CASES = (("c8_train", 4, True, 5), ("c8_eval", 4, False, 5), ("c7_train", 3, True, 5), ("c6_train", 2, True, 6))


def samples():
    rng = np.random.RandomState(77)
    out = {}
    for i, (h, w) in enumerate(SIZES):
        out["s%d.imL" % i] = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        out["s%d.imR" % i] = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        for side in ("dispL", "dispR"):
            d = rng.randint(0, 40 * 256, size=(h, w)).astype(np.uint16)
            d[rng.rand(h, w) < 0.2] = 0
            out["s%d.%s" % (i, side)] = d
    return out


def load_reference(store):
    stub = types.ModuleType("img_rw")
    stub.imread = stub.load_disp = lambda key: store[key]
    had = sys.modules.get("img_rw")
    sys.modules["img_rw"] = stub
    try:
        mod = RL._exec_text("ref_dataset_stereo", os.path.join(RL.REFERENCE_ROOT, "myDatasets_stereo", "Dataset_stereo.py"))
    finally:
        if had is None:
            del sys.modules["img_rw"]
        else:
            sys.modules["img_rw"] = had
    logging.getLogger().setLevel(logging.WARNING)        # the module switches the root logger to DEBUG
    return mod


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    store = samples()
    ref = load_reference(store)
    n = len(SIZES)
    kinds = ("imL", "imR", "dispL", "dispR")
    out = dict(store)
    meta = {"numpy": np.__version__, "size_min": SIZE_MIN, "sizes": [list(s) for s in SIZES], "cases": {},
            "reference": "sunshinnnn/DSMnet myDatasets_stereo/Dataset_stereo.py (loaders injected)"}
    seen = {"flip": 0, "noflip": 0}
    for name, planes, train, seed in CASES:
        lists = [["s%d.%s" % (i, k) for i in range(n)] for k in kinds[:planes]] + [None] * (4 - planes)
        ds = ref.Dataset_stereo(lists[0], lists[1], lists[2], lists[3], size_min=list(SIZE_MIN), Train=train)
        np.random.seed(seed)
        want = [ds[i] for i in range(n)]
        nxt = float(np.random.rand())
        np.random.seed(seed)
        mine = [FO.getitem([store["s%d.%s" % (i, k)] for k in kinds[:planes]], SIZE_MIN, train, FO.DISP_U16)
                for i in range(n)]
        if float(np.random.rand()) != nxt:
            raise SystemExit("%s: the oracle leaves np.random in another state" % name)
        for i in range(n):
            img, fname = want[i]
            if img.dtype != np.float32 or img.shape != (SIZE_MIN[0], SIZE_MIN[1], planes + 4) or fname != lists[0][i]:
                raise SystemExit("%s[%d]: unexpected %s %s %r" % (name, i, img.dtype, img.shape, fname))
            if not np.array_equal(img, mine[i][0]):
                raise SystemExit("%s[%d]: the oracle differs from the reference" % (name, i))
        flips = [bool(m[1]) for m in mine]
        if name == "c8_train":
            seen["flip"] += sum(flips)
            seen["noflip"] += n - sum(flips)
        if name == "c7_train":
            np.random.seed(seed)
            if nxt != float(np.random.rand()):
                raise SystemExit("c7_train drew a random number")
        out[name + ".out"] = np.stack([w[0] for w in want])
        out[name + ".next_rand"] = np.float64(nxt)
        meta["cases"][name] = {"planes": planes, "train": train, "seed": seed, "flips": flips}
        print("  %-9s C %d  flips %s" % (name, planes + 4, flips))
    if not all(seen.values()):
        raise SystemExit("the seed does not reach both a flipped and an unflipped sample: %s" % seen)
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_frames.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
