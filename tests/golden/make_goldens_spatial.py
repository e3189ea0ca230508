#!/usr/bin/env python3
"""Generate tests/golden/golden_spatial.npz from the REFERENCE's spatial transform itself.

Runs only where the reference tree exists (never on the GPU box).  ``myTransforms/aug_spatial.py``
and ``aug_color.py`` are executed from their text as modules; the lines of
``myTransforms/__init__.py`` that build the stereo pipelines (:8 the ImageNet mean / std, :11-14
Normalize_Imagenet, :88-95 Stereo_train, :103-107 Stereo_Spatial) are executed from the file text
with a ``transforms.Compose`` that applies its list in turn.

cv2 is not installed here.  aug_spatial.py's ``import cv2`` gets a stub whose ``resize`` is
``tests/spatial_oracle.resize_linear``, cv2's linear resize stated as a rule.  THAT THIS RULE
EQUALS THE cv2 BINARY IS NOT MEASURED ANYWHERE; the fixture's metadata says so.  The crop-only
cases (scale_delt == 0) never reach ``resize``: their goldens are the reference's own output.

Everything runs on the CPU in float32.  ``np.random.seed`` (the spatial draws) and
``torch.manual_seed`` (Lighting's ``normal_`` of Stereo_train, CPU generator) are fixed before
each batch, and the frames go through the pipeline one by one, as a dataset would.  The reference
shifts its input in place, so every frame is handed over as a copy.

The script REFUSES to write unless
  * the scale cases include both a final scale > 1 and < 1, and at least one scale_adjust > 1;
  * the crop cases include a shift of 0 and a shift > 0;
  * the product's planner (dsmnet_amd.transforms), seeded alike, makes exactly the reference's
    ``np.random`` calls with the same results, leaves ``scale_rand`` / ``shift_max`` on the object
    as the reference does, and leaves ``np.random`` in the same state;
  * ``spatial_oracle.restate`` of the planner's records equals the reference bit for bit
    (crop-only), or within 4 * 2^-23 * M (scale; M = the pixel's largest tap, output units).

Usage:  python tests/golden/make_goldens_spatial.py
"""
import json
import os
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
from tests import spatial_oracle as SO          # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402

warnings.filterwarnings("ignore")

CV2_NOTE = ("cv2 is not installed where this fixture is written: the scale cases ran the reference with "
            "cv2.resize replaced by tests/spatial_oracle.resize_linear (cv2's linear rule restated); that "
            "the rule equals the cv2 binary is NOT measured.  The crop-only cases call no stubbed code.")

# name, frames key, size_crop [w, h], scale_delt, shift_max, seed, store the Stereo_train output too
FRAMES = {"a": (3, 23, 37, 8), "b": (2, 20, 31, 7), "c": (2, 17, 29, 6)}
CASES = (("crop_a", "a", [16, 12], 0, 5, 3, True),
         ("crop_b", "b", [16, 12], 0, 5, 2, False),
         ("crop_c", "c", [16, 12], 0, 5, 3, False),
         ("scale_a", "a", [16, 12], 0.5, 5, 4, True),
         ("scale_b", "b", [16, 12], 0.5, 5, 5, False),
         ("scale_c", "c", [16, 12], 0.5, 5, 6, False),
         ("scale_big_c", "c", [32, 20], 0.5, 5, 7, False))     # crop larger than the frame: scale_adjust > 1


class _Compose(object):
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, img):
        for t in self.ts:
            img = t(img)
        return img


class _Recorder(object):
    """Stands in for ``np.random`` in a module's ``np``: forwards and logs every call."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fn = getattr(np.random, name)

        def call(*args):
            v = fn(*args)
            self.log.append((name, [float(a) for a in args], float(v)))
            return v
        return call


def _np_with(recorder):
    return types.SimpleNamespace(random=recorder, ndarray=np.ndarray)


def load_reference(recorder):
    stub = types.ModuleType("cv2")
    stub.resize, stub.INTER_LINEAR = SO.resize_linear, 1
    had = sys.modules.get("cv2")
    sys.modules["cv2"] = stub
    try:
        spatial = RL._exec_text("ref_aug_spatial", os.path.join(RL.REFERENCE_ROOT, "myTransforms", "aug_spatial.py"))
    finally:
        if had is None:
            del sys.modules["cv2"]
        else:
            sys.modules["cv2"] = had
    spatial.np = _np_with(recorder)
    aug = RL._exec_text("ref_aug_color_sp", os.path.join(RL.REFERENCE_ROOT, "myTransforms", "aug_color.py"))
    ns = {"torch": torch, "transforms": types.SimpleNamespace(Compose=_Compose),
          "Normalize": aug.Normalize, "Lighting": aug.Lighting, "ToTensor_numpy": aug.ToTensor_numpy,
          "Spatial_stereo": spatial.Spatial_stereo}
    for a, b in ((8, 8), (11, 14), (88, 95), (103, 107)):
        exec(ref_lines("myTransforms/__init__.py", a, b), ns)
    return ns


def frames(key):
    B, H, W, C = FRAMES[key]
    rng = np.random.RandomState(100 + ord(key))
    x = rng.randint(0, 256, size=(B, H, W, C)).astype(np.float32)        # 8-bit images, 0..255
    for c in range(6, C):
        d = rng.randint(-160, 1601, size=(B, H, W)).astype(np.float32) / 8     # -20 .. 200, steps of 1/8
        d[rng.rand(B, H, W) < 0.2] = 0.0                                   # invalid pixels: exact zeros
        x[..., c] = d
    return x


def run_reference(ref, factory, x, args, seed, recorder):
    """The batch through the reference pipeline frame by frame.  Returns the outputs, the np.random
    calls per frame, scale_rand after each frame, the final shift_max and the next np.random.rand()."""
    t = ref[factory](*args)
    np.random.seed(seed)
    torch.manual_seed(seed)
    outs, logs, scales = [], [], []
    for b in range(x.shape[0]):
        del recorder.log[:]
        outs.append(t(x[b].copy()).numpy())
        logs.append(list(recorder.log))
        scales.append(float(t.ts[0].scale_rand))
    return np.stack(outs), logs, scales, int(t.ts[0].shift_max), float(np.random.rand())


def run_planner(T, factory, x, args, seed, recorder):
    t = getattr(T, factory)(*args)
    np.random.seed(seed)
    torch.manual_seed(seed)
    B, H0, W0, C = x.shape
    hw = t.spatial.out_hw(H0, W0)
    records, logs, scales = [], [], []
    for b in range(B):                                  # plan_spatial's loop, one frame at a time for the log
        del recorder.log[:]
        records.append(t.spatial.draw(H0, W0))
        logs.append(list(recorder.log))
        scales.append(float(t.spatial.scale_rand))
    color = t.plan(B, C, "cpu")
    return records, hw, color, logs, scales, int(t.spatial.shift_max), float(np.random.rand())


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    from dsmnet_amd import transforms as T
    rec_ref, rec_mine = _Recorder(), _Recorder()
    ref = load_reference(rec_ref)
    real_np = T.np
    T.np = types.SimpleNamespace(random=rec_mine)
    store = {"frames." + k: frames(k) for k in FRAMES}
    meta = {"torch": torch.__version__, "numpy": np.__version__, "cases": {}, "cv2": CV2_NOTE,
            "reference": "sunshinnnn/DSMnet myTransforms/aug_spatial.py, aug_color.py, __init__.py"}
    seen = {"s>1": 0, "s<1": 0, "adj>1": 0, "shift0": 0, "shift+": 0}
    print("spatial goldens (float32 CPU, reference lines executed from the file text)")
    try:
        for name, key, crop, delt, smax, seed, with_train in CASES:
            x = store["frames." + key]
            args = (list(crop), delt, smax)
            want, logs, scales, smax_after, nxt = run_reference(ref, "Stereo_Spatial", x, args, seed, rec_ref)
            records, hw, _, mlogs, mscales, msmax, mnxt = run_planner(T, "Stereo_Spatial", x, args, seed, rec_mine)
            if (logs, scales, smax_after, nxt) != (mlogs, mscales, msmax, mnxt):
                raise SystemExit("%s: the planner's draws differ from the reference's:\n%r\n%r"
                                 % (name, (logs, scales, smax_after, nxt), (mlogs, mscales, msmax, mnxt)))
            if tuple(want.shape[2:]) != tuple(hw):
                raise SystemExit("%s: output size %s, planned %s" % (name, want.shape[2:], hw))
            got = SO.restate_batch(x, records, hw)
            err = np.abs(got.astype(np.float64) - want)
            if delt == 0:
                if not np.array_equal(got, want):
                    raise SystemExit("%s: crop-only restatement is not bit-equal (max %.3e)" % (name, err.max()))
            else:
                bound = 4 * 2.0 ** -23 * SO.tap_bound_batch(x, records, hw)
                if (err > bound).any():
                    raise SystemExit("%s: restatement outside the bound (max %.3e)" % (name, err.max()))
            for r, log, s in zip(records, logs, scales):
                if delt == 0:
                    seen["shift0" if r[0] == 0 else "shift+"] += 1
                else:
                    u, coin = log[1][2], log[2][2]
                    pre = 1 + u
                    pre = 1.0 / pre if coin > 0.5 else pre
                    seen["adj>1"] += s != pre
                    seen["s>1" if s > 1 else "s<1"] += 1
            print("  %-12s out %s  max |restatement - reference| %.2e  records %s"
                  % (name, want.shape, err.max(), [tuple(r[:6]) + (round(r[6], 4),) for r in records]))
            store[name + ".out"] = want
            store[name + ".records"] = np.array(records, dtype=np.float64)
            store[name + ".next_rand"] = np.float64(nxt)
            meta["cases"][name] = {"frames": key, "size_crop": list(crop), "scale_delt": delt, "shift_max": smax,
                                   "seed": seed, "shift_max_after": smax_after, "scale_rand_after": scales[-1],
                                   "train": bool(with_train)}
            if with_train:
                twant, tlogs, _, _, tnxt = run_reference(ref, "Stereo_train", x, args, seed, rec_ref)
                _, _, color, _, _, _, _ = run_planner(T, "Stereo_train", x, args, seed, rec_mine)
                if tlogs != logs or tnxt != nxt:
                    raise SystemExit("%s: Stereo_train drew other spatial numbers than Stereo_Spatial" % name)
                out = torch.from_numpy(got).double()
                for recs, alpha, G in color:
                    out = CO.restate(out, recs, alpha, G)
                terr = (out - torch.from_numpy(twant).double()).abs().max().item()
                print("  %-12s Stereo_train max |restatement - reference| %.2e" % ("", terr))
                if terr > 1e-5:
                    raise SystemExit("%s: Stereo_train restatement disagrees with the reference" % name)
                store[name + ".train"] = twant
    finally:
        T.np = real_np
    print("  coverage: %s" % seen)
    if not all(seen.values()):
        raise SystemExit("the seeds do not reach every branch: %s" % seen)
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_spatial.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
