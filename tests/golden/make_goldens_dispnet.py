#!/usr/bin/env python3
"""Generate tests/golden/golden_dispnet.npz from the REFERENCE's models/dispnet.py.

Runs only where the reference tree exists (oracle/reference_loader.py).  This project's dispnet(192) is built
on the CPU under a recorded torch seed, its state dict is loaded into the reference's model with strict=True
(which certifies the 52 keys and their shapes), both run the same synthetic pairs in mode "train" and "test",
and the fixture is REFUSED unless they agree to 1e-5 of each output's maximum (the bound make_goldens.py uses
for DispNetC).  Stored: the reference's seven outputs per case, the seeds, and per parameter tensor its shape,
float64 sum and absolute sum -- nothing of the reference's text.

Usage:  python tests/golden/make_goldens_dispnet.py
"""
import importlib
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import reference_loader as RL   # noqa: E402
from tests import dispnet_cases as DC       # noqa: E402

warnings.filterwarnings("ignore")
TOL = 1e-5


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    RL.load()
    ref = importlib.import_module("dispnet").dispnet(DC.MAXDISP)
    mine = DC.build_model(DC.MODEL_SEED)
    sd = mine.state_dict()
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    store = {}
    for tag, seed, h, w in DC.CASES:
        imL, imR = DC.images(seed, h, w)
        for mode in DC.MODES:
            with torch.no_grad():
                rs, ro = ref(imL, imR, mode=mode)
                ms, mo = mine(imL, imR, mode=mode)
            assert list(rs) == list(ms) == list(range(7)), (rs, ms)
            for i, (r, m) in enumerate(zip(ro, mo)):
                assert r.shape == m.shape, (tag, mode, i, r.shape, m.shape)
                err, scale = (r - m).abs().max().item(), max(r.abs().max().item(), 1e-30)
                print("  %s %-5s out%d %-18s max|ref-ours| = %.3e (max %.3g)" % (tag, mode, i, tuple(r.shape), err, scale))
                if err > TOL * max(scale, 1.0):
                    raise SystemExit("this project's dispnet disagrees with the reference on %s %s out%d" % (tag, mode, i))
                store["out.%s.%s.%d" % (tag, mode, i)] = r.numpy().astype(np.float32)
    meta = {"torch": torch.__version__, "model_seed": DC.MODEL_SEED, "maxdisparity": DC.MAXDISP,
            "cases": [list(c) for c in DC.CASES], "modes": list(DC.MODES),
            "params": {k: {"shape": list(v.shape), "sum": v.double().sum().item(),
                           "abssum": v.double().abs().sum().item()} for k, v in sd.items()}}
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(DC.FIXTURE, **store)
    print("wrote %s (%.1f KiB, %d arrays, %d parameter tensors)"
          % (DC.FIXTURE, os.path.getsize(DC.FIXTURE) / 1024.0, len(store), len(sd)))


if __name__ == "__main__":
    main()
