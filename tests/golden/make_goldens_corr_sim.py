#!/usr/bin/env python3
"""Generate tests/golden/golden_corr_sim.npz: the reference's own ``Corr1d`` with
``simfun=nn.CosineSimilarity(dim=1)`` in float64, beside the restatement of tests/corr1d_sim_oracle.py.

Needs the reference tree (oracle/reference_loader.py reads models/util_conv.py as text from where it lies and
executes it with this torch; nothing of it is stored).  Cases (k, s, D) on (2,16,3,24) float32-representable
seeded inputs, one of them with D > W, plus one degenerate case (tests/corr1d_sim_oracle.make_degenerate: two
zero feature vectors and one shorter than eps).  Stored, all float64: inputs, outputs and the input gradients
for a seeded cotangent.

The script REFUSES to write when the restatement differs from the reference by more than 1e-12 (forward and
both gradients; absolute, |out| <= 1 and the gradients are O(1)).  In the degenerate case only the forward is
compared: inside the clamp region the installed torch's autograd of ``F.cosine_similarity`` differentiates
through the clamped norm's neighbourhood differently (about 1 % there), and the contract is the restatement
(a clamped norm is a constant), so the stored gradients of that case are the restatement's.

Usage:  python tests/golden/make_goldens_corr_sim.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import reference_loader as RL          # noqa: E402
from tests import corr1d_sim_oracle as CS           # noqa: E402
from tests.helpers import seeded                    # noqa: E402

warnings.filterwarnings("ignore")
SHAPE = (2, 16, 3, 24)
CASES = [  # tag, k, s, D, degenerate
    ("k1_s1_D9", 1, 1, 9, False),
    ("k3_s2_D5", 3, 2, 5, False),
    ("k1_s1_D30", 1, 1, 30, False),       # D > W
    ("degenerate_k1_s1_D9", 1, 1, 9, True),
]
SEED_L, SEED_R, SEED_COT = 41, 42, 43
TOL = 1e-12
OUT = os.path.join(HERE, "golden_corr_sim.npz")
LIMIT = 256 * 1024


def main():
    Corr1d = RL.load()["util_conv"].Corr1d
    store, meta = {}, {"torch": torch.__version__, "shape": list(SHAPE), "eps": 1e-8, "cases": [],
                       "seeds": {"fL": SEED_L, "fR": SEED_R, "cot": SEED_COT}}
    for tag, k, s, D, degenerate in CASES:
        fL, fR = seeded(SEED_L, *SHAPE).double(), seeded(SEED_R, *SHAPE).double()
        if degenerate:
            CS.make_degenerate(fL, fR)
        cot = seeded(SEED_COT, SHAPE[0], D, SHAPE[2], SHAPE[3]).double()
        out, gL, gR = CS.with_grads(fL, fR, cot, D, s, k, 1e-8)
        l, r = fL.clone().requires_grad_(True), fR.clone().requires_grad_(True)
        ref = Corr1d(k, s, D, simfun=nn.CosineSimilarity(dim=1))(l, r)
        rL, rR = torch.autograd.grad(ref, (l, r), cot)
        assert ref.dtype == torch.float64 and torch.isfinite(ref).all() and torch.isfinite(rL).all()
        errs = [(ref.detach() - out).abs().max().item(), (rL - gL).abs().max().item(), (rR - gR).abs().max().item()]
        print("%-22s max|ref - restatement|: out %.3e dL %.3e dR %.3e   (max |dL| %.3e)"
              % (tag, errs[0], errs[1], errs[2], gL.abs().max().item()))
        checked = errs[:1] if degenerate else errs
        if max(checked) > TOL:
            raise SystemExit("the restatement disagrees with the reference on %s: nothing written" % tag)
        if degenerate:
            assert torch.isfinite(gL).all() and torch.isfinite(gR).all()
        inputs = "degenerate_inputs" if degenerate else "inputs"     # the regular cases share one pair
        store[inputs + ".fL"], store[inputs + ".fR"] = fL.numpy(), fR.numpy()
        store[tag + ".out"] = ref.detach().numpy()
        store[tag + ".dL"], store[tag + ".dR"] = (gL if degenerate else rL).numpy(), (gR if degenerate else rR).numpy()
        meta["cases"].append({"tag": tag, "k": k, "s": s, "D": D, "degenerate": degenerate, "inputs": inputs,
                              "grads_from": "restatement" if degenerate else "reference"})
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print("%s: %d bytes" % (OUT, size))
    if size > LIMIT:
        os.remove(OUT)
        raise SystemExit("fixture larger than %d bytes: removed" % LIMIT)


if __name__ == "__main__":
    main()
