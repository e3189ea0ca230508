#!/usr/bin/env python3
"""Generate tests/golden/golden_lrcheck.npz from the REFERENCE's own warp and weight.

Runs only where the reference tree exists (never on the GPU box).  ``utils/imwrap.py`` is executed from its
text as a module (:37-72 ``imwrap_BCHW``), and losses/loss.py:393-404 ``weight_common`` from the file text
as a method of a holder class (``ref_lines`` of make_goldens.py), with the shims make_goldens_selfsup.py
documents: ``.data[0]`` -> ``.item()``, ``(disp_delt<3) - mask1`` -> ``(disp_delt<3) & ~mask1``, and
``Variable(...)`` without its ``requires_grad`` keyword.  Everything the reference computes here is float32 on
the CPU, what it would compute in training; torch's CPU generator is seeded before the warp, so its own
``torch.rand(1)`` epsilon is reproducible and is stored as ``delt``.

Cases (B,H,W): smooth disparities of 0 .. dmax px (dmax starts at 40) with an occluding box in ``disp``; the
other view's map is roughly consistent with it outside the box.  Disparities are multiples of 2^-10 (the
fixture compresses, and nothing is lost: every kernel reads them as they are).

E_ref, per case: the largest |reference float32 - float64 restatement| of ``wrap`` and of ``weight``
(tests/lrcheck_oracle.py).  The margin: every pixel's delta is kept 1e-3 away from the threshold, from 1 and
from 3, and its sample position 1e-3 away from 0 and W - 1 -- offending disparities are MOVED (by multiples of
2^-6), never masked out.  A case is written only if 1e-3 >= 8 * E_ref; the disparity range is halved until the
reference satisfies that.

Usage:  python tests/golden/make_goldens_lrcheck.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL       # noqa: E402
from tests import lrcheck_oracle as LO          # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402

warnings.filterwarnings("ignore")

MARGIN = 1e-3
THRESHOLD = 1.0
Q = 1024.0                                       # disparities are multiples of 1 / Q
CASES = (("c2x2", 1, 2, 2, 1.0, 501), ("c5x63", 2, 5, 63, 1.0, 502), ("c3x65", 1, 3, 65, 1.0, 503),
         ("c4x257", 2, 4, 257, 1.0, 504), ("c6x1030", 1, 6, 1030, 1.0, 505), ("c8x64f4", 1, 8, 64, 4.0, 506))


def load_reference():
    imwrap_mod = RL._exec_text("ref_imwrap", os.path.join(RL.REFERENCE_ROOT, "utils", "imwrap.py"))
    body = []
    for l in ref_lines("losses/loss.py", 393, 404).splitlines():
        l = l.replace(".data[0]", ".item()")
        l = l.replace("(disp_delt<3) - mask1", "(disp_delt<3) & ~mask1")
        l = l.replace("Variable(torch.zeros(disp_delt.shape), requires_grad=False)", "(torch.zeros(disp_delt.shape))")
        body.append("    " + l)
    ns = {"torch": torch, "logging": __import__("logging")}
    exec("class Ref(object):\n" + "\n".join(body) + "\n", ns)
    return imwrap_mod.imwrap_BCHW, ns["Ref"]().weight_common


def quant(t):
    return torch.round(t * Q) / Q


def smooth(g, B, H, W, lo, hi, cell):
    coarse = torch.rand(B, 1, max(2, H // cell + 2), max(2, W // cell + 2), generator=g)
    return lo + (hi - lo) * F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)


def make_maps(seed, B, H, W, dmax):
    """disp (left frame) and other (mirrored frame), float32 (B,1,H,W)."""
    g = torch.Generator().manual_seed(seed)
    # gentle slopes: the reference's float32 sample position is off by about W * 2^-23, and the error of
    # `wrap` is that times the slope of `other`
    base = smooth(g, B, H, W, 0.0, dmax, max(16, W // 4))
    # the right camera's map, roughly: the left one shifted by itself, then mirrored; a gentle disagreement
    # of up to 1.5 thresholds on top, so that delta lands on both sides of 1 outside the box too
    xs = torch.arange(W).view(1, 1, 1, W).float()
    src = (xs + base).clamp(0, W - 1).round().long().expand(B, 1, H, W)
    other = torch.flip(torch.gather(base, 3, src), dims=[-1])
    other = (other + smooth(g, B, H, W, -1.5, 1.5, max(8, W // 8)) * min(1.0, dmax / 8.0)).clamp(min=0)
    if W > 128:
        # where the sample leaves the image the zero padding makes `wrap` as steep as `other` is large
        # there: wide maps let `other` fall to zero over W / 8 columns at both ends
        ramp = (torch.arange(W).float() / (W // 8)).clamp(max=1)
        other = other * (ramp * ramp.flip(0)).view(1, 1, 1, W)
    disp = base.clone()
    if W > 4:                                    # the occluding box: nearer than the background by 3/8 dmax
        x0, x1 = W // 3, W // 3 + max(2, W // 6)
        disp[:, :, H // 4: max(H // 4 + 1, 3 * H // 4), x0:x1] += 0.375 * dmax
    return quant(disp), quant(other)


def offenders(disp, other, delt, factor):
    r = LO.lr_check(disp, other, delt, factor, THRESHOLD)
    W = disp.shape[-1]
    bad = torch.zeros_like(r.mask)
    for edge in (THRESHOLD, 1.0, 3.0):
        bad |= (r.delta - edge).abs() < MARGIN
    bad |= (r.ix.abs() < MARGIN) | ((r.ix - (W - 1)).abs() < MARGIN)
    return bad


def gen_case(ref_warp, ref_weight, store, meta, name, B, H, W, factor, seed):
    dmax = 40.0
    while True:
        disp, other = make_maps(seed, B, H, W, dmax)
        torch.manual_seed(seed)
        delt = LO.SO.draw_delt()
        for _ in range(64):                      # move, never mask: a pixel's delta depends on its own disparity only
            bad = offenders(disp, other, delt, factor)
            if not bad.any():
                break
            disp = torch.where(bad, disp + 1.0 / 64, disp)
        else:
            raise SystemExit("%s: the margin cannot be reached" % name)
        torch.manual_seed(seed)
        wrap = ref_warp(other, disp, fliplr=True, LeftTop=[0, 0], scale_factor=1)
        weight = ref_weight(disp, wrap, factor=factor)
        assert wrap.dtype == torch.float32 and weight.dtype == torch.float32
        mine = LO.lr_check(disp, other, delt, factor, THRESHOLD)
        e_wrap = float((wrap.double() - mine.wrap).abs().max())
        e_weight = float((weight.double() - mine.weight).abs().max())
        ok = MARGIN >= 8 * max(e_wrap, e_weight)
        print("  %-9s dmax %-6g delt %.3e  E_ref wrap %.3e weight %.3e  mask true %.1f %%  %s"
              % (name, dmax, delt, e_wrap, e_weight, 100.0 * float(mine.mask.double().mean()), "ok" if ok else "halve"))
        if ok:
            break
        dmax /= 2
        if dmax < 1:
            raise SystemExit("%s: the reference's own error stays above the margin" % name)
    delta32 = (disp - wrap).abs() / factor                       # loss.py:394, the reference's float32 delta
    if not torch.equal((delta32 < THRESHOLD) & (mine.ix >= 0) & (mine.ix <= W - 1), mine.mask):
        raise SystemExit("%s: the reference's delta and the restatement's disagree on the mask" % name)
    if H * W > 4 and not 0.05 < float(mine.mask.double().mean()) < 0.95:
        raise SystemExit("%s: the mask does not separate anything" % name)
    store[name + ".disp"], store[name + ".other"] = disp.numpy(), other.numpy()
    store[name + ".wrap"], store[name + ".weight"] = wrap.numpy(), weight.numpy()
    store[name + ".delt"] = np.float64(delt)
    store[name + ".e_ref"] = np.array([e_wrap, e_weight], dtype=np.float64)
    meta["cases"][name] = {"B": B, "H": H, "W": W, "factor": factor, "threshold": THRESHOLD, "seed": seed, "dmax": dmax}


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    ref_warp, ref_weight = load_reference()
    store, meta = {}, {"torch": torch.__version__, "align_corners": False, "margin": MARGIN, "cases": {},
                       "reference": "sunshinnnn/DSMnet utils/imwrap.py:37-72, losses/loss.py:393-404"}
    print("lrcheck goldens (float32 reference lines executed from the file text)")
    for case in CASES:
        gen_case(ref_warp, ref_weight, store, meta, *case)
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_lrcheck.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
