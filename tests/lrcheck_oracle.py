"""TEST INFRASTRUCTURE ONLY: float64 restatement of the left-right check and the plain-loop hole fill,
the yardsticks of csrc/lrcheck.hip (``costvolume.lr_check`` / ``costvolume.fill_background``).

  lr_check         utils/imwrap.py:37-72 with fliplr=True, LeftTop [0,0], scale 1 (as loss.py:451-452 call
                   it) and loss.py:393-404 weight_common: ``selfsup_oracle.imwrap_bchw`` and
                   ``selfsup_oracle.weight_common``, imported.  The mask adds the inside test on the
                   sample position, which the reference does not make.
  fill_background  the semantics of include/dsmnet_hip.h as loops over numpy arrays.

Pinned against the reference's own lines by tests/golden/make_goldens_lrcheck.py (fixture
tests/golden/golden_lrcheck.npz).
"""
import collections

import numpy as np
import torch

from tests import selfsup_oracle as SO

Result = collections.namedtuple("Result", ("wrap", "weight", "mask", "masked", "delta", "ix"))


def as_bchw(t):
    return t.unsqueeze(1) if t.dim() == 3 else t


def sample_ix(disp, dtype=torch.float64):
    """Un-normalised x position of the flip grid's sample, (B,1,H,W): the base grid is torch.linspace in
    fp32 (as the reference builds it), everything after it in ``dtype``."""
    d = as_bchw(disp).to(dtype)
    W = d.shape[-1]
    gx = -(torch.linspace(-1, 1, W).to(dtype).view(1, 1, 1, W) - d * 2.0 / (W - 1))
    return ((gx + 1) * W - 1) / 2


def lr_check(disp, other, delt=0.0, factor=1.0, threshold=1.0, mirrored=True, dtype=torch.float64):
    """(wrap, weight, mask, masked, delta, ix) of (B,1,H,W) or (B,H,W) maps, in ``dtype``; ``masked`` is
    ``disp`` in its own dtype times the mask."""
    d, o = as_bchw(disp).to(dtype), as_bchw(other).to(dtype)
    if not mirrored:
        o = o.flip(-1)
    W = d.shape[-1]
    wrap = SO.imwrap_bchw(o, d, delt, fliplr=True)
    delta = (d - wrap).abs() / factor
    weight = SO.weight_common(d, wrap, factor)
    ix = sample_ix(d, dtype)
    mask = (delta < threshold) & (ix >= 0) & (ix <= W - 1)
    masked = torch.where(mask, as_bchw(disp), torch.zeros_like(as_bchw(disp)))
    shape = disp.shape
    return Result(*[t.reshape(shape) for t in (wrap, weight, mask, masked, delta, ix)])


def known_scene():
    """A background plane at d = 4 and a foreground box at d = 12 (rows 2..5, left-image columns 40..59) at
    8x96, both cameras' maps built analytically: ``(dispL, dispR)``, (1,1,8,96) float32, each in its own
    frame.  In the right image the box lies 12 columns further left (28..47)."""
    dL, dR = torch.full((1, 1, 8, 96), 4.0), torch.full((1, 1, 8, 96), 4.0)
    dL[:, :, 2:6, 40:60] = 12.0
    dR[:, :, 2:6, 28:48] = 12.0
    return dL, dR


def check_known_scene(maskL, maskR):
    """What the geometry says about the masks of ``known_scene`` (both in their own camera's frame).

    The sampler reads the other view at (x - d) * W / (W - 1) - 0.5 (align_corners=False on a linspace(-1, 1)
    grid), within half a pixel of x - d, and row y at y * 8 / 7 - 0.5: rows 3 and 4 read box rows only, rows
    1 and 6 background rows only, rows 2 and 5 mix the two and rows 0 and 7 the zero padding -- those four
    are not judged.  Left view: the background columns 32..39 see the right image's box where they should
    see background -- they are hidden behind the box from the right camera.  Right view: columns 48..55,
    by the mirrored argument.  One pixel at either end of a band may go either way (the half-pixel above);
    everything else inside is consistent.  Columns whose sample leaves the image are not interior:
    x < 6 on the left, x > 89 on the right."""
    mL, mR = maskL.reshape(8, 96).cpu(), maskR.reshape(8, 96).cpu()
    for m, band, interior in ((mL, (32, 40), (6, 96)), (mR, (48, 56), (0, 90))):
        for y in (3, 4):
            assert not m[y, band[0] + 1:band[1] - 1].any(), (y, band)
            assert m[y, interior[0]:band[0] - 1].all() and m[y, band[1] + 1:interior[1]].all(), (y, band)
        for y in (1, 6):
            assert m[y, interior[0]:interior[1]].all(), y


def fill_background(disp, mask):
    """numpy (B,H,W) float32 and bool -> filled float32.  Invalid values are never read."""
    disp, mask = np.asarray(disp), np.asarray(mask).astype(bool)
    B, H, W = disp.shape
    out = np.zeros((B, H, W), dtype=np.float32)
    for b in range(B):
        nonempty = [bool(mask[b, y].any()) for y in range(H)]
        # 1. rows
        for y in range(H):
            if not nonempty[y]:
                continue
            for x in range(W):
                if mask[b, y, x]:
                    out[b, y, x] = disp[b, y, x]
                    continue
                l = x - 1
                while l >= 0 and not mask[b, y, l]:
                    l -= 1
                r = x + 1
                while r < W and not mask[b, y, r]:
                    r += 1
                if l >= 0 and r < W:
                    out[b, y, x] = np.fmin(disp[b, y, l], disp[b, y, r])
                elif l >= 0:
                    out[b, y, x] = disp[b, y, l]
                else:
                    out[b, y, x] = disp[b, y, r]
        # 2. empty rows, from the rows as filled above
        for y in range(H):
            if nonempty[y]:
                continue
            u = y - 1
            while u >= 0 and not nonempty[u]:
                u -= 1
            v = y + 1
            while v < H and not nonempty[v]:
                v += 1
            if u >= 0 and v < H:
                out[b, y] = np.fmin(out[b, u], out[b, v])
            elif u >= 0:
                out[b, y] = out[b, u]
            elif v < H:
                out[b, y] = out[b, v]
    return out
