"""Restatements of the reference's colour transforms (myTransforms/aug_color.py:28-45, 66-101,
103-203; myTransforms/__init__.py:109-135), written from the reference's documented behaviour.

``restate``: float64, given explicit per-(image, group) records and Lighting draws -- the contract
of ``costvolume.stereo_color`` / ``dsm_stereo_color``.  ``reference_nan=True`` reproduces the
reference's NaN for a negative base of Gamma; the default is the product's drift, max(x, 0).

``stereo_color_batch_torch``: the reference's per-image loop with stock torch ops on the batch's
device and in its dtype, drawing its own ``torch.randperm``, ``random.uniform`` and device
``normal_`` numbers in the reference's order (Gamma drift applied).  Seeded like the product's
planner, it must consume the generators identically.
"""
import random

import numpy as np
import torch

JITTER, LIGHTING, NORMALIZE = 1, 2, 4

# the reference's constants are float32 tensors / float32-cast scalars
_F32 = lambda v: [float(np.float32(x)) for x in v]
EIGVAL = _F32([0.2175, 0.0188, 0.0045])
EIGVEC = [_F32(r) for r in ([-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203])]
MEAN = _F32([0.485, 0.456, 0.406])
STD = _F32([0.229, 0.224, 0.225])
GRAY = _F32([0.299, 0.587, 0.114])


def _gray(v):
    return GRAY[0] * v[0] + GRAY[1] * v[1] + GRAY[2] * v[2]


def restate(x, records, alpha, groups, reference_nan=False):
    """float64 copy of ``x`` (B,C,H,W) after the records' steps; channels 3*groups.. untouched."""
    out = x.detach().to(torch.float64).clone()
    a = None if alpha is None else alpha.detach().to(torch.float64).reshape(-1, 3)
    ev = torch.tensor(EIGVEC, dtype=torch.float64, device=out.device)
    el = torch.tensor(EIGVAL, dtype=torch.float64, device=out.device)
    for b in range(out.shape[0]):
        for g in range(groups):
            order, jit, flags, row = records[b * groups + g]
            j = _F32(jit)
            v = out[b, 3 * g:3 * g + 3].clone()
            if flags & JITTER:
                for t in order:
                    if t == 0:
                        v = v * j[0]
                    elif t == 1:
                        v = v + j[1]
                    elif t == 2:
                        v = v + _gray(v).unsqueeze(0) * j[2]
                    else:
                        v = (v if reference_nan else v.clamp_min(0)) ** j[3]
                v = v.clamp(0, 1)
            if flags & LIGHTING:
                rgb = (ev * a[row].to(out.device).view(1, 3) * el.view(1, 3)).sum(1)
                v = (v + rgb.view(3, 1, 1)).clamp(0, 1)
            if flags & NORMALIZE:
                for c in range(3):
                    v[c] = (v[c] - MEAN[c]) / STD[c]
            out[b, 3 * g:3 * g + 3] = v
    return out


def stereo_color_batch_torch(batch, same_group=True, color=True, jitter=0.4, alphastd=0.1):
    """In place on ``batch`` (B,C,H,W): Stereo_color(same_group) (``color``) or Stereo_normalize,
    image by image as Stereo_color_batch does."""
    B, C, H, W = batch.shape
    G = min(2, C // 3)
    ev = torch.tensor(EIGVEC, dtype=batch.dtype, device=batch.device)
    el = torch.tensor(EIGVAL, dtype=batch.dtype, device=batch.device)
    for i in range(B):
        img = batch[i]
        if color:
            # ColorJitter: one random order for both groups, or one per group
            spans = [(0, 3 * G)] if (same_group and G > 1) else [(3 * g, 3 * g + 3) for g in range(G)]
            for lo, hi in spans:
                for t in torch.randperm(4).tolist():
                    u = [random.uniform(-0.5, 0.5) * jitter for _ in range(3)][0]
                    seg = img[lo:hi].view(-1, 3, H, W)
                    if t == 0:
                        seg.mul_(1 + u)
                    elif t == 1:
                        seg.add_(u)
                    elif t == 2:
                        gray = seg[:, 0] * GRAY[0] + seg[:, 1] * GRAY[1] + seg[:, 2] * GRAY[2]
                        seg.add_(gray.unsqueeze(1) * u)
                    else:
                        seg.copy_(seg.clamp_min(0) ** (1 + u))
            img[:3 * G].clamp_(0, 1)
            # Lighting: a 3-element normal_ on the image's device, once per image or per group
            if alphastd != 0:
                alpha = None
                for g in range(G):
                    if alpha is None or not (same_group and G > 1):
                        alpha = img.new_empty(3).normal_(0, alphastd)
                    rgb = (ev * alpha.view(1, 3) * el.view(1, 3)).sum(1)
                    img[3 * g:3 * g + 3] = (img[3 * g:3 * g + 3] + rgb.view(3, 1, 1)).clamp(0, 1)
        for g in range(G):
            for c in range(3):
                img[3 * g + c].sub_(MEAN[c]).div_(STD[c])
    return batch
