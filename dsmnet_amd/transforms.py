"""The reference's colour transforms (myTransforms/aug_color.py, myTransforms/__init__.py:109-135)
on a device batch, as one ``dsm_stereo_color`` launch per batch (csrc/color.hip).

    transform = transforms.Stereo_color(same_group=True)     # training (stereo_selfsupervised.py:59)
    batch_aug = transforms.Stereo_color_batch(batch_aug, transform)
    transform = transforms.Stereo_normalize()                # validation (stereo_selfsupervised.py:159)

A transform object is callable on a (B, C, H, W) fp32 device batch or on one (C, H, W) image
(B = 1) and rewrites it in place, as the reference's do; so it can be passed as ``augment=`` to
``train.train_step_selfsup`` / ``validate_step_selfsup``.  C >= 6: channels 6.. (a disparity) are
untouched.

The host draws every random number the reference draws, in its order, image by image:
ColorJitter's ``torch.randperm(4)`` (CPU generator) and three ``random.uniform`` per step in the
drawn order, then Lighting's ``normal_(0, alphastd)`` of 3 elements on the batch's device (one call
per image, or per group with ``same_group=False``).  Nothing is read back from the device.

The defaults are the stereo recipe's (group=2, same_group=True), not aug_color.py's class defaults.
One drift from the reference: Gamma raises max(x, 0), where the reference yields NaN for the
negative values Contrast or Saturation can leave before it.
"""
import random

import torch

from . import _lib
from . import costvolume as cv

_IDENTITY = (0, 1, 2, 3)


def _groups(group, C):
    g = min(group, C // 3)
    if C < 6 or g not in (1, 2):
        raise ValueError("colour transforms run on (B, C >= 6, H, W) batches with 1 or 2 RGB groups; "
                         "got C = %d, group = %d" % (C, group))
    return g


class _Step(object):
    rank = None            # position in the kernel's fixed pipeline: jitter, lighting, normalize

    def __call__(self, img):
        return Compose([self])(img)


class ColorJitter(_Step):
    """aug_color.py:175-224: Brightness x*(1+u), Contrast x+u, Saturation x+gray*u, Gamma
    max(x,0)**(1+u) in a random order, u = uniform(-0.5, 0.5) * Jitter, then clamp(0, 1)."""
    rank = 0

    def __init__(self, Jitter=0.4, group=2, same_group=True):
        self.var, self.group, self.same_group = float(Jitter), int(group), bool(same_group)

    def _draw(self):
        order = [int(i) for i in torch.randperm(4)]
        vals = [0.0] * 4
        for t in order:
            u = [random.uniform(-0.5, 0.5) * self.var for _ in range(3)][0]
            vals[t] = 1 + u if t in (0, 3) else u          # Brightness, Gamma: 1 + u
        return tuple(order), tuple(vals)

    def _plan(self, recs, alpha, i, G):
        same = self.same_group and G > 1
        draws = [self._draw()] if same else [self._draw() for _ in range(G)]
        for g in range(G):
            r = recs[i * G + g]
            r["order"], r["jitter"] = draws[0 if same else g]
            r["flags"] |= _lib.DSM_COLOR_JITTER


class Lighting(_Step):
    """aug_color.py:66-101: x += eigvec @ (alpha * eigval) with alpha ~ N(0, alphastd), drawn on the
    batch's device, then clamp(0, 1).  alphastd == 0 draws nothing and does nothing."""
    rank = 1

    def __init__(self, alphastd=0.1, group=2, same_group=True):
        self.alphastd, self.group, self.same_group = float(alphastd), int(group), bool(same_group)

    def _plan(self, recs, alpha, i, G):
        if self.alphastd == 0:
            return
        same = self.same_group and G > 1
        for g in range(G):
            row = i * G + (0 if same else g)
            if g == 0 or not same:
                alpha[row].normal_(0, self.alphastd)
            recs[i * G + g]["alpha_row"] = row
            recs[i * G + g]["flags"] |= _lib.DSM_COLOR_LIGHTING


class Normalize_Imagenet(_Step):
    """aug_color.py:28-45 with the ImageNet mean / std: (x - mean) / std per group."""
    rank = 2

    def __init__(self, group=2):
        self.group = int(group)

    def _plan(self, recs, alpha, i, G):
        for g in range(G):
            recs[i * G + g]["flags"] |= _lib.DSM_COLOR_NORMALIZE


class Compose(object):
    """A sequence of the steps above.  Consecutive steps in the kernel's order (jitter, lighting,
    normalize) with the same ``group`` share one launch."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        for t in self.transforms:
            if not isinstance(t, _Step):
                raise TypeError("Compose takes ColorJitter, Lighting and Normalize_Imagenet steps, got %r" % (t,))
        self.launches = []
        for t in self.transforms:
            last = self.launches[-1] if self.launches else None
            if last is not None and last[-1].rank < t.rank and last[-1].group == t.group:
                last.append(t)
            else:
                self.launches.append([t])

    def plan(self, B, C, device, dtype=torch.float32):
        """Draw every random number of the batch in the reference's order (image by image, step by
        step).  Returns one ``(records, alpha, groups)`` per launch; ``alpha`` is (B, groups, 3) on
        ``device`` (rows of a shared draw are left unwritten) or None."""
        plans = []
        for steps in self.launches:
            G = _groups(steps[0].group, C)
            recs = [{"order": _IDENTITY, "jitter": (1.0, 0.0, 0.0, 1.0), "flags": 0, "alpha_row": 0}
                    for _ in range(B * G)]
            lights = any(isinstance(s, Lighting) and s.alphastd != 0 for s in steps)
            alpha = torch.empty(B * G, 3, device=device, dtype=dtype) if lights else None
            plans.append((steps, G, recs, alpha))
        for i in range(B):
            for steps, G, recs, alpha in plans:
                for s in steps:
                    s._plan(recs, alpha, i, G)
        out = []
        for steps, G, recs, alpha in plans:
            tuples = [(r["order"], r["jitter"], r["flags"], r["alpha_row"]) for r in recs]
            out.append((tuples, None if alpha is None else alpha.view(B, G, 3), G))
        return out

    def __call__(self, img):
        if img.dim() not in (3, 4):
            raise ValueError("colour transforms take a (C,H,W) image or a (B,C,H,W) batch, got %s"
                             % (tuple(img.shape),))
        if not img.is_cuda:
            cv._require_device("transforms", img)
        x = img.unsqueeze(0) if img.dim() == 3 else img
        for records, alpha, G in self.plan(x.shape[0], x.shape[1], x.device, x.dtype):
            cv.stereo_color(x, records, alpha, G)
        return img


def Stereo_color(same_group=True):
    """myTransforms/__init__.py:109-114: ColorJitter + Lighting + Normalize_Imagenet, group 2."""
    return Compose([ColorJitter(Jitter=0.4, group=2, same_group=same_group),
                    Lighting(alphastd=0.1, group=2, same_group=same_group),
                    Normalize_Imagenet(group=2)])


def Stereo_normalize():
    """myTransforms/__init__.py:121-124: Normalize_Imagenet(group=2); draws nothing."""
    return Compose([Normalize_Imagenet(group=2)])


def Stereo_color_batch(sample_batch, transform):
    """myTransforms/__init__.py:130-135: ``transform`` on every image of the (B, C, H, W) batch, in
    place.  The transforms of this module take the whole batch in one launch."""
    if sample_batch.dim() != 4:
        raise ValueError("Stereo_color_batch: a (B, C, H, W) batch, got %s" % (tuple(sample_batch.shape),))
    if isinstance(transform, (Compose, _Step)):
        return transform(sample_batch)
    for i in range(sample_batch.shape[0]):
        sample_batch[i] = transform(sample_batch[i])
    return sample_batch
