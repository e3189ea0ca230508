"""The reference's colour transforms (myTransforms/aug_color.py, myTransforms/__init__.py:109-135)
on a device batch, as one ``dsm_stereo_color`` launch per batch (csrc/color.hip),
and its spatial transform with ToTensor as one ``dsm_stereo_spatial`` launch (further down).

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

The spatial half (myTransforms/aug_spatial.py:7-88, aug_color.py:15-26, __init__.py:88-119), one
``dsm_stereo_spatial`` launch per batch (csrc/spatial.hip):

    transform = transforms.Stereo_train(size_crop=[768, 384], scale_delt=0, shift_max=32)
    batch = transform(frames)            # (B, H0, W0, C) channels-last frames, values 0..255
    loss, d1, epe = train.train_step(model, optim, lossfun, batch)

``Stereo_train``, ``Stereo_Spatial``, ``Stereo_ToTensor`` and ``Stereo_eval`` are callable on a
(B, H0, W0, C) fp32 device batch of raw frames (imL | imR [| dispL [| dispR]], 6 <= C <= 8) or on
one (H0, W0, C) frame, and return a NEW (B, C, h, w) / (C, h, w) tensor; the frames are not
modified (the reference shifts its input in place).  The host draws the reference's ``np.random``
numbers in its order, image by image: ``randint`` for the shift, then ``randint, randint`` for the
crop or ``uniform, rand, randint, randint`` for crop and scale, skipping the draws the reference
skips.  With ``scale_delt == 0`` the reference's output width is min(W0 - shift, w1), which can
differ per image; ``ValueError`` when W0 - (shift_max - 1) < w1, as the batch could otherwise not
be rectangular.  The resize is cv2's linear rule as stated in DESIGN.md §13b; that it equals the
cv2 binary is not measured.

``Compose.call_raw`` is the same pipeline started from the decoded files' bytes instead of fp32
frames (``costvolume.stereo_spatial_raw``, csrc/frames.hip); ``datasets.DeviceLoader``
is its caller.
"""
import random

import numpy as np
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


class Spatial_stereo(_Step):
    """aug_spatial.py:7-88: random shift of the right view (and of a right disparity, channel 7;
    every disparity channel += shift where != 0), random crop to ``size_crop`` = [w, h], and with
    ``scale_delt != 0`` a random scale of the window (cv2's linear resize; disparities * scale).
    ``draw`` is the reference's ``__call__`` up to the pixels: it consumes ``np.random`` as the
    reference does, clamps ``shift_max`` to the frame width for good, and keeps the last image's
    ``scale_rand``, ``ws`` and ``hs`` on the object."""
    rank = -2

    def __init__(self, size_crop=[768, 384], scale_delt=0.5, shift_max=32):
        self.size_crop = size_crop
        self.ws = 0
        self.hs = 0
        self.scale_rand = 1
        self.scale_delt = scale_delt
        self.shift_max = shift_max

    def out_hw(self, h0, w0):
        """(h, w) of the output for (h0, w0) frames.  With ``scale_delt == 0`` the reference's
        width is min(w0 - shift, w1), which differs from image to image when the largest shift
        leaves fewer than w1 columns: ValueError, the batch could not be rectangular."""
        w1, h1 = self.size_crop
        if self.scale_delt != 0:
            return h1, w1
        if self.shift_max > 0 and w0 - (min(self.shift_max, w0) - 1) < w1:
            raise ValueError("Spatial_stereo: a crop of width %d does not fit %d columns less a shift of up to "
                             "%d: the images of a batch would differ in width" % (w1, w0, min(self.shift_max, w0) - 1))
        return min(h0, h1), min(w0, w1)

    def draw(self, h0, w0):
        """One image's record ``(shift, ws, hs, w, h, resize, scale_rand, scale_x, scale_y)``."""
        w1, h1 = self.size_crop
        shift_rand = 0
        if self.shift_max > 0:
            self.shift_max = min(self.shift_max, w0)
            shift_rand = int(np.random.randint(0, self.shift_max))
            w0 -= abs(shift_rand)
        if self.scale_delt == 0:
            w1 = min(w0, w1)
            h1 = min(h0, h1)
            w, h = w1, h1
            ws = np.random.randint(0, w0 - w) if w0 > w else 0
            hs = np.random.randint(0, h0 - h) if h0 > h else 0
            resize = False
        else:
            self.scale_rand = 1 + np.random.uniform(0, self.scale_delt)
            if np.random.rand() > 0.5:
                self.scale_rand = 1.0 / self.scale_rand
            w = int(w1 / self.scale_rand + 0.5)
            h = int(h1 / self.scale_rand + 0.5)
            scale_adjust = max(float(h) / min(h, h0), float(w) / min(w, w0))
            self.scale_rand *= scale_adjust
            w = int(w / scale_adjust + 0.5)
            h = int(h / scale_adjust + 0.5)
            ws = np.random.randint(0, w0 - w) if w0 > w else 0
            hs = np.random.randint(0, h0 - h) if h0 > h else 0
            resize = self.scale_rand != 1
            if not resize and (w, h) != (w1, h1):
                raise ValueError("Spatial_stereo: scale 1 with a %dx%d window for a %dx%d crop" % (w, h, w1, h1))
        self.ws, self.hs = int(ws), int(hs)
        scale_x = 1.0 / (float(w1) / w) if resize else 1.0
        scale_y = 1.0 / (float(h1) / h) if resize else 1.0
        return (shift_rand, int(ws), int(hs), w, h, int(resize), float(self.scale_rand), scale_x, scale_y)


class ToTensor_numpy(_Step):
    """aug_color.py:15-26: HWC -> CHW and the first ``channel`` planes / 255.  The kernel divides
    the two RGB groups or nothing: ``channel`` is 6."""
    rank = -1

    def __init__(self, channel=6):
        if channel != 6:
            raise ValueError("ToTensor_numpy: channel must be 6 (imL | imR), got %r" % (channel,))
        self.channel = channel


class Compose(object):
    """A sequence of the steps above.  Consecutive colour steps in the kernel's order (jitter,
    lighting, normalize) with the same ``group`` share one launch.  ``Spatial_stereo`` and / or
    ``ToTensor_numpy`` may lead the sequence: they are one ``dsm_stereo_spatial`` launch on
    (B, H0, W0, C) channels-last frames that returns the new (B, C, h, w) batch, which the colour
    launches then rewrite."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        for t in self.transforms:
            if not isinstance(t, _Step):
                raise TypeError("Compose takes ColorJitter, Lighting and Normalize_Imagenet steps, got %r" % (t,))
        self.spatial = self.to_tensor = None
        color = list(self.transforms)
        if color and isinstance(color[0], Spatial_stereo):
            self.spatial = color.pop(0)
        if color and isinstance(color[0], ToTensor_numpy):
            self.to_tensor = color.pop(0)
        for t in color:
            if t.rank < 0:
                raise TypeError("Compose: Spatial_stereo, then ToTensor_numpy, come first and once; got %r after them" % (t,))
        self.launches = []
        for t in color:
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

    def plan_spatial(self, B, H0, W0):
        """Draw the spatial numbers of B frames of H0 x W0 in the reference's order, image by
        image (``np.random``).  Returns ``(records, (h, w), to_tensor_channels)`` for
        ``costvolume.stereo_spatial``; needs no GPU."""
        if self.spatial is None:
            records, hw = [(0, 0, 0, W0, H0, 0, 1.0, 1.0, 1.0)] * B, (H0, W0)
        else:
            hw = self.spatial.out_hw(H0, W0)
            records = [self.spatial.draw(H0, W0) for _ in range(B)]
        return records, hw, self.to_tensor.channel if self.to_tensor is not None else 0

    def call_raw(self, raw, sources, frame_hw, C, draw_flip=None):
        """The hook of ``datasets.DeviceLoader``: plan for ``len(sources)`` frames of ``frame_hw`` =
        (H0, W0), then launch from the decoded files' bytes instead of from fp32 frames
        (``costvolume.stereo_spatial_raw``; ``raw`` and ``sources`` as there), then the colour
        launches on the result.  ``draw_flip()`` -> 0 / 1, if given, is called once per image
        right before that image's spatial numbers are drawn and overrides the source's ``flip``:
        the order of the reference's loop (Dataset_stereo.py:122, then the transform).  Returns
        the new (B, C, h, w) batch, bit-identical to ``__call__`` on the assembled frames."""
        if self.spatial is None and self.to_tensor is None:
            raise TypeError("Compose.call_raw: the sequence must be led by Spatial_stereo and / or ToTensor_numpy")
        H0, W0 = int(frame_hw[0]), int(frame_hw[1])
        hw = self.spatial.out_hw(H0, W0) if self.spatial is not None else (H0, W0)
        records, sources = [], [tuple(s) for s in sources]
        for i, s in enumerate(sources):
            if draw_flip is not None:
                sources[i] = s[:8] + (int(draw_flip()),) + s[9:]
            records.append(self.spatial.draw(H0, W0) if self.spatial is not None
                           else (0, 0, 0, W0, H0, 0, 1.0, 1.0, 1.0))
        out = cv.stereo_spatial_raw(raw, sources, records, (H0, W0), C, hw,
                                    self.to_tensor.channel if self.to_tensor is not None else 0)
        for records, alpha, G in self.plan(out.shape[0], out.shape[1], out.device, out.dtype):
            cv.stereo_color(out, records, alpha, G)
        return out

    def _call_spatial(self, img):
        if img.dim() not in (3, 4):
            raise ValueError("spatial transforms take a (H0,W0,C) frame or a (B,H0,W0,C) batch, got %s"
                             % (tuple(img.shape),))
        if not img.is_cuda:
            cv._require_device("transforms", img)
        x = img.unsqueeze(0) if img.dim() == 3 else img
        if x.dtype != torch.float32 or not 6 <= x.shape[3] <= 8 or not x.is_contiguous():
            raise ValueError("spatial transforms take dense float32 channels-last frames with 6 <= C <= 8, got %s %s"
                             % (x.dtype, tuple(img.shape)))
        records, hw, channels = self.plan_spatial(x.shape[0], x.shape[1], x.shape[2])
        out = cv.stereo_spatial(x, records, hw, channels)
        for records, alpha, G in self.plan(out.shape[0], out.shape[1], out.device, out.dtype):
            cv.stereo_color(out, records, alpha, G)
        return out[0] if img.dim() == 3 else out

    def __call__(self, img):
        if self.spatial is not None or self.to_tensor is not None:
            return self._call_spatial(img)
        if img.dim() not in (3, 4):
            raise ValueError("colour transforms take a (C,H,W) image or a (B,C,H,W) batch, got %s"
                             % (tuple(img.shape),))
        if not img.is_cuda:
            cv._require_device("transforms", img)
        x = img.unsqueeze(0) if img.dim() == 3 else img
        for records, alpha, G in self.plan(x.shape[0], x.shape[1], x.device, x.dtype):
            cv.stereo_color(x, records, alpha, G)
        return img


def Stereo_train(size_crop=[768, 384], scale_delt=0.4, shift_max=32):
    """myTransforms/__init__.py:88-95: Spatial_stereo + ToTensor_numpy(6) (one launch), then
    Lighting + Normalize_Imagenet, group 2 (one launch).  ColorJitter is commented out there."""
    return Compose([Spatial_stereo(size_crop, scale_delt, shift_max), ToTensor_numpy(channel=6),
                    Lighting(alphastd=0.1, group=2, same_group=True), Normalize_Imagenet(group=2)])


def Stereo_eval():
    """myTransforms/__init__.py:97-101: ToTensor_numpy(6) + Normalize_Imagenet(group=2)."""
    return Compose([ToTensor_numpy(channel=6), Normalize_Imagenet(group=2)])


def Stereo_Spatial(size_crop=[768, 384], scale_delt=0.4, shift_max=32):
    """myTransforms/__init__.py:103-107: Spatial_stereo + ToTensor_numpy(6), one launch."""
    return Compose([Spatial_stereo(size_crop, scale_delt, shift_max), ToTensor_numpy(channel=6)])


def Stereo_ToTensor():
    """myTransforms/__init__.py:116-119: ToTensor_numpy(6) alone: transpose and / 255."""
    return Compose([ToTensor_numpy(channel=6)])


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
