"""A stereo dataset of image pairs and their disparity maps (myDatasets_stereo/Dataset_stereo.py).

``Dataset_stereo[i]`` is the reference's sample: the fp32 (H, W, C) array imL | imR [| dispL
[| dispR]] of the files cropped centre-bottom to ``size_min``, mirrored when ``Train`` and C is even
and ``np.random.rand() > 0.5`` (so a 7-channel sample never flips, as in the reference), then
``transform``; and the left image's file name.  ``raw_item(i)`` is the same sample before any of
that: the decoded arrays as they are plus the crop's origin, what ``DeviceLoader`` ships to the
device for ``costvolume.stereo_spatial_raw`` to do the rest there.

Kept divergences: a decode error raises with the four paths, where the reference logs
it and retries another index; 16-bit disparity PNGs read as value / 256 (KITTI's encoding) unless
``disp_png="raw"``.
"""
import os

import numpy as np

from .. import _lib
from ..img_rw import imread, load_disp
from .stereo_check import disp_values


def Datasets_stereo(datasets):
    """Merge into the first dataset (Dataset_stereo.py:18-45): the path lists are extended; a
    disparity list becomes None as soon as one dataset lacks it; size_min is the minimum."""
    assert len(datasets) > 0
    dataset = datasets[0]
    for other in datasets[1:]:
        assert dataset.Train == other.Train
        assert dataset.disp_png == other.disp_png
        dataset.paths_img_left.extend(other.paths_img_left)
        dataset.paths_img_right.extend(other.paths_img_right)
        if dataset.paths_disp_left is not None:
            if other.paths_disp_left is None:
                dataset.paths_disp_left = None
            else:
                dataset.paths_disp_left.extend(other.paths_disp_left)
            if dataset.paths_disp_right is not None:
                if other.paths_disp_right is None:
                    dataset.paths_disp_right = None
                else:
                    dataset.paths_disp_right.extend(other.paths_disp_right)
        if other.size_min is not None:
            if dataset.size_min is not None:
                dataset.size_min[0] = min(dataset.size_min[0], other.size_min[0])
                dataset.size_min[1] = min(dataset.size_min[1], other.size_min[1])
            else:
                dataset.size_min = other.size_min
    return dataset


class Dataset_stereo(object):
    def __init__(self, paths_img_left, paths_img_right, paths_disp_left=None, paths_disp_right=None,
                 transform=None, loader_img=imread, loader_disp=load_disp, size_min=None, Train=False,
                 disp_png="kitti"):
        if disp_png not in ("kitti", "raw"):
            raise ValueError("disp_png is 'kitti' (uint16 / 256) or 'raw', got %r" % (disp_png,))
        self.paths_img_left = paths_img_left
        self.paths_img_right = paths_img_right
        self.paths_disp_left = paths_disp_left
        self.paths_disp_right = paths_disp_right
        self.loader_img = loader_img
        self.loader_disp = loader_disp
        self.transform = transform
        self.size_min = size_min
        self.Train = Train
        self.disp_png = disp_png

    def __len__(self):
        return len(self.paths_img_left)

    @property
    def channels(self):
        """6 without disparities, 7 with the left one, 8 with both (a right one alone is not read)."""
        if self.paths_disp_left is None:
            return 6
        return 7 if self.paths_disp_right is None else 8

    def crop_origin(self, h, w):
        """(y0, x0) of Crop_center_bottom's window in an h x w plane (Dataset_stereo.py:63-74)."""
        if self.size_min is None:
            return 0, 0
        h_min, w_min = self.size_min
        assert h_min <= h and w_min <= w
        return h - h_min, (w - w_min) // 2

    def Crop_center_bottom(self, img):
        if self.size_min is None:
            return img
        y0, x0 = self.crop_origin(*img.shape[:2])
        return img[y0:y0 + self.size_min[0], x0:x0 + self.size_min[1]]

    def paths(self, index):
        return [p[index] for p in (self.paths_img_left, self.paths_img_right, self.paths_disp_left,
                                   self.paths_disp_right)[:2 + self.channels - 6]]

    def raw_item(self, index):
        """``(planes, (y0, x0), (H0, W0), filename)``: the decoded arrays untouched -- imL, imR
        (Hs, Ws, 3) uint8, then dispL [, dispR] (Hs, Ws) uint8 / uint16 / float32 -- and the crop
        they are to get.  No float conversion, no crop, no flip."""
        paths = self.paths(index)
        try:
            planes = [np.ascontiguousarray(self.loader_img(p)) for p in paths[:2]]
            for p in paths[2:]:
                d = np.asarray(self.loader_disp(p))
                if d.dtype not in (np.uint8, np.uint16, np.float32):
                    if d.dtype.kind not in "iu" or d.min() < 0 or d.max() > 65535:
                        raise ValueError("a disparity is neither 8/16-bit nor float32: %s" % d.dtype)
                    d = d.astype(np.uint16)                      # a 16-bit PNG decoded into int32
                planes.append(np.ascontiguousarray(d))
            hw = planes[0].shape[:2]
            if any(p.shape != hw + (3,) or p.dtype != np.uint8 for p in planes[:2]):
                raise ValueError("the images are not 8-bit RGB of one size: %s" % [(p.dtype, p.shape) for p in planes[:2]])
            if any(p.shape != hw for p in planes[2:]):
                raise ValueError("the planes differ in size: %s" % [p.shape for p in planes])
        except Exception as err:
            raise RuntimeError("Dataset_stereo: cannot load sample %d %s: %s" % (index, paths, err))
        y0, x0 = self.crop_origin(*hw)
        size = tuple(self.size_min) if self.size_min is not None else hw
        return planes, (y0, x0), size, os.path.basename(paths[0])

    def disp_format(self, plane):
        if plane.dtype == np.float32:
            return _lib.DSM_DISP_F32
        if plane.dtype == np.uint16:
            return _lib.DSM_DISP_U16_256 if self.disp_png == "kitti" else _lib.DSM_DISP_U16
        return _lib.DSM_DISP_U8

    def __getitem__(self, index):
        paths = self.paths(index)
        try:
            parts = [np.float32(self.Crop_center_bottom(self.loader_img(p))) for p in paths[:2]]
            for p in paths[2:]:
                disp = self.Crop_center_bottom(self.loader_disp(p))[:, :, None]
                parts.append(disp_values(disp, self.disp_png))
            img = np.concatenate(parts, axis=2)
        except Exception as err:
            raise RuntimeError("Dataset_stereo: cannot load sample %d %s: %s" % (index, paths, err))
        if self.Train and img.shape[2] % 2 == 0 and np.random.rand() > 0.5:
            img = np.flip(img, axis=1).copy()
        if self.transform is not None:
            img = self.transform(img)
        return img, os.path.basename(paths[0])
