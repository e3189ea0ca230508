"""Check a stereo dataset's file groups and remember the result (myDatasets_stereo/stereo_check.py).

    paths, size_min = check_dataset_stereo("kitti2015-tr", root).getpaths()
    # paths = [img_left[], img_right[], disp_left[] or None, disp_right[] or None]; size_min = [h, w]

A group is bad when one of its files is missing or cannot be decoded, or when a disparity fails
``checkdisp`` (more than 20 % of it above a third of the width).  ``h`` / ``w`` are the minima over
the right images that were read: as in the reference, a group whose disparity then fails has
already counted.  The result is kept under ``<root>/paths/<name>.json``
and ``<name>_bad.json``; a cache that exists is used.  JSON, where the reference pickles: this
project does not execute pickles.  Image sizes come from the file header (PIL opens lazily;
``verify`` then checks the file without keeping pixels); disparities are decoded, ``checkdisp``
needs their values.  ``disp_png="kitti"`` reads 16-bit disparities as value / 256.
"""
import json
import logging
import os

import numpy as np

from .. import img_rw
from .stereo_paths import paths_stereo_by_name

log = logging.getLogger(__name__)


def image_size(path):
    """(h, w) of an image file, from its header where the decoder allows it."""
    if path.find(".pfm") > 0:
        return img_rw.load_pfm(path)[0].shape[:2]
    try:
        from PIL import Image
    except ImportError:
        return img_rw.imread(path).shape[:2]
    with Image.open(path) as im:
        w, h = im.size
        im.verify()
    return h, w


def disp_values(disp, disp_png="kitti"):
    """The float32 disparities a decoded plane stands for: uint16 is value / 256 (KITTI's
    encoding) unless ``disp_png == "raw"``; everything else is the value itself."""
    if disp.dtype == np.uint16 and disp_png == "kitti":
        return np.float32(disp) / np.float32(256.0)
    return np.float32(disp)


class check_dataset_stereo(object):
    def __init__(self, name="kitti2015-tr", root="./kitti", disp_png="kitti"):
        if disp_png not in ("kitti", "raw"):
            raise ValueError("disp_png is 'kitti' (uint16 / 256) or 'raw', got %r" % (disp_png,))
        self.name, self.root, self.disp_png = name, root, disp_png
        assert os.path.isdir(self.root), "dataset[%s] do not exist! \n " % (self.name,)
        self.paths_good = None
        self.h = 100000
        self.w = 100000
        self.paths_all = paths_stereo_by_name(self.name, self.root)
        self.name = self.paths_all.flag_dataset
        assert self.paths_all.count > 0, "dataset[%s] do not exist! \n " % (self.name,)
        self.idxs = range(self.paths_all.count)

    def checkdisp(self, disp):
        assert len(disp.shape) == 2
        return not (disp > disp.shape[1] / 3.0).mean() > 0.2

    def checkgroup(self, paths_group):
        assert type(paths_group) == list
        for j, path in enumerate(paths_group):
            try:
                assert os.path.exists(path), "no such file"
                if j < 2:
                    h, w = image_size(path)
                    if j == 1:
                        self.h, self.w = min(self.h, h), min(self.w, w)
                elif not self.checkdisp(disp_values(img_rw.load_disp(path), self.disp_png)):
                    return False
            except Exception as err:
                log.error("an error occurred when checking img(%s): %s", path, err)
                return False
        return True

    def checkpaths_file(self, savepath, savepath_bad):
        if os.path.exists(savepath) and os.path.exists(savepath_bad):
            with open(savepath, "r") as f:
                paths_good, self.h, self.w = json.load(f)
            with open(savepath_bad, "r") as f:
                paths_bad = json.load(f)
            return [paths_good, paths_bad]
        return None

    def checkpaths(self):
        log.info("checking stereo dataset paths: %s", self.name)
        n = len(self.paths_all.get_paths_idx(0))
        paths_good, paths_bad = [[] for _ in range(n)], [[] for _ in range(n)]
        for idx in self.idxs:
            group = self.paths_all.get_paths_idx(idx)
            into = paths_good if self.checkgroup(group) else paths_bad
            for j in range(n):
                into[j].append(group[j])
        return [paths_good, paths_bad]

    def checkandsavepath(self):
        dirpath = os.path.join(self.root, "paths")
        if not os.path.exists(dirpath):
            os.mkdir(dirpath)
        savepath = os.path.join(dirpath, "%s.json" % self.name)
        savepath_bad = os.path.join(dirpath, "%s_bad.json" % self.name)
        paths = self.checkpaths_file(savepath, savepath_bad)
        if paths is not None:
            paths_good, paths_bad = paths
        else:
            paths_good, paths_bad = self.checkpaths()
            with open(savepath, "w") as f:
                json.dump([paths_good, self.h, self.w], f)
            with open(savepath_bad, "w") as f:
                json.dump(paths_bad, f)
        log.info("dataset Name: %s, Count_good: %d, Count_bad: %d", self.name, len(paths_good[0]), len(paths_bad[0]))
        self.paths_good = paths_good
        self.paths_bad = paths_bad

    def getpaths(self):
        if self.paths_good is None:
            self.checkandsavepath()
        paths = list(self.paths_good)
        while len(paths) < 4:
            paths.append(None)
        return paths, [self.h, self.w]
