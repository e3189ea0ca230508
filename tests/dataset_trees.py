"""Synthetic dataset trees in the layouts dsmnet_amd/datasets/stereo_paths.py looks for, written
with PIL and img_rw.save_pfm from a seed; each writer returns the arrays it wrote, sample by
sample, as [imL, imR, dispL, dispR] (absent ones left out)."""
import os

import numpy as np
from PIL import Image

from dsmnet_amd import img_rw

SIZES = ((13, 41), (12, 44), (14, 40))          # three sizes; size_min = [12, 40]


def _rgb(rng, h, w):
    return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def disp_u16(rng, h, w, max_px=None):
    """16-bit KITTI-style disparity: value / 256 px, below a third of the width, 20 % holes."""
    top = int((w // 3 if max_px is None else max_px) * 256)
    d = rng.randint(1, top, size=(h, w)).astype(np.uint16)
    d[rng.rand(h, w) < 0.2] = 0
    return d


def _save(path, a):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.endswith(".pfm"):
        img_rw.save_pfm(path, a)
    elif path.endswith(".webp"):
        Image.fromarray(a).save(path, lossless=True)
    else:
        Image.fromarray(a).save(path)
    return path


def write_kitti(root, name="kitti2015-tr", sizes=SIZES, seed=0):
    """kitti2015-tr / kitti2012-tr: 8-bit RGB pairs and a 16-bit left disparity."""
    sub, left, right, disp = {"kitti2015-tr": ("data_scene_flow/training", "image_2", "image_3", "disp_occ_0"),
                              "kitti2012-tr": ("data_stereo_flow/training", "colored_0", "colored_1", "disp_occ")}[name]
    rng = np.random.RandomState(seed)
    samples = []
    for i, (h, w) in enumerate(sizes):
        planes = [_rgb(rng, h, w), _rgb(rng, h, w), disp_u16(rng, h, w)]
        for folder, a in zip((left, right, disp), planes):
            _save(os.path.join(root, sub, folder, "%06d_10.png" % i), a)
        _save(os.path.join(root, sub, left, "%06d_11.png" % i), planes[0])       # not a *_10 frame: ignored
        samples.append(planes)
    return samples


def write_kitti_raw(root, sizes=SIZES[:2], seed=1):
    rng = np.random.RandomState(seed)
    samples = []
    for i, (h, w) in enumerate(sizes):
        planes = [_rgb(rng, h, w), _rgb(rng, h, w)]
        for cam, a in zip(("image_02", "image_03"), planes):
            _save(os.path.join(root, "raw", "2011_09_26", "drive_%04d_sync" % i, cam, "data", "%010d.png" % i), a)
        samples.append(planes)
    return samples


def write_flyingthings(root, sizes=SIZES[:2], seed=2):
    """flyingthings3d-tr: lossless .webp pairs, float32 .pfm disparities for both sides."""
    rng = np.random.RandomState(seed)
    samples = []
    for i, (h, w) in enumerate(sizes):
        planes = [_rgb(rng, h, w), _rgb(rng, h, w)]
        for _ in range(2):
            d = (rng.rand(h, w) * (w // 3)).astype(np.float32)
            d[rng.rand(h, w) < 0.2] = 0
            planes.append(d)
        scene = os.path.join("TRAIN", "A", "%04d" % i)
        for kind, side, ext, a in (("frames_finalpass_webp", "left", ".webp", planes[0]),
                                   ("frames_finalpass_webp", "right", ".webp", planes[1]),
                                   ("disparity", "left", ".pfm", planes[2]), ("disparity", "right", ".pfm", planes[3])):
            _save(os.path.join(root, "flyingthings3d", kind, scene, side, "%04d%s" % (i + 6, ext)), a)
        samples.append(planes)
    return samples


def write_list(root, groups):
    """stereo-list: ``paths_stereo.txt`` names one list file per kind; ``groups`` = [[imL, imR, ...], ...]."""
    os.makedirs(root, exist_ok=True)
    names = ["left.txt", "right.txt", "disp_left.txt", "disp_right.txt"][:len(groups[0])]
    for k, name in enumerate(names):
        with open(os.path.join(root, name), "w") as f:
            f.write("\n".join(g[k] for g in groups) + "\n\n")
    with open(os.path.join(root, "paths_stereo.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
