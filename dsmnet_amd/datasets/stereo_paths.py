"""The file groups of the stereo datasets by name (myDatasets_stereo/stereo_paths.py).

    paths_stereo_by_name("kitti2015-tr", root).paths_all   # [[img_left, img_right, disp_left], ...]

A group is [img_left, img_right] plus disp_left and disp_right where the dataset has them.  The
left images are found with the reference's glob pattern below ``rootpath``; the other paths follow
by substituting in the part of the path behind ``rootpath`` (so that a root that itself contains
'left' or 'image_2' cannot interfere): left -> right, image folder -> disparity folder (and the
extension, where they differ), left disparity -> right disparity.  The KITTI lists are sorted, the
others are in glob order, as in the reference.  ``stereo-list`` reads ``paths_stereo.txt``.  An
unknown name yields an empty list, and ``get_paths_idx`` then asserts.
"""
import glob
import logging
import os

log = logging.getLogger(__name__)


class paths_stereo(object):
    flag_dataset = None
    flag_img_left_right = (None, None)
    flag_img_disp_left = (None, None)
    flag_disp_left_right = (None, None)
    flag_img_type = None
    flag_disp_type = None
    flag_same_type = True
    pattern = None                      # below rootpath
    flag_sort = False

    def __init__(self, rootpath):
        self.rootpath = rootpath
        self.n_root = len(rootpath)
        self.str_filter = None if self.pattern is None else rootpath + self.pattern
        self.paths_all = [] if self.pattern is None else self.get_paths_all(self.str_filter, self.flag_sort)

    def get_group_from_left(self, path_img_left):
        sub = path_img_left[self.n_root:]
        paths = [path_img_left, self.rootpath + sub.replace(*self.flag_img_left_right)]
        if self.flag_img_disp_left[0] is None:
            return paths
        disp = sub.replace(*self.flag_img_disp_left)
        if not self.flag_same_type:
            disp = disp.replace(self.flag_img_type, self.flag_disp_type)
        paths.append(self.rootpath + disp)
        if self.flag_disp_left_right[0] is None:
            return paths
        paths.append(self.rootpath + disp.replace(*self.flag_disp_left_right))
        return paths

    def get_paths_all(self, str_filter_glob, flag_sort=False):
        lefts = glob.glob(str_filter_glob)
        if flag_sort:
            lefts.sort()
        return [self.get_group_from_left(p) for p in lefts]

    def get_paths_all_from_list(self, root, flag_sort=False):
        """``root/paths_stereo.txt`` names one list file per kind (left images, right images,
        [left disparities, [right disparities]]); list file k holds one path per line, line i of
        every list file being sample i."""
        listing = os.path.join(root, "paths_stereo.txt")
        if not os.path.isdir(root) or not os.path.isfile(listing):
            return []
        columns = []
        for name in _lines(listing):
            tpath = os.path.join(root, name)
            assert os.path.isfile(tpath), tpath
            column = _lines(tpath)
            for filepath in column:
                assert os.path.isfile(filepath), filepath
            assert not columns or len(column) == len(columns[-1])
            columns.append(column)
        if not columns:
            return []
        return [[column[i] for column in columns] for i in range(len(columns[0]))]

    def get_paths_idx(self, idx):
        assert idx < len(self.paths_all), "dataset[%s] do not exist!" % (self.flag_dataset,)
        return self.paths_all[idx]

    @property
    def count(self):
        return len(self.paths_all)


def _lines(path):
    with open(path, "r") as f:
        return [l.strip() for l in f if l.strip() != ""]


class paths_list(paths_stereo):
    def __init__(self, rootpath):
        super(paths_list, self).__init__(rootpath)
        self.flag_dataset = "list(%s)" % os.path.basename(rootpath)
        self.paths_all = self.get_paths_all_from_list(rootpath)


class _sceneflow(paths_stereo):
    flag_img_left_right = ("left", "right")
    flag_img_disp_left = ("frames_finalpass_webp", "disparity")
    flag_disp_left_right = ("left", "right")
    flag_img_type = ".webp"
    flag_disp_type = ".pfm"
    flag_same_type = False


class paths_monkaa(_sceneflow):
    flag_dataset = "monkaa"
    pattern = "/monkaa/frames_finalpass_webp/*/left/*.webp"


class paths_driving(_sceneflow):
    flag_dataset = "driving"
    pattern = "/driving/frames_finalpass_webp/*/*/*/left/*.webp"


class paths_flyingthings3d_train(_sceneflow):
    flag_dataset = "flyingthings3d-tr"
    pattern = "/flyingthings3d/frames_finalpass_webp/TRAIN/*/*/left/*.webp"


class paths_flyingthings3d_test(_sceneflow):
    flag_dataset = "flyingthings3d-te"
    pattern = "/flyingthings3d/frames_finalpass_webp/TEST/*/*/left/*.webp"


class _kitti(paths_stereo):
    flag_img_type = ".png"
    flag_disp_type = ".png"
    flag_sort = True


class paths_kitti2015_train(_kitti):
    flag_dataset = "kitti15-tr"
    flag_img_left_right = ("image_2", "image_3")
    flag_img_disp_left = ("image_2", "disp_occ_0")
    pattern = "/data_scene_flow/training/image_2/*_10.png"


class paths_kitti2015_test(_kitti):
    flag_dataset = "kitti15-te"
    flag_img_left_right = ("image_2", "image_3")
    pattern = "/data_scene_flow/testing/image_2/*_10.png"


class paths_kitti2012_train(_kitti):
    flag_dataset = "kitti12-tr"
    flag_img_left_right = ("colored_0", "colored_1")
    flag_img_disp_left = ("colored_0", "disp_occ")
    pattern = "/data_stereo_flow/training/colored_0/*_10.png"


class paths_kitti2012_test(_kitti):
    flag_dataset = "kitti12-te"
    flag_img_left_right = ("colored_0", "colored_1")
    pattern = "/data_stereo_flow/testing/colored_0/*_10.png"


class paths_kitti_raw(_kitti):
    flag_dataset = "kitti-raw"
    flag_img_left_right = ("image_02", "image_03")
    pattern = "/raw/*/*/image_02/data/*.png"
    flag_sort = False


BY_NAME = {"kitti-raw": paths_kitti_raw,
           "kitti2012-te": paths_kitti2012_test, "kitti2012-tr": paths_kitti2012_train,
           "kitti2015-te": paths_kitti2015_test, "kitti2015-tr": paths_kitti2015_train,
           "flyingthings3d-te": paths_flyingthings3d_test, "flyingthings3d-tr": paths_flyingthings3d_train,
           "driving": paths_driving, "monkaa": paths_monkaa, "stereo-list": paths_list}


class paths_stereo_by_name(object):
    def __init__(self, flag_dataset="kitti-raw", rootpath="./"):
        self.flag_dataset = flag_dataset
        self.rootpath = rootpath
        self.paths_all = self.get_paths_all_from_dataset(flag_dataset, rootpath)

    def get_paths_all_from_dataset(self, flag_dataset, rootpath):
        cls = BY_NAME.get(flag_dataset.lower())
        paths_all = []
        if cls is None:
            log.info("unknown dataset %r; the datasets are: %s", flag_dataset.lower(), ", ".join(sorted(BY_NAME)))
        else:
            if cls is paths_list:
                self.flag_dataset = "list(%s)" % os.path.basename(rootpath)
            paths_all = cls(rootpath).paths_all
        self.__init_sucessed__ = paths_all != []
        return paths_all

    def get_paths_idx(self, idx):
        assert self.__init_sucessed__, "dataset[%s] do not exist!" % (self.flag_dataset,)
        return self.paths_all[idx]

    @property
    def count(self):
        return len(self.paths_all)
