"""CPU: the dataset layer (dsmnet_amd/datasets) on synthetic trees written under tmp_path: path
groups per dataset name, the check (size_min, bad samples, the JSON cache), merging, __getitem__
against the fixture written from the reference's Dataset_stereo (tests/golden/golden_frames.npz),
raw_item, and the loader's packing."""
import json
import os

import numpy as np
import pytest

from dsmnet_amd import _lib, datasets, img_rw
from dsmnet_amd import transforms as T
from dsmnet_amd.datasets import Dataset_stereo, Datasets_stereo, check_dataset_stereo, paths_stereo_by_name
from dsmnet_amd.datasets.loader import pack_layout
from tests import dataset_trees as DT
from tests import frames_oracle as FO
from tests.conftest import Golden


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("stereo"))
    out = {"root": root,
           "kitti2015-tr": DT.write_kitti(root, "kitti2015-tr", seed=10),
           "kitti2012-tr": DT.write_kitti(root, "kitti2012-tr", sizes=DT.SIZES[:2], seed=11),
           "kitti-raw": DT.write_kitti_raw(root),
           "flyingthings3d-tr": DT.write_flyingthings(root)}
    return out


def test_path_groups(trees):
    root = trees["root"]
    k15 = paths_stereo_by_name("kitti2015-tr", root)
    assert k15.count == 3 and k15.flag_dataset == "kitti2015-tr"
    assert k15.get_paths_idx(1) == [root + "/data_scene_flow/training/image_2/000001_10.png",
                                    root + "/data_scene_flow/training/image_3/000001_10.png",
                                    root + "/data_scene_flow/training/disp_occ_0/000001_10.png"]
    assert [g[0] for g in k15.paths_all] == sorted(g[0] for g in k15.paths_all)          # sorted, *_11 ignored
    k12 = paths_stereo_by_name("KITTI2012-TR", root)                                      # the name is case-blind
    assert k12.get_paths_idx(0) == [root + "/data_stereo_flow/training/colored_0/000000_10.png",
                                    root + "/data_stereo_flow/training/colored_1/000000_10.png",
                                    root + "/data_stereo_flow/training/disp_occ/000000_10.png"]
    raw = paths_stereo_by_name("kitti-raw", root)
    assert raw.count == 2 and all(len(g) == 2 for g in raw.paths_all)
    g = sorted(raw.paths_all)[0]
    assert g == [root + "/raw/2011_09_26/drive_0000_sync/image_02/data/0000000000.png",
                 root + "/raw/2011_09_26/drive_0000_sync/image_03/data/0000000000.png"]
    ft = paths_stereo_by_name("flyingthings3d-tr", root)
    assert sorted(ft.paths_all)[0] == [root + "/flyingthings3d/frames_finalpass_webp/TRAIN/A/0000/left/0006.webp",
                                       root + "/flyingthings3d/frames_finalpass_webp/TRAIN/A/0000/right/0006.webp",
                                       root + "/flyingthings3d/disparity/TRAIN/A/0000/left/0006.pfm",
                                       root + "/flyingthings3d/disparity/TRAIN/A/0000/right/0006.pfm"]
    assert all(os.path.isfile(p) for grp in k15.paths_all + k12.paths_all + raw.paths_all + ft.paths_all for p in grp)
    for name in ("kitti2015-te", "kitti2012-te", "flyingthings3d-te", "driving", "monkaa", "stereo-list", "nonesuch"):
        empty = paths_stereo_by_name(name, root)
        assert empty.paths_all == [] and empty.count == 0
        with pytest.raises(AssertionError, match="do not exist"):
            empty.get_paths_idx(0)


def test_a_root_that_contains_the_substituted_words(tmp_path):
    """The substitutions act behind the root only: a root named '.../left_image_2' is left alone."""
    root = str(tmp_path / "left_image_2")
    DT.write_kitti(root, "kitti2015-tr", sizes=DT.SIZES[:1])
    g = paths_stereo_by_name("kitti2015-tr", root).get_paths_idx(0)
    assert all(p.startswith(root + "/data_scene_flow") and os.path.isfile(p) for p in g) and "image_3" in g[1]


def test_stereo_list(trees, tmp_path):
    root = str(tmp_path / "mylist")
    groups = paths_stereo_by_name("kitti2015-tr", trees["root"]).paths_all
    DT.write_list(root, groups)
    lst = paths_stereo_by_name("stereo-list", root)
    assert lst.flag_dataset == "list(mylist)" and lst.paths_all == groups
    paths, size_min = check_dataset_stereo("stereo-list", root).getpaths()
    assert paths[:3] == [list(c) for c in zip(*groups)] and paths[3] is None and size_min == [12, 40]
    assert os.path.isfile(os.path.join(root, "paths", "list(mylist).json"))


def test_check_size_min_bad_samples_and_the_cache(tmp_path):
    root = str(tmp_path)
    sizes = DT.SIZES + ((9, 30), (20, 50))
    samples = DT.write_kitti(root, "kitti2015-tr", sizes=sizes, seed=3)
    sub = os.path.join(root, "data_scene_flow", "training")
    # sample 3 (the smallest): more than 20 % of its disparity above W / 3 px
    far = np.full((9, 30), 11 * 256, np.uint16)
    far[:, :20] = 5 * 256
    DT._save(os.path.join(sub, "disp_occ_0", "000003_10.png"), far)
    # sample 4: no right image
    os.remove(os.path.join(sub, "image_3", "000004_10.png"))
    chk = check_dataset_stereo("kitti2015-tr", root)
    assert chk.checkdisp(np.float32(far) / 256) is False
    far[:, 25:] = 5 * 256                                     # 5 of 30 columns: 16.7 %
    assert chk.checkdisp(np.float32(far) / 256) is True
    paths, size_min = chk.getpaths()
    assert [len(p) for p in paths[:3]] == [3, 3, 3] and paths[3] is None
    assert [os.path.basename(p) for p in paths[0]] == ["%06d_10.png" % i for i in range(3)]
    # h / w are minima over the right images seen: as in the reference, sample 3's right image
    # counts although its disparity then fails
    assert size_min == [9, 30]
    good, bad = (os.path.join(root, "paths", "kitti2015-tr" + s) for s in (".json", "_bad.json"))
    assert json.load(open(good)) == [paths[:3], 9, 30]
    assert [os.path.basename(p) for p in json.load(open(bad))[0]] == ["000003_10.png", "000004_10.png"]
    # raw 16-bit values: every disparity is 'too far', every sample bad
    os.rename(good, good + ".kept"), os.rename(bad, bad + ".kept")
    raw_paths, _ = check_dataset_stereo("kitti2015-tr", root, disp_png="raw").getpaths()
    assert raw_paths[0] == []
    os.rename(good + ".kept", good), os.rename(bad + ".kept", bad)
    # a cache that exists is used: edit it and remove a file it names
    json.dump([[p[:2] for p in paths[:3]], 7, 8], open(good, "w"))
    os.remove(paths[0][2])
    again, size_again = check_dataset_stereo("kitti2015-tr", root).getpaths()
    assert again == [paths[0][:2], paths[1][:2], paths[2][:2], None] and size_again == [7, 8]
    del samples


def test_check_reads_sizes_and_rejects_undecodable_files(trees, tmp_path):
    root = str(tmp_path)
    DT.write_kitti(root, "kitti2012-tr", sizes=DT.SIZES, seed=4)
    broken = os.path.join(root, "data_stereo_flow", "training", "colored_0", "000001_10.png")
    with open(broken, "wb") as f:
        f.write(b"not a png")
    paths, size_min = check_dataset_stereo("kitti2012-tr", root).getpaths()
    assert [os.path.basename(p) for p in paths[0]] == ["000000_10.png", "000002_10.png"] and size_min == [13, 40]
    ft_paths, ft_size = check_dataset_stereo("flyingthings3d-tr", trees["root"]).getpaths()
    assert [len(p) for p in ft_paths] == [2, 2, 2, 2] and ft_size == [12, 41]
    with pytest.raises(AssertionError, match="do not exist"):
        check_dataset_stereo("monkaa", root)
    with pytest.raises(AssertionError):
        check_dataset_stereo("kitti2012-tr", os.path.join(root, "nowhere"))


def _ds(c, size_min=(3, 4), train=False):
    lists = [["%s%d" % (k, i) for i in range(2)] for k in "abcd"]
    return Dataset_stereo(lists[0], lists[1], lists[2] if c >= 7 else None, lists[3] if c >= 8 else None,
                          size_min=None if size_min is None else list(size_min), Train=train)


def test_datasets_stereo_merging():
    m = Datasets_stereo([_ds(8, (5, 9)), _ds(8, (6, 7))])
    assert len(m) == 4 and m.channels == 8 and m.size_min == [5, 7]
    assert m.paths_disp_right == ["d0", "d1", "d0", "d1"]
    m = Datasets_stereo([_ds(8), _ds(7)])                    # the right disparities go, the left ones stay
    assert m.paths_disp_right is None and len(m.paths_disp_left) == 4 and m.channels == 7
    m = Datasets_stereo([_ds(8), _ds(6), _ds(8)])            # None propagates: no disparity at all, for good
    assert m.paths_disp_left is None and m.paths_disp_right is None and m.channels == 6 and len(m) == 6
    m = Datasets_stereo([_ds(6), _ds(8)])                    # the first has none: nothing is added
    assert m.paths_disp_left is None and m.paths_disp_right is None
    m = Datasets_stereo([_ds(7, None), _ds(7, (4, 4))])
    assert m.size_min == [4, 4]
    m = Datasets_stereo([_ds(7, (4, 4)), _ds(7, None)])
    assert m.size_min == [4, 4]
    with pytest.raises(AssertionError):
        Datasets_stereo([_ds(7, train=True), _ds(7, train=False)])
    with pytest.raises(AssertionError):
        Datasets_stereo([])


def _golden_dataset(gold, planes, train, disp_png="raw"):
    store = {k: gold[k] for k in gold.z.files if k.startswith("s")}
    n = len(gold.meta["sizes"])
    lists = [["s%d.%s" % (i, k) for i in range(n)] for k in ("imL", "imR", "dispL", "dispR")[:planes]] + [None] * (4 - planes)
    return Dataset_stereo(lists[0], lists[1], lists[2], lists[3], loader_img=store.__getitem__,
                          loader_disp=store.__getitem__, size_min=list(gold.meta["size_min"]), Train=train,
                          disp_png=disp_png), store


@pytest.mark.parametrize("case", ["c8_train", "c8_eval", "c7_train", "c6_train"])
def test_getitem_against_the_reference_fixture(case):
    gold = Golden("frames")
    meta = gold.meta["cases"][case]
    ds, _ = _golden_dataset(gold, meta["planes"], meta["train"])
    np.random.seed(meta["seed"])
    got = [ds[i] for i in range(len(ds))]
    assert float(np.random.rand()) == float(gold[case + ".next_rand"])          # the same draws
    for i, (img, name) in enumerate(got):
        assert img.dtype == np.float32 and name == "s%d.imL" % i
        assert np.array_equal(img, gold[case + ".out"][i]), (case, i)
    if case == "c8_train":
        assert sorted(meta["flips"]) == [False, False, True]                     # both outcomes are in the fixture
    if case == "c7_train":                                                       # 7 channels never flip, and draw nothing
        assert meta["flips"] == [False] * 3
        np.random.seed(meta["seed"])
        first = float(np.random.rand())
        np.random.seed(meta["seed"])
        ds[0]
        assert float(np.random.rand()) == first
    seen = []
    ds.transform = lambda img: seen.append(img.shape) or "transformed"
    assert ds[0][0] == "transformed" and seen == [(12, 40, meta["planes"] + 4)]


def test_kitti_disparities_are_value_over_256_by_default(trees):
    root = trees["root"]
    ds = datasets.dataset_stereo_by_name("kitti2015-tr_kitti2012-tr", root, Train=False)
    assert len(ds) == 5 and ds.channels == 7 and ds.size_min == [12, 40] and ds.disp_png == "kitti"
    samples = trees["kitti2015-tr"] + trees["kitti2012-tr"]
    for i in (0, 1, 4):
        img, name = ds[i]
        assert name == "%06d_10.png" % (i if i < 3 else i - 3)
        assert np.array_equal(img, FO.frame(samples[i], [12, 40], False, FO.DISP_U16_256))
        assert np.array_equal(img[:, :, 6] * 256, FO.frame(samples[i], [12, 40], False, FO.DISP_U16)[:, :, 6])
    raw = Dataset_stereo(ds.paths_img_left, ds.paths_img_right, ds.paths_disp_left, size_min=[12, 40], disp_png="raw")
    assert np.array_equal(raw[2][0], FO.frame(samples[2], [12, 40], False, FO.DISP_U16))
    assert np.array_equal(raw[2][0][:, :, 6], img_rw.load_disp(ds.paths_disp_left[2])[-12:, :40].astype(np.float32))
    with pytest.raises(ValueError):
        Dataset_stereo([], [], disp_png="high-byte")


def test_raw_item_and_decode_errors(trees):
    root = trees["root"]
    ds = datasets.dataset_stereo_by_name("kitti2015-tr", root, Train=True)
    planes, origin, size, name = ds.raw_item(0)
    assert [p.dtype for p in planes] == [np.uint8, np.uint8, np.uint16] and name == "000000_10.png"
    assert [p.shape for p in planes] == [(13, 41, 3), (13, 41, 3), (13, 41)] and origin == (1, 0) and size == (12, 40)
    assert all(np.array_equal(a, b) for a, b in zip(planes, trees["kitti2015-tr"][0]))
    assert ds.raw_item(1)[1] == (0, 2) and ds.raw_item(2)[1] == (2, 0)
    assert ds.disp_format(planes[2]) == _lib.DSM_DISP_U16_256
    ft = datasets.dataset_stereo_by_name("flyingthings3d-tr", root, Train=True)
    planes, origin, size, _ = ft.raw_item(0)
    assert [p.dtype for p in planes] == [np.uint8, np.uint8, np.float32, np.float32] and ft.channels == 8
    want = sorted(trees["flyingthings3d-tr"], key=lambda s: s[0].shape != planes[0].shape)[0]
    assert all(np.array_equal(a, b) for a, b in zip(planes, want))               # lossless webp, pfm
    assert ft.disp_format(planes[2]) == _lib.DSM_DISP_F32 and ft.disp_format(planes[0][:, :, 0]) == _lib.DSM_DISP_U8
    rawmode = Dataset_stereo(ds.paths_img_left, ds.paths_img_right, ds.paths_disp_left, disp_png="raw")
    assert rawmode.disp_format(ds.raw_item(0)[0][2]) == _lib.DSM_DISP_U16
    gone = Dataset_stereo(ds.paths_img_left, [p + ".gone" for p in ds.paths_img_right], ds.paths_disp_left)
    for fn in (gone.raw_item, gone.__getitem__):
        with pytest.raises(RuntimeError) as e:                                   # no retry on another index
            fn(1)
        assert ds.paths_img_left[1] in str(e.value) and ds.paths_disp_left[1] in str(e.value) and ".gone" in str(e.value)


def test_device_loader_refuses_other_transforms(trees):
    ds = datasets.dataset_stereo_by_name("kitti2015-tr", trees["root"], Train=True)
    for t in (T.Stereo_color(), T.Stereo_normalize(), T.Lighting(), lambda img: img, None,
              T.Spatial_stereo([8, 6], 0, 3)):
        with pytest.raises(TypeError, match="Spatial_stereo"):
            datasets.DeviceLoader(ds, t, 2)
    for t in (T.Stereo_train([8, 6], 0, 3), T.Stereo_Spatial([8, 6], 0, 3), T.Stereo_ToTensor(), T.Stereo_eval()):
        loader = datasets.DeviceLoader(ds, t, 2, threads=64)
        assert len(loader) == 2 and loader.threads == 16                         # capped, never the CPU count
    assert len(datasets.DeviceLoader(ds, T.Stereo_eval(), 2, drop_last=True)) == 1
    with pytest.raises(TypeError):
        T.Stereo_color().call_raw(None, [], (4, 4), 6)


def test_packed_offsets_respect_the_alignment_rules(trees):
    """Odd plane sizes: 13 x 41 x 3 = 1599 B of RGB puts everything behind it at odd offsets
    unless the packer aligns."""
    for name, fmts in (("kitti2015-tr", [_lib.DSM_DISP_U16_256] * 3), ("flyingthings3d-tr", [_lib.DSM_DISP_F32] * 2)):
        ds = datasets.dataset_stereo_by_name(name, trees["root"], Train=True)
        items = [ds.raw_item(i) for i in range(len(ds))]
        sources, total = pack_layout(items, fmts)
        spans = []
        for (planes, origin, _, _), s in zip(items, sources):
            assert s[4:8] == planes[0].shape[:2] + origin and s[8] == 0
            offs = list(s[:4])
            assert offs[len(planes):] == [-1] * (4 - len(planes))
            for p, off in zip(planes, offs):
                assert off % p.dtype.itemsize == 0, (name, off, p.dtype)
                spans.append((off, off + p.nbytes))
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] <= b[0] < a[1] + 4 for a, b in zip(spans, spans[1:]))    # no overlap, at most 3 B of padding
    assert any(s[0] % 2 for s in sources) or any(s[1] % 2 for s in sources)       # RGB does sit at odd offsets
