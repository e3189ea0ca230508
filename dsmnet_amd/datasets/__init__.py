"""The reference's dataset layer (myDatasets_stereo/) and a loader that ends in device batches.

    dataset = dataset_stereo_by_name("kitti2015-tr_kitti2012-tr", root, Train=True)
    loader = DeviceLoader(dataset, transforms.Stereo_train([768, 384], 0.4, 32), batch_size=4, shuffle=True)
    for batch, filenames in loader:
        loss, d1, epe = train.train_step(model, optim, lossfun, batch)
"""
from .Dataset_stereo import Dataset_stereo, Datasets_stereo
from .loader import DeviceLoader
from .stereo_check import check_dataset_stereo
from .stereo_paths import paths_stereo_by_name


def dataset_stereo_by_name(names_dataset="kitti2015-tr_kitti2012-tr", root="./kitti", transform=None, Train=True,
                           disp_png="kitti"):
    """The datasets named in ``names_dataset`` ('_'-separated), checked and merged
    (myDatasets_stereo/__init__.py:7-15).  ``disp_png``: 'kitti' reads 16-bit disparity PNGs as
    value / 256, 'raw' as the value (what ``img_rw.load_disp`` returns)."""
    datasets = []
    for name in names_dataset.split("_"):
        paths, size_min = check_dataset_stereo(name, root, disp_png=disp_png).getpaths()
        assert len(paths) == 4
        datasets.append(Dataset_stereo(paths[0], paths[1], paths[2], paths[3], transform=transform,
                                       size_min=size_min, Train=Train, disp_png=disp_png))
    return Datasets_stereo(datasets)
