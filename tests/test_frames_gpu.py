"""GPU: dsm_stereo_spatial_raw (csrc/frames.hip) and datasets.DeviceLoader.  Every comparison is
``torch.equal`` against the existing path -- ``costvolume.stereo_spatial`` (or the existing
transforms) on fp32 frames assembled on the host by tests/frames_oracle.py, same records, same
seeds: uint8 -> float and uint16 / 256 are exact and the float sequence is shared
(csrc/spatial_taps.hpp), so no tolerance is involved."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dataset_trees as DT
from tests import frames_oracle as FO

pytestmark = pytest.mark.gpu

SIZES = ((13, 37), (11, 41), (12, 39))          # frame 11 x 37; crop origins (2, 0), (0, 2), (1, 1)
FRAME = (11, 37)
FORMATS = (FO.DISP_F32, FO.DISP_U16_256, FO.DISP_U16, FO.DISP_U8)

# crop only, out 6 x 20: the window touches the frame's last row and the shifted frame's last
# column (the right view then reads the frame's last column), with and without a shift
CROP_HW = (6, 20)
CROP = [(0, 17, 5, 20, 6, 0, 1.0, 1.0, 1.0), (3, 2, 1, 20, 6, 0, 1.0, 1.0, 1.0), (5, 12, 5, 20, 6, 0, 1.0, 1.0, 1.0)]


def _resize(shift, ws, hs, w, h, out_hw, scale_rand):
    return (shift, ws, hs, w, h, 1, scale_rand, 1.0 / (float(out_hw[1]) / w), 1.0 / (float(out_hw[0]) / h))


# resize, out 9 x 25: up from 4 x 11, down from 11 x 34 (the whole shifted frame: last row, last
# column), and a same-size window (every weight 0) with a shift and a scale
RESIZE_HW = (9, 25)
RESIZE = [_resize(2, 24, 7, 11, 4, RESIZE_HW, 1.37), _resize(3, 0, 0, 34, 11, RESIZE_HW, 0.43),
          _resize(4, 5, 2, 25, 9, RESIZE_HW, 0.97)]


def _disp(rng, h, w, fmt):
    if fmt == FO.DISP_F32:
        d = (rng.rand(h, w) * 220 - 20).astype(np.float32)
        kind = rng.randint(0, 12, size=(h, w))                 # a third: exact 0, inf, -inf, nan
        for k, v in enumerate((0.0, np.inf, -np.inf, np.nan)):
            d[kind == k] = v
        return d
    d = rng.randint(0, 256 if fmt == FO.DISP_U8 else 65536, size=(h, w))
    d[rng.rand(h, w) < 0.25] = 0
    return d.astype(FO.DISP_DTYPE[fmt])


def _samples(sizes, C, fmt, seed):
    rng = np.random.RandomState(seed)
    return [[rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(2)] +
            [_disp(rng, h, w, fmt) for _ in range(C - 6)] for h, w in sizes]


def _pack(samples, frame_hw, flips, fmt, odd=True):
    """One byte buffer and the sources (centre-bottom origins).  ``odd``: the RGB planes start at
    odd offsets; disparities are aligned to their element size."""
    chunks, sources, at = [], [], 0
    for planes, flip in zip(samples, flips):
        offs = []
        for i, p in enumerate(planes):
            align = p.dtype.itemsize if i >= 2 else 1
            pad = -at % align + (1 if i < 2 and odd and (at + -at % align) % 2 == 0 else 0)
            chunks.append(np.full(pad, 0xA5, np.uint8))
            at += pad
            offs.append(at)
            chunks.append(p.reshape(-1).view(np.uint8))
            at += p.nbytes
        offs += [-1] * (4 - len(offs))
        y0, x0 = FO.crop_origin(planes[0].shape[:2], frame_hw)
        sources.append(tuple(offs) + planes[0].shape[:2] + (y0, x0, int(flip), fmt))
    return np.concatenate(chunks), sources


def _both(samples, frame_hw, flips, fmt, records, hw, channels=6, odd=True):
    """(raw path, existing path on host-assembled frames), both on the device."""
    from dsmnet_amd import costvolume as cv
    C = 4 + len(samples[0])
    raw, sources = _pack(samples, frame_hw, flips, fmt, odd)
    if odd:
        assert all(s[0] % 2 == 1 and s[1] % 2 == 1 for s in sources)
    frames = np.stack([FO.frame(p, frame_hw, f, fmt) for p, f in zip(samples, flips)])
    assert frames.shape == (len(samples),) + tuple(frame_hw) + (C,) and np.isfinite(frames).all()
    got = cv.stereo_spatial_raw(torch.from_numpy(raw).cuda(), sources, records, frame_hw, C, hw, channels)
    want = cv.stereo_spatial(torch.from_numpy(frames).cuda(), records, hw, channels)
    assert got.shape == want.shape == (len(samples), C) + tuple(hw) and got.is_contiguous()
    return got, want


@pytest.mark.parametrize("flips", [(0, 0, 0), (1, 1, 1)], ids=["noflip", "flip"])
@pytest.mark.parametrize("fmt", FORMATS, ids=["f32", "u16_256", "u16", "u8"])
@pytest.mark.parametrize("C", [6, 7, 8])
def test_raw_equals_the_fp32_path(hip_lib, C, fmt, flips):
    assert [FO.crop_origin(s, FRAME) for s in SIZES] == [(2, 0), (0, 2), (1, 1)]
    samples = _samples(SIZES, C, fmt, 100 * C + 10 * fmt + flips[0])
    for records, hw in ((CROP, CROP_HW), (RESIZE, RESIZE_HW)):
        for channels in (6, 0):
            got, want = _both(samples, FRAME, flips, fmt, records, hw, channels)
            assert torch.equal(got, want), (hw, channels)
    if C == 8 and fmt != FO.DISP_F32:                      # the test does exercise the shift rule and the flip
        plain = _both(samples, FRAME, (0, 0, 0), fmt, [(0,) + r[1:] for r in CROP], CROP_HW)[0]
        got = _both(samples, FRAME, flips, fmt, CROP, CROP_HW)[0]
        assert not torch.equal(got[1], plain[1])


def test_mixed_flips_and_even_offsets(hip_lib):
    samples = _samples(SIZES, 8, FO.DISP_U16_256, 7)
    for odd in (True, False):
        got, want = _both(samples, FRAME, (1, 0, 1), FO.DISP_U16_256, RESIZE, RESIZE_HW, odd=odd)
        assert torch.equal(got, want)
    # a flip mirrors every channel and does not swap the views: identity records, no ToTensor
    ident = [(0, 0, 0, FRAME[1], FRAME[0], 0, 1.0, 1.0, 1.0)] * 3
    got, _ = _both(samples, FRAME, (1, 0, 1), FO.DISP_U16, ident, FRAME, 0)
    for b, flip in enumerate((1, 0, 1)):
        y0, x0 = FO.crop_origin(SIZES[b], FRAME)
        left = samples[b][0][y0:y0 + FRAME[0], x0:x0 + FRAME[1]].astype(np.float32).transpose(2, 0, 1)
        assert np.array_equal(got[b, :3].cpu().numpy(), left[:, :, ::-1] if flip else left)


def test_non_finite_disparities_at_the_taps(hip_lib):
    """inf, -inf, nan and 0 in turn along every row of a float32 disparity: each output pixel's
    taps meet them under a shift > 0 (the `!= 0` rule) and under both lerps.  They read as 0."""
    rng = np.random.RandomState(5)
    samples = _samples(SIZES, 8, FO.DISP_F32, 6)
    cycle = np.array([np.inf, 7.5, -np.inf, np.nan, 0.0, -3.25], np.float32)
    for planes in samples:
        for d in planes[2:]:
            h, w = d.shape
            d[:] = cycle[(np.arange(w)[None, :] + np.arange(h)[:, None] + rng.randint(6)) % 6]
    for flips in ((0, 0, 0), (1, 0, 1)):
        for records, hw in ((CROP, CROP_HW), (RESIZE, RESIZE_HW)):
            got, want = _both(samples, FRAME, flips, FO.DISP_F32, records, hw)
            assert torch.isfinite(got).all() and torch.equal(got, want)


def test_two_chunks(hip_lib):
    """B = 33: launches of 32 and 1; the last image's record and source differ from the first's."""
    from dsmnet_amd import _lib
    B = _lib.DSM_FRAMES_MAX_RECORDS + 1
    sizes = [SIZES[b % 3] for b in range(B)]
    samples = _samples(sizes, 7, FO.DISP_U16_256, 9)
    flips = [b % 2 for b in range(B - 1)] + [1]
    records = [CROP[b % 3] if b % 2 == 0 else _resize(b % 4, b % 3, b % 2, 2 + b % 5, 3, CROP_HW, 1.0 + b / 100.0)
               for b in range(B)]
    assert records[-1] != records[0] and flips[-1] != flips[0]
    got, want = _both(samples, FRAME, flips, FO.DISP_U16_256, records, CROP_HW)
    assert torch.equal(got, want)
    assert not torch.equal(got[-1], got[0])


def test_a_refused_call_leaves_y_untouched(hip_lib):
    from dsmnet_amd import _lib
    from dsmnet_amd import costvolume as cv
    samples = _samples(SIZES, 7, FO.DISP_U16, 11)
    raw, sources = _pack(samples, FRAME, (0, 1, 0), FO.DISP_U16)
    rawd = torch.from_numpy(raw).cuda()
    bad = list(CROP)
    bad[2] = (5, 13, 5, 20, 6, 0, 1.0, 1.0, 1.0)                        # one column past the shifted frame
    srcs = (_lib.FrameSource * 3)()
    recs = (_lib.SpatialRecord * 3)()
    for s, t in zip(srcs, sources):
        s.imL, s.imR, s.dispL, s.dispR, s.Hs, s.Ws, s.y0, s.x0, s.flip, s.disp_format = t
    for r, t in zip(recs, bad):
        r.shift, r.ws, r.hs, r.w, r.h, r.resize, r.scale_rand, r.scale_x, r.scale_y = t
    y = torch.full((3, 7) + CROP_HW, -7.0, device="cuda")
    rc = hip_lib.dsm_stereo_spatial_raw(ctypes.c_void_p(rawd.data_ptr()), raw.size, srcs, ctypes.c_void_p(y.data_ptr()),
                                        recs, 3, 3, 7, FRAME[0], FRAME[1], CROP_HW[0], CROP_HW[1], 6,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and (y == -7.0).all()
    with pytest.raises(_lib.DsmnetHipError):
        cv.stereo_spatial_raw(rawd, sources, bad, FRAME, 7, CROP_HW)
    with pytest.raises(_lib.DsmnetHipError):                            # a plane that ends past the buffer
        cv.stereo_spatial_raw(rawd[:-1], sources, CROP, FRAME, 7, CROP_HW)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.stereo_spatial_raw(rawd.cpu(), sources, CROP, FRAME, 7, CROP_HW)
    for args in ((rawd.float(), sources, CROP, FRAME, 7, CROP_HW), (rawd, sources, CROP[:2], FRAME, 7, CROP_HW),
                 (rawd, sources, CROP, FRAME, 9, CROP_HW), (rawd, sources, CROP, FRAME, 7, CROP_HW, 3),
                 (rawd[::2], sources, CROP, FRAME, 7, CROP_HW)):
        with pytest.raises(ValueError, match="stereo_spatial_raw"):
            cv.stereo_spatial_raw(*args)


# ---------------------------------------------------------------------------- DeviceLoader

LOADER_SIZES = tuple((14 + i % 3, 52 + (3 * i) % 7) for i in range(10))           # size_min [14, 52]


def _host_path(ds, make_transform, seed):
    """The existing path: fp32 frames assembled on the host (frames_oracle), one device tensor per
    sample, the existing transform -- drawing, per image in index order, the flip (when it is
    drawn) and then the transform's numbers, as the reference's loop does."""
    t = make_transform()
    np.random.seed(seed)
    torch.manual_seed(seed)
    outs = []
    for i in range(len(ds)):
        planes = ds.raw_item(i)[0]
        frame, _ = FO.getitem(planes, ds.size_min, ds.Train, ds.disp_format(planes[2]) if len(planes) > 2 else 0)
        outs.append(t(torch.from_numpy(frame).cuda()))
    return torch.stack(outs), (float(np.random.rand()), torch.rand(1, device="cuda").item())


def _loader_path(ds, make_transform, seed, batch_size):
    from dsmnet_amd import datasets
    np.random.seed(seed)
    torch.manual_seed(seed)
    loader = datasets.DeviceLoader(ds, make_transform(), batch_size, threads=3)
    batches = list(loader)                                   # consecutive batches, nothing waits in between
    names = [n for _, ns in batches for n in ns]
    after = (float(np.random.rand()), torch.rand(1, device="cuda").item())
    return batches, names, after


def test_loader_five_consecutive_batches_equal_the_host_path(hip_lib, tmp_path):
    """5 batches of 2 without a synchronise between them: batch k + 2 is packed into the staging
    buffer batch k was copied from, so this is the test of the staging-buffer guards."""
    from dsmnet_amd import datasets
    from dsmnet_amd import transforms as T
    DT.write_kitti(str(tmp_path), "kitti2015-tr", sizes=LOADER_SIZES, seed=21)
    ds = datasets.dataset_stereo_by_name("kitti2015-tr", str(tmp_path), Train=True)
    assert len(ds) == 10 and ds.channels == 7 and ds.size_min == [14, 52]

    def make():
        return T.Stereo_train(size_crop=[32, 8], scale_delt=0.4, shift_max=4)
    want, want_after = _host_path(ds, make, 31)
    batches, names, after = _loader_path(ds, make, 31, 2)
    torch.cuda.synchronize()
    assert len(batches) == 5 and names == ["%06d_10.png" % i for i in range(10)] and after == want_after
    for k, (batch, _) in enumerate(batches):
        assert batch.shape == (2, 7, 8, 32)
        assert torch.equal(batch, want[2 * k:2 * k + 2]), k
    assert len({b.data_ptr() for b, _ in batches}) == 5                          # new tensors, all alive


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", ["kitti-raw", "flyingthings3d-tr"])
def test_loader_flip_draws_keep_the_record_stream_aligned(hip_lib, tmp_path, name, train):
    """An even channel count (6, 8): with Train the flip's rand() is drawn before each image's
    spatial numbers; without it nothing is drawn for the flip."""
    from dsmnet_amd import datasets
    from dsmnet_amd import transforms as T
    sizes = LOADER_SIZES[:5]
    if name == "kitti-raw":
        DT.write_kitti_raw(str(tmp_path), sizes=sizes, seed=22)
    else:
        DT.write_flyingthings(str(tmp_path), sizes=sizes, seed=23)
    ds = datasets.dataset_stereo_by_name(name, str(tmp_path), Train=train)
    assert ds.channels == (6 if name == "kitti-raw" else 8)

    def make():
        return T.Stereo_train(size_crop=[32, 8], scale_delt=0.4, shift_max=4)
    seed = 0 if name == "kitti-raw" else 3
    want, want_after = _host_path(ds, make, seed)
    batches, _, after = _loader_path(ds, make, seed, 2)
    assert [b.shape[0] for b, _ in batches] == [2, 2, 1] and after == want_after
    assert torch.equal(torch.cat([b for b, _ in batches]), want)
    if train:                                                # the seeds give both outcomes of the flip
        np.random.seed(seed)
        t, flips = make(), []
        for _ in range(len(ds)):
            flips.append(np.random.rand() > 0.5)
            t.spatial.draw(*ds.size_min)
        assert len(set(flips)) == 2, flips
    ev = list(datasets.DeviceLoader(ds, T.Stereo_eval(), 5, shuffle=True, drop_last=True))
    assert len(ev) == 1 and ev[0][0].shape == (5, ds.channels) + tuple(ds.size_min)


def test_one_training_step_on_a_loader_batch(hip_lib, tmp_path):
    from dsmnet_amd import datasets, train
    from dsmnet_amd import transforms as T
    from dsmnet_amd.models import model_create_by_name
    DT.write_kitti(str(tmp_path), "kitti2015-tr", sizes=((70, 140), (66, 136)), seed=24)
    ds = datasets.dataset_stereo_by_name("kitti2015-tr", str(tmp_path), Train=True)
    np.random.seed(4)
    torch.manual_seed(0)
    loader = datasets.DeviceLoader(ds, T.Stereo_train(size_crop=[128, 64], scale_delt=0, shift_max=8), 2)
    (batch, names), = list(loader)
    assert batch.shape == (2, 7, 64, 128) and len(names) == 2
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lf = train.losses("supervised", model.count_levels, 37)
    lf.Weight_Adjust_levels(10)
    opt = train.make_optimizer(model, lr=1e-4)
    loss, d1, epe = train.train_step(model, opt, lf, batch)
    assert np.isfinite(loss) and np.isfinite(d1) and np.isfinite(epe)
