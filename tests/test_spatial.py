"""CPU: the spatial-augmentation planner (dsmnet_amd.transforms) and the numpy restatement
(tests/spatial_oracle.py) against the fixture written from the reference's own transform, the
rectangular-batch refusal, and the argument checks of the fused op (no kernel is launched).

Crop-only cases are the reference's own output and must match bit for bit.  Scale cases went
through ``resize_linear`` in place of cv2.resize (see the fixture's ``cv2`` note): bound
4 * 2^-23 * M per pixel, M = the largest of the pixel's four taps in output units."""
import ctypes

import numpy as np
import pytest
import torch

from tests import color_oracle as CO
from tests import spatial_oracle as SO
from tests.conftest import Golden

CASES = ["crop_a", "crop_b", "crop_c", "scale_a", "scale_b", "scale_c", "scale_big_c"]
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def gold():
    return Golden("spatial")


def _transform(meta, factory="Stereo_Spatial"):
    from dsmnet_amd import transforms as T
    return getattr(T, factory)(list(meta["size_crop"]), meta["scale_delt"], meta["shift_max"])


def _records(gold, case):
    return [tuple(r) for r in gold[case + ".records"].tolist()]


@pytest.mark.parametrize("case", CASES)
def test_planner_reproduces_the_reference_draws(gold, case):
    meta = gold.meta["cases"][case]
    x = gold["frames." + meta["frames"]]
    t = _transform(meta)
    np.random.seed(meta["seed"])
    records, hw, channels = t.plan_spatial(x.shape[0], x.shape[1], x.shape[2])
    assert float(np.random.rand()) == float(gold[case + ".next_rand"])
    assert [tuple(float(v) for v in r) for r in records] == _records(gold, case)
    assert tuple(hw) == tuple(gold[case + ".out"].shape[2:]) and channels == 6
    assert t.spatial.shift_max == meta["shift_max_after"]
    assert float(t.spatial.scale_rand) == meta["scale_rand_after"]
    assert all(isinstance(v, int) for r in records for v in r[:6])


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_reference(gold, case):
    meta = gold.meta["cases"][case]
    x, want = gold["frames." + meta["frames"]], gold[case + ".out"]
    records = _records(gold, case)
    records = [tuple(int(v) for v in r[:6]) + r[6:] for r in records]
    got = SO.restate_batch(x, records, want.shape[2:])
    assert got.dtype == np.float32
    if meta["scale_delt"] == 0:
        assert np.array_equal(got, want)
    else:
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= 4 * EPS * SO.tap_bound_batch(x, records, want.shape[2:])).all(), err.max()


def test_fixture_reaches_every_branch(gold):
    assert "NOT measured" in gold.meta["cv2"]
    crop = [r for c in CASES if c.startswith("crop") for r in _records(gold, c)]
    scale = [r for c in CASES if c.startswith("scale") for r in _records(gold, c)]
    assert any(r[0] == 0 for r in crop) and any(r[0] > 0 for r in crop)
    assert all(r[5] == 0 and r[6] == 1.0 for r in crop)
    assert any(r[6] > 1 for r in scale) and any(r[6] < 1 for r in scale)
    assert all(r[5] == 1 for r in scale)
    for c in ("a", "b"):                                       # disparities: zeros, negatives, ~200
        d = gold["frames." + c][..., 6:]
        assert (d == 0).any() and (d < 0).any() and d.max() > 190


@pytest.mark.parametrize("case", ["crop_a", "scale_a"])
def test_stereo_train_planner_and_restatements(gold, case):
    """Spatial restatement, then the colour restatement fed by the planner's Lighting draws on the
    CPU generator, against the reference's Stereo_train (the colour kernel's 1e-5 bound)."""
    meta = gold.meta["cases"][case]
    x, want = gold["frames." + meta["frames"]], torch.from_numpy(gold[case + ".train"]).double()
    t = _transform(meta, "Stereo_train")
    np.random.seed(meta["seed"])
    torch.manual_seed(meta["seed"])
    records, hw, channels = t.plan_spatial(x.shape[0], x.shape[1], x.shape[2])
    out = torch.from_numpy(SO.restate_batch(x, records, hw, channels)).double()
    launches = t.plan(x.shape[0], x.shape[3], "cpu")
    assert len(launches) == 1
    for recs, alpha, G in launches:
        assert all(r[2] == CO.LIGHTING | CO.NORMALIZE for r in recs)
        out = CO.restate(out, recs, alpha, G)
    assert (out - want).abs().max().item() <= 1e-5
    assert torch.equal(out[:, 6:], torch.from_numpy(gold[case + ".out"]).double()[:, 6:])


def test_resize_rule_by_hand():
    """2x1 -> 4x1: taps (0,0,f=0), (0,1,.25), (0,1,.75), (1,1,0); identity when sizes agree."""
    img = np.array([[10.0, 30.0]], dtype=np.float32).reshape(1, 2, 1)
    out = SO.resize_linear(img, (4, 1))
    assert out.reshape(-1).tolist() == [10.0, 15.0, 25.0, 30.0]
    big = np.random.RandomState(0).rand(5, 7, 3).astype(np.float32)
    assert np.array_equal(SO.resize_linear(big, (7, 5), 1), big)            # the stray third argument
    col = SO.resize_linear(big[:, :1], (3, 5))                               # 1-pixel-wide source
    assert np.array_equal(col, np.repeat(big[:, :1], 3, axis=1))


def test_planner_draw_order_and_skipped_draws():
    from dsmnet_amd import transforms as T
    np.random.seed(5)
    rec = T.Spatial_stereo([16, 12], 0, 5).draw(12, 20)         # h0 == h: no hs draw
    after = np.random.rand()
    np.random.seed(5)
    shift = np.random.randint(0, 5)
    ws = np.random.randint(0, 20 - shift - 16) if 20 - shift > 16 else 0
    assert rec == (shift, ws, 0, 16, 12, 0, 1.0, 1.0, 1.0) and after == np.random.rand()
    np.random.seed(6)
    s = T.Spatial_stereo([16, 12], 0.5, 0)                      # shift_max <= 0: no shift draw
    rec = s.draw(30, 40)
    after = np.random.rand()
    np.random.seed(6)
    sc = 1 + np.random.uniform(0, 0.5)
    sc = 1.0 / sc if np.random.rand() > 0.5 else sc
    w, h = int(16 / sc + 0.5), int(12 / sc + 0.5)
    ws, hs = np.random.randint(0, 40 - w), np.random.randint(0, 30 - h)
    assert rec == (0, ws, hs, w, h, 1, sc, 1.0 / (16.0 / w), 1.0 / (12.0 / h))
    assert after == np.random.rand() and s.scale_rand == sc and s.shift_max == 0
    s = T.Spatial_stereo([16, 12], 0, 50)                       # shift_max clamps to the width, for good
    s.draw(12, 20)
    assert s.shift_max == 20
    t = T.Stereo_ToTensor()
    np.random.seed(7)
    assert t.plan_spatial(2, 9, 13) == ([(0, 0, 0, 13, 9, 0, 1.0, 1.0, 1.0)] * 2, (9, 13), 6)
    np.random.seed(7)
    first = np.random.rand()
    np.random.seed(7)
    t.plan_spatial(2, 9, 13)
    assert np.random.rand() == first                            # draws nothing


def test_factories_and_launch_grouping():
    from dsmnet_amd import transforms as T
    t = T.Stereo_train([384, 192], 0, 8)
    assert isinstance(t.spatial, T.Spatial_stereo) and t.to_tensor.channel == 6 and len(t.launches) == 1
    assert [type(s) for s in t.launches[0]] == [T.Lighting, T.Normalize_Imagenet]
    assert (t.spatial.size_crop, t.spatial.scale_delt, t.spatial.shift_max) == ([384, 192], 0, 8)
    e = T.Stereo_eval()
    assert e.spatial is None and e.to_tensor is not None and len(e.launches) == 1
    s = T.Stereo_Spatial()
    assert (s.spatial.size_crop, s.spatial.scale_delt, s.spatial.shift_max) == ([768, 384], 0.4, 32)
    assert s.launches == []
    d = T.Spatial_stereo()
    assert (d.size_crop, d.scale_delt, d.shift_max) == ([768, 384], 0.5, 32)
    c = T.Stereo_color()
    assert c.spatial is None and c.to_tensor is None and len(c.launches) == 1     # colour-only: unchanged
    with pytest.raises(TypeError):
        T.Compose([T.Normalize_Imagenet(), T.ToTensor_numpy()])
    with pytest.raises(TypeError):
        T.Compose([T.ToTensor_numpy(), T.Spatial_stereo()])
    with pytest.raises(ValueError):
        T.ToTensor_numpy(channel=4)


def test_rectangular_batch_refusal():
    from dsmnet_amd import transforms as T
    t = T.Stereo_Spatial([16, 12], 0, 5)
    assert t.plan_spatial(2, 23, 20)[1] == (12, 16)             # 20 - 4 >= 16
    np.random.seed(0)
    with pytest.raises(ValueError, match="width"):
        T.Stereo_Spatial([16, 12], 0, 5).plan_spatial(2, 23, 19)      # 19 - 4 < 16
    assert np.random.rand() == np.random.RandomState(0).rand()        # refused before any draw
    assert T.Stereo_Spatial([16, 12], 0, 5).plan_spatial(1, 8, 20)[1] == (8, 16)   # short frames: h = h0
    assert T.Stereo_Spatial([16, 12], 0.5, 5).plan_spatial(2, 23, 19)[1] == (12, 16)   # scaling always fills the crop


def test_ops_refuse_cpu_tensors():
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import transforms as T
    x = torch.rand(2, 9, 13, 7)
    recs = [(0, 0, 0, 13, 9, 0, 1.0, 1.0, 1.0)] * 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.stereo_spatial(x, recs, (9, 13))
    for t in (T.Stereo_Spatial([8, 6], 0, 3), T.Stereo_train([8, 6], 0, 3), T.Stereo_ToTensor(), T.Stereo_eval(),
              T.Spatial_stereo([8, 6], 0, 3), T.ToTensor_numpy()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(x[0])


def test_dsm_stereo_spatial_rejects_bad_arguments(hip_lib):
    from dsmnet_amd import _lib
    assert ctypes.sizeof(_lib.SpatialRecord) == 48
    assert ctypes.sizeof(_lib.SpatialRecord) * _lib.DSM_SPATIAL_MAX_RECORDS <= \
        ctypes.sizeof(_lib.ColorRecord) * _lib.DSM_COLOR_MAX_RECORDS
    one = ctypes.c_void_p(16)

    def recs(n, shift=1, ws=2, hs=1, w=8, h=6, resize=0, scale_rand=1.0, sx=1.0, sy=1.0):
        a = (_lib.SpatialRecord * n)()
        for r in a:
            r.shift, r.ws, r.hs, r.w, r.h, r.resize = shift, ws, hs, w, h, resize
            r.scale_rand, r.scale_x, r.scale_y = scale_rand, sx, sy
        return a

    call = hip_lib.dsm_stereo_spatial
    # frames 9 x 13 x 7, output 6 x 8: the window [2, 10) fits 13 - 1 columns
    assert call(None, one, recs(2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1            # null x
    assert call(one, None, recs(2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1            # null y
    assert call(one, one, None, 2, 2, 7, 9, 13, 6, 8, 6, None) == -1                # null records
    assert call(one, one, recs(2), 2, 2, 5, 9, 13, 6, 8, 6, None) == -1             # C < 6
    assert call(one, one, recs(2), 2, 2, 9, 9, 13, 6, 8, 6, None) == -1             # C > 8
    assert call(one, one, recs(2), 1, 2, 7, 9, 13, 6, 8, 6, None) == -1             # records != B
    assert call(one, one, recs(2), 2, 2, 7, 9, 13, 6, 8, 3, None) == -1             # to_tensor not 0 or 6
    assert call(one, one, recs(2), 2, 2, 7, 0, 13, 6, 8, 6, None) == -1             # H0 < 1
    assert call(one, one, recs(2), 2, 2, 7, 9, 13, 6, 0, 6, None) == -1             # w < 1
    assert call(one, one, recs(2, shift=-1), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1   # shift < 0
    assert call(one, one, recs(2, shift=13, ws=0, w=1, h=1), 2, 2, 7, 9, 13, 1, 1, 6, None) == -1   # shift == W0
    assert call(one, one, recs(2, ws=5), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1       # 5 + 8 > 13 - 1
    assert call(one, one, recs(2, shift=4, ws=2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1   # 2 + 8 > 13 - 4
    assert call(one, one, recs(2, hs=4), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1       # 4 + 6 > 9
    assert call(one, one, recs(2, ws=-1), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, hs=-1), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, w=0), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, w=7), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1        # flag off, window != output
    assert call(one, one, recs(2, h=5), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, resize=2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1   # unknown flag
    assert call(one, one, recs(2, resize=1, sx=0.0), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, resize=1, sy=float("nan")), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    assert call(one, one, recs(2, resize=1, scale_rand=float("inf")), 2, 2, 7, 9, 13, 6, 8, 6, None) == -1
    # one image of 2^31 elements or more, input or output
    assert call(one, one, recs(1), 1, 1, 8, 16384, 16384, 6, 8, 6, None) == -2
    big = recs(1, shift=0, ws=0, hs=0, w=2, h=2, resize=1, sx=1e-4, sy=1e-4)
    assert call(one, one, big, 1, 1, 8, 9, 13, 16384, 16384, 6, None) == -2
    # misaligned bases
    assert call(ctypes.c_void_p(18), one, recs(2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -4
    assert call(one, ctypes.c_void_p(17), recs(2), 2, 2, 7, 9, 13, 6, 8, 6, None) == -4
