"""CPU: the float64 restatement of utils/evaluate.py (tests/metrics_oracle.py) against the fixture made
from the reference's own lines, ``stereo_metrics_finish``, and the host side of dsm_stereo_metrics."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from dsmnet_amd import _lib, costvolume as cv, train
from tests import metrics_oracle as MO
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "golden_metrics.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(z["meta"]).decode())
    d["keys"] = json.loads(bytes(z["keys"]).decode())
    return d


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def test_restatement_against_the_fixture(fx):
    B, C, H, W = fx["meta"]["shape"]
    imgs, gt, pred = (torch.from_numpy(fx[k]) for k in ("imgs", "gt", "pred"))
    assert MO.precondition_holds(pred, gt)
    imL, imR = MO.images_of(imgs)
    sums = MO.sums(pred, gt, imL, imR, float(fx["delt"]), negate_warp=fx["meta"]["negate_warp"])
    want = torch.from_numpy(fx["sums"])
    assert sums.shape == (B, 16)
    assert torch.equal(sums[:, list(MO.COUNT_SLOTS)], want[:, list(MO.COUNT_SLOTS)])
    assert ((sums - want).abs() <= 1e-12 * want.abs()).all()
    got = MO.finish(sums, (C, H, W))
    for k, v in zip(fx["keys"], fx["reference"]):
        assert rel(got[k], v) <= 1e-6, (k, float(got[k]), v)
    assert rel(got["pixelerror"], fx["pixelerror"]) <= 1e-12
    # the inputs do what they are for: holes, bad and good pixels, every a-threshold separating some
    n = float(want[:, 0].sum())
    assert 0.5 * B * H * W < n < 0.9 * B * H * W
    assert 0 < float(want[:, 8].sum()) < float(want[:, 9].sum()) < float(want[:, 10].sum()) < n
    assert 0 < float(want[:, 2].sum()) < n and float(want[:, 2].sum()) + float(want[:, 3].sum()) == n
    assert 0 < float(want[:, 13].sum()) < B * H * W and float(want[:, 15].sum()) / (B * C * H * W) >= 0.1


def test_finish_on_the_fixture_sums(fx):
    B, C, H, W = fx["meta"]["shape"]
    sums = torch.from_numpy(fx["sums"])
    whole = cv.stereo_metrics_finish(sums, image_shape=(C, H, W))
    assert sorted(whole) == sorted(cv.METRIC_KEYS) == sorted(MO.KEYS)
    for k, v in zip(fx["keys"], fx["reference"]):
        assert whole[k].dtype == torch.float64 and whole[k].dim() == 0
        assert rel(whole[k], v) <= 1e-6, k
    assert rel(whole["pixelerror"], fx["pixelerror"]) <= 1e-12
    per = cv.stereo_metrics_finish(sums, per_image=True, image_shape=(C, H, W))
    for b in range(B):
        one = MO.finish(sums[b:b + 1], (C, H, W))
        for k in cv.METRIC_KEYS:
            assert per[k].shape == (B,) and rel(per[k][b], one[k]) <= 1e-12, (k, b)
    # the rows are additive: the whole batch is the finish of the summed rows
    summed = cv.stereo_metrics_finish(sums.sum(0, keepdim=True), image_shape=(C, H * B, W))
    for k in cv.METRIC_KEYS:
        assert rel(summed[k], whole[k]) <= 1e-12, k
    # the shape noted by stereo_metrics on its result is the default
    sums.image_shape = (C, H, W)
    assert rel(cv.stereo_metrics_finish(sums)["pixelerror"], fx["pixelerror"]) <= 1e-12
    with pytest.raises(ValueError):
        cv.stereo_metrics_finish(torch.zeros(2, 15, dtype=torch.float64))


def test_finish_without_valid_pixels_and_without_inside_pixels():
    C, H, W = 3, 4, 5
    s = torch.zeros(2, 16, dtype=torch.float64)
    s[0, :11] = torch.tensor([10, 20, 7, 3, 90, 1.5, 2.5, 6, 2, 5, 9], dtype=torch.float64)
    s[0, 11:] = torch.tensor([30, 6, 12, 9, 12], dtype=torch.float64)
    s[1, 15] = 6.0                                           # image 1: no gt pixel, nothing warped from inside
    per = cv.stereo_metrics_finish(s, per_image=True, image_shape=(C, H, W))
    gt_keys = [k for k in cv.METRIC_KEYS if not k.startswith("pixelerror")]
    for k in gt_keys:
        assert math.isnan(float(per[k][1])) and math.isfinite(float(per[k][0])), k
    assert float(per["d1"][0]) == 30.0 and float(per["d1_kitti"][0]) == 30.0 and float(per["epe"][0]) == 2.0
    assert float(per["rmse"][0]) == 3.0 and float(per["a1"][0]) == 0.2 and float(per["abs_rel"][0]) == 0.25
    assert rel(per["pixelerror"][0], 255.0 * 9 / (C * 12)) <= 1e-14
    assert rel(per["pixelerror"][1], 255.0 * 6 / (C * H * W)) <= 1e-14        # the fallback: every element
    assert rel(per["pixelerror_elem"][0], 255.0 * 6 / 30) <= 1e-14 and math.isnan(float(per["pixelerror_elem"][1]))
    whole = cv.stereo_metrics_finish(s, image_shape=(C, H, W))
    assert float(whole["epe"]) == 2.0 and rel(whole["pixelerror"], 255.0 * 9 / (C * 12)) <= 1e-14
    none = cv.stereo_metrics_finish(s[1:], image_shape=(C, H, W))
    assert math.isnan(float(none["d1"])) and rel(none["pixelerror"], 255.0 * 6 / (C * H * W)) <= 1e-14
    assert math.isnan(float(cv.stereo_metrics_finish(s)["pixelerror"]))    # no image shape known


def _args(**kw):
    a = _lib.MetricsArgs()
    a.pred = a.gt = a.imL = a.imR = a.workspace = a.out = 64
    a.B, a.C, a.H, a.W, a.delt, a.flags = 1, 3, 8, 8, 1e-5, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_refusals(hip_lib):
    """Every refusal happens before a launch: the pointers are fake."""
    call = lambda **kw: hip_lib.dsm_stereo_metrics(ctypes.byref(_args(**kw)), None)
    assert ctypes.sizeof(_lib.MetricsArgs) == 72
    assert hip_lib.dsm_stereo_metrics(None, None) == -1
    for name in ("pred", "out", "workspace"):
        assert call(**{name: None}) == -1, name
    assert call(imL=None) == -1 and call(imR=None) == -1               # one image without the other
    assert call(gt=None, imL=None, imR=None) == -1                      # nothing to measure
    for name in ("B", "C", "H", "W"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(H=1) == -1 and call(W=1) == -1                          # imwrap.py:48
    for flags in (2, 3, -1, 256):
        assert call(flags=flags) == -1, flags
    for name in ("pred", "gt", "imL", "imR"):
        assert call(**{name: 66}) == -4, name                           # not 4-byte aligned
    assert call(workspace=68) == -4 and call(out=68) == -4              # float64: 8 bytes
    assert call(B=1 << 20, H=4096, W=4096) == -2                        # 2^34 tiles: past the grid's x extent
    assert call(B=0, H=1 << 20) == -1                                   # the argument checks come first


def test_workspace_size(hip_lib):
    f = hip_lib.dsm_stereo_metrics_workspace_bytes
    assert f(1, 5, 7) == 16 * 8
    assert f(2, 37, 300) == 2 * 3 * 5 * 16 * 8
    assert f(4, 540, 960) == 4 * 34 * 15 * 16 * 8
    assert f(1, 16, 64) == 16 * 8 and f(1, 17, 65) == 4 * 16 * 8
    assert f(0, 4, 4) == 0 and f(1, 0, 4) == 0 and f(1, 4, -1) == 0


def test_cpu_tensors_are_refused():
    from dsmnet_amd import evaluate as ev
    p, im = torch.ones(1, 1, 4, 6), torch.ones(1, 3, 4, 6)
    for fn in (lambda: cv.stereo_metrics(p, p), lambda: cv.stereo_metrics(p, None, im, im, delt=1e-5),
               lambda: cv.stereo_metrics(p[:, 0], p)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev.compute_errors(p.numpy(), p.numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.evaluate(im, im, p, p, device="cpu")


def test_evaluate_step_leaves_the_validation_steps_alone():
    assert list(inspect.signature(train.evaluate_step).parameters) == ["model", "batch", "augment", "per_image"]
    assert list(inspect.signature(train.validate_step).parameters) == ["model", "lossfun", "batch"]
    assert list(inspect.signature(train.validate_step_selfsup).parameters) == ["model", "lossfun", "batch", "augment"]
    assert list(inspect.signature(train.accuracy).parameters) == ["dispL", "dispL_gt"]
    src = inspect.getsource(train.evaluate_step)
    assert "validate_step" not in src.split('"""')[2] and "accuracy(" not in src
    for fn in (train.validate_step, train.validate_step_selfsup, train.accuracy, train._selfsup_accuracy):
        assert "stereo_metrics" not in inspect.getsource(fn), fn.__name__
    # accuracy is still the stock restatement, and agrees with the new finish on what both give
    g = torch.Generator().manual_seed(3)
    gt = 40 * torch.rand(2, 1, 9, 11, generator=g) * (torch.rand(2, 1, 9, 11, generator=g) > 0.3)
    pred = gt + 8 * torch.rand(2, 1, 9, 11, generator=g) - 4
    d1, epe = train.accuracy(pred, gt)
    f = MO.finish(MO.sums(pred, gt))
    assert rel(d1, f["d1"]) <= 1e-5 and rel(epe, f["epe"]) <= 1e-5
