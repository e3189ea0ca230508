"""GPU: the fused evaluation metrics (csrc/metrics.hip, costvolume.stereo_metrics) against the float64
restatement of utils/evaluate.py (tests/metrics_oracle.py).

Counts (slots 0, 2, 3, 8-11, 13) must be EXACTLY equal: every input is kept at least 1e-3 away from
every counted threshold (metrics_oracle.condition; asserted again here), far beyond what fp32 rounding
moves.  Every other slot and every finished metric is held to 1e-5 relative, the project's bound for
fp32 fused ops with fp64 sums (tests/test_suploss_gpu.py).  Two runs must agree bit for bit.

Shapes are the smallest that reach each branch: below one block (5x7), the vector path with ragged
tiles in both axes (37x300: 3 x 5 tiles of 16x64), the scalar path (19x301, and 37x300 from a base
that is not 16-byte aligned), C = 1, (B,H,W) predictions, every disparity beyond W (slot 13 = 0, the
fallback), no gt, no images, both warp signs, a replayed graph, evaluate_step on a small model."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics_oracle as MO
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-5
DELT = 6.25e-05
COUNTS = list(MO.COUNT_SLOTS)


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@functools.lru_cache(maxsize=None)
def case(name):
    """(pred, gt, imL, imR) on the CPU, float32; computed once and never modified."""
    if name == "tiny":
        imgs, gt, pred = MO.make_inputs(11, 1, 3, 5, 7, dlo=0.5, dhi=4.0)
    elif name == "vector":
        imgs, gt, pred = MO.make_inputs(12, 2, 3, 37, 300)
        gt[1] = 0                                            # image 1: all holes
    elif name == "scalar":
        imgs, gt, pred = MO.make_inputs(13, 1, 3, 19, 301)
    elif name == "gray":
        imgs, gt, pred = MO.make_inputs(14, 2, 1, 18, 68, dhi=30.0)
    elif name == "beyond":
        imgs, gt, pred = MO.make_inputs(15, 1, 3, 17, 40, dlo=90.0, dhi=120.0)     # 0.5 * 90 - 0.2 > W
    else:
        raise KeyError(name)
    assert MO.precondition_holds(pred, gt) and float(pred.min()) > 0
    imL, imR = MO.images_of(imgs)
    return pred, gt, imL, imR


@functools.lru_cache(maxsize=None)
def oracle(name, use_gt=True, use_im=True, negate=False):
    pred, gt, imL, imR = case(name)
    return MO.sums(pred, gt if use_gt else None, imL if use_im else None, imR if use_im else None, DELT, negate)


def dev(t):
    return None if t is None else t.cuda()


def run(cv, name, use_gt=True, use_im=True, negate=False, prep=dev):
    pred, gt, imL, imR = case(name)
    out = cv.stereo_metrics(prep(pred), prep(gt) if use_gt else None, prep(imL) if use_im else None,
                            prep(imR) if use_im else None, delt=DELT, negate_warp=negate)
    torch.cuda.synchronize()
    return out


def close(got, want, what):
    got, want = got.double().cpu().reshape(-1), want.double().cpu().reshape(-1)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN pattern %s vs %s" % (what, got, want)
    err = ((got - want).abs() / want.abs().clamp(min=1e-30))[~nan]
    zero = (want == 0) & ~nan
    assert bool((got[zero] == 0).all()), "%s: nonzero where the oracle has 0: %s" % (what, got)
    worst = float(err[~zero[~nan]].max()) if bool((~zero[~nan]).any()) else 0.0
    print("%s: max rel err %.3e" % (what, worst))
    assert worst <= RTOL, "%s: rel err %.3e > %.0e\n%s\n%s" % (what, worst, RTOL, got, want)


def check(cv, got, want, image_shape, what):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape) and got.is_cuda
    g = got.cpu()
    assert torch.equal(g[:, COUNTS], want[:, COUNTS]), "%s: counts\n%s\n%s" % (what, g[:, COUNTS], want[:, COUNTS])
    close(g, want, what + " sums")
    for per in (False, True):
        mine = cv.stereo_metrics_finish(got, per_image=per, image_shape=image_shape)
        ref = MO.finish(want, image_shape, per_image=per)
        for k in MO.KEYS:
            assert mine[k].is_cuda and mine[k].dtype == torch.float64
            close(mine[k], ref[k], "%s %s%s" % (what, k, " per image" if per else ""))


def shape_of(name):
    return tuple(case(name)[2].shape[1:])


@pytest.mark.parametrize("name", ["tiny", "vector", "scalar", "gray"])
def test_against_the_oracle(cv, name):
    got = run(cv, name)
    check(cv, got, oracle(name), shape_of(name), name)
    assert torch.equal(got, run(cv, name)), "two runs differ"
    assert got.image_shape == shape_of(name)


def test_all_holes_image_is_nan_alone(cv):
    got = run(cv, "vector")
    per = cv.stereo_metrics_finish(got, per_image=True)
    whole = cv.stereo_metrics_finish(got)
    assert float(got[1, 0]) == 0 and float(got[0, 0]) > 0
    for k in ("d1", "epe", "abs_rel", "rmse_log", "a3", "d1_kitti"):
        assert math.isnan(float(per[k][1])) and math.isfinite(float(per[k][0])) and math.isfinite(float(whole[k])), k
        assert float(whole[k]) == float(per[k][0])           # image 1 adds nothing
    assert math.isfinite(float(per["pixelerror"][1])) and math.isfinite(float(per["pixelerror_elem"][1]))


def test_base_not_16_byte_aligned(cv):
    def shifted(t):
        buf = torch.empty(t.numel() + 4, device="cuda", dtype=torch.float32)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    got = run(cv, "vector", prep=shifted)
    check(cv, got, oracle("vector"), shape_of("vector"), "vector, shifted base")
    # the width of a load changes no arithmetic and no order
    assert torch.equal(got, run(cv, "vector"))


def test_three_dimensional_predictions(cv):
    pred, gt, imL, imR = case("scalar")
    got = cv.stereo_metrics(pred[:, 0].cuda(), gt.cuda(), imL.cuda(), imR.cuda(), delt=DELT)
    assert torch.equal(got, run(cv, "scalar"))
    with pytest.raises(ValueError):
        cv.stereo_metrics(pred.cuda(), gt[:, :, :-1].cuda())
    with pytest.raises(ValueError):
        cv.stereo_metrics(pred.cuda(), None, imL.cuda(), None)
    with pytest.raises(ValueError):
        cv.stereo_metrics(pred.cuda())


def test_every_disparity_beyond_the_image(cv):
    got = run(cv, "beyond")
    want = oracle("beyond")
    assert float(want[0, 13]) == 0 and float(want[0, 11]) == 0 and float(want[0, 15]) > 0
    check(cv, got, want, shape_of("beyond"), "beyond")
    C, H, W = shape_of("beyond")
    f = cv.stereo_metrics_finish(got)
    assert abs(float(f["pixelerror"]) - 255.0 * float(want[0, 15]) / (C * H * W)) <= RTOL * float(f["pixelerror"])
    assert math.isnan(float(f["pixelerror_elem"]))


def test_without_gt_and_without_images(cv):
    no_gt = run(cv, "vector", use_gt=False)
    check(cv, no_gt, oracle("vector", use_gt=False), shape_of("vector"), "no gt")
    assert float(no_gt[:, :11].abs().sum()) == 0
    no_im = run(cv, "vector", use_im=False)
    check(cv, no_im, oracle("vector", use_im=False), None, "no images")
    assert float(no_im[:, 11:].abs().sum()) == 0 and no_im.image_shape is None
    both = run(cv, "vector")
    assert torch.equal(both[:, :11], no_im[:, :11]) and torch.equal(both[:, 11:], no_gt[:, 11:])


def test_warp_sign(cv):
    plus, minus = run(cv, "vector"), run(cv, "vector", negate=True)
    check(cv, minus, oracle("vector", negate=True), shape_of("vector"), "negated warp")
    assert torch.equal(plus[:, :11], minus[:, :11])
    assert not torch.equal(plus[:, 11:], minus[:, 11:]) and float(plus[0, 13]) != float(minus[0, 13])


def test_timed_as_one_op(cv):
    timer = cv.LaunchTimer()
    cv.set_timer(timer)
    try:
        run(cv, "tiny")
    finally:
        cv.set_timer(None)
    assert list(timer.summary()) == ["metrics_tiles+reduce"]


def test_replayed_graph_follows_its_inputs(cv):
    a, b = case("scalar"), None
    imgs, gt2, pred2 = MO.make_inputs(23, 1, 3, 19, 301)
    b = (pred2, gt2) + MO.images_of(imgs)
    static = [t.cuda() for t in a]
    step = lambda: cv.stereo_metrics(static[0], static[1], static[2], static[3], delt=DELT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
        fin = cv.stereo_metrics_finish(out)
    for inputs in (b, a):
        for s, t in zip(static, inputs):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = cv.stereo_metrics(*[t.cuda() for t in inputs], delt=DELT)
        assert torch.equal(out, eager)
        assert torch.equal(fin["rmse"], cv.stereo_metrics_finish(eager)["rmse"])
    check(cv, out, oracle("scalar"), shape_of("scalar"), "replayed graph")


def test_evaluate_step_on_a_small_model(cv):
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    model = model_create_by_name("dispnetcorr", 192).cuda().eval()
    imgs, gt, _ = MO.make_inputs(31, 2, 3, 64, 128)
    imL, imR = MO.images_of(imgs)
    pair = torch.cat([imL, imR], 1).cuda()
    with torch.no_grad(), cv.amax_scope(pair.device):
        pred = model(pair[:, :3], pair[:, 3:6])[1][0].float().cpu()
    if pred.dim() == 3:
        pred = pred.unsqueeze(1)
    assert tuple(pred.shape) == (2, 1, 64, 128)
    # ground truth around the model's OWN output: holes where it is not clearly positive, moved onto the
    # prediction where a threshold would be too close (here the prediction is given, gt is ours to place)
    g = torch.Generator().manual_seed(32)
    factor = 0.5 + 1.9 * torch.rand(pred.shape, generator=g)
    gt = torch.where((pred > 0.05) & (gt > 0), pred * factor, torch.zeros(()))
    near_gt, near_warp = MO.offenders(pred, gt, warp_signs=(1.0,))
    gt[near_gt] = pred[near_gt]
    assert MO.precondition_holds(pred, gt, warp_signs=(1.0,)), "%d pixels at the warp's edge" % int(near_warp.sum())
    batch = torch.cat([pair, gt.cuda()], 1)
    torch.manual_seed(5)
    delt = MO.SO.draw_delt()
    want = MO.sums(pred, gt, imL, imR, delt, negate_warp=False)
    for per in (False, True):
        torch.manual_seed(5)                                 # evaluate_step draws the same epsilon
        got = train.evaluate_step(model, batch, per_image=per)
        ref = MO.finish(want, (3, 64, 128), per_image=per)
        assert sorted(got) == sorted(MO.KEYS)
        for k in MO.KEYS:
            close(got[k], ref[k], "evaluate_step %s" % k)
    assert not model.training
    torch.manual_seed(5)
    no_gt = train.evaluate_step(model, batch[:, :6])
    assert math.isnan(float(no_gt["epe"]))
    close(no_gt["pixelerror"], MO.finish(want, (3, 64, 128))["pixelerror"], "evaluate_step without gt")


def test_reference_names_against_the_fixture(cv):
    from dsmnet_amd import evaluate as ev
    z = np.load(os.path.join(GOLDEN, "golden_metrics.npz"), allow_pickle=False)
    want = dict(zip(json.loads(bytes(z["keys"]).decode()), z["reference"]))
    imgs, gt, pred = torch.from_numpy(z["imgs"]), z["gt"], z["pred"]
    assert MO.precondition_holds(torch.from_numpy(pred), torch.from_numpy(gt))
    imL, imR = MO.images_of(imgs)
    delt = float(z["delt"])
    ok = lambda a, b: abs(a - b) <= RTOL * abs(b)
    d1, epe, pixelerror = ev.evaluate(imL.numpy(), imR.numpy(), pred, gt, delt=delt)
    assert all(isinstance(v, float) for v in (d1, epe, pixelerror))
    assert ok(d1, want["d1"]) and ok(epe, want["epe"]) and ok(pixelerror, float(z["pixelerror"]))
    assert ev.evaluate(imL, imR, torch.from_numpy(pred), delt=delt)[:2] == (-1, -1)
    assert ok(ev.imwrap_pixel_errors(imL, imR, torch.from_numpy(pred), delt=delt), want["pixelerror_elem"])
    got = ev.compute_errors(gt, torch.from_numpy(pred).cuda())
    names = ("abs_rel", "sq_rel", "rmse", "rmse_log", "d1_kitti", "a1", "a2", "a3")
    assert len(got) == 8
    for k, v in zip(names, got):
        assert ok(v, want[k]), (k, v, want[k])
    # the default epsilon is drawn as the reference draws it: 1e-4 * (U[0,1) + 0.1), too small to matter here
    assert abs(ev.imwrap_pixel_errors(imL, imR, pred) - want["pixelerror_elem"]) <= 0.05
