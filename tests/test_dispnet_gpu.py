"""GPU: the DispNet model against tests/golden/golden_dispnet.npz (the reference's outputs), and DispNet /
DispNetC with the ``conv2d_k5`` option on against off: the 5x5 stride-2 layers on the MFMA kernel
(dsmnet_amd/csrc/conv_wide2d.hpp with K = 5), graph capture of the NHWC chain, training and deploy."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests import dispnet_cases as DC
from tests.helpers import maxerr, seeded

pytestmark = pytest.mark.gpu

DISP_TOL = 1e-3           # pixels: the north-star bound of tests/test_models_gpu.py


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@pytest.fixture(scope="module")
def fixture():
    return DC.Fixture()


@pytest.fixture(scope="module")
def dispnet_gpu():
    return DC.build_model().cuda()


@contextmanager
def options(cv, **kw):
    old = {k: cv.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            cv.set_option(k, v)


def forward(cv, m, imL, imR, k5, wide=False, timer=None, mode="train"):
    with options(cv, conv_precision="f16x2", wide_conv2d=wide, conv2d_k5=k5), torch.no_grad():
        cv.set_timer(timer)
        try:
            return m(imL, imR, mode=mode)[1]
        finally:
            cv.set_timer(None)


def launches(timer, prefix):
    return sum(v["launches"] for k, v in timer.summary().items() if k.startswith(prefix))


@pytest.mark.parametrize("tag,seed,h,w", DC.CASES)
def test_dispnet_matches_the_reference_and_itself_with_the_k5_kernel(cv, fixture, dispnet_gpu, tag, seed, h, w):
    imL, imR = (t.cuda() for t in DC.images(seed, h, w))
    off_timer, on_timer = cv.LaunchTimer(), cv.LaunchTimer()
    off = forward(cv, dispnet_gpu, imL, imR, False, timer=off_timer)
    on = forward(cv, dispnet_gpu, imL, imR, True, timer=on_timer)
    test = forward(cv, dispnet_gpu, imL, imR, False, mode="test")
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(zip(off, fixture.outputs(tag, "train"))):
        assert got.shape == want.shape and maxerr(got, want) <= DISP_TOL, (tag, i, maxerr(got, want))
    for i, (got, want) in enumerate(zip(test, fixture.outputs(tag, "test"))):
        assert got.shape == want.shape and maxerr(got, want) <= DISP_TOL, (tag, "test", i, maxerr(got, want))
    assert len(on) == len(off) == 7
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and maxerr(a, b) <= DISP_TOL, (tag, i, maxerr(a, b))
    assert launches(on_timer, "conv2d_k5_") == 2 and launches(off_timer, "conv2d_k5_") == 0     # conv2, conv3a
    assert launches(on_timer, "conv2d_wide_") == launches(off_timer, "conv2d_wide_") == 0


@pytest.mark.parametrize("tag,seed,h,w", DC.CASES)
def test_dispnetcorr_runs_its_two_conv2_calls_on_the_k5_kernel(cv, tag, seed, h, w):
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(11)
    m = model_create_by_name("dispnetcorr", 192).cuda().eval()
    imL, imR = (t.cuda() for t in DC.images(seed, h, w))
    timers = {(k5, wide): cv.LaunchTimer() for k5 in (False, True) for wide in (False, True)}
    outs = {key: forward(cv, m, imL, imR, key[0], wide=key[1], timer=t) for key, t in timers.items()}
    torch.cuda.synchronize()
    for wide in (False, True):
        for i, (a, b) in enumerate(zip(outs[(True, wide)], outs[(False, wide)])):
            assert a.shape == b.shape and maxerr(a, b) <= DISP_TOL, (tag, wide, i, maxerr(a, b))
        # conv2 of the left and of the right image; conv3a (105 inputs) stays on the stock layer
        assert launches(timers[(True, wide)], "conv2d_k5_") == 2 and launches(timers[(False, wide)], "conv2d_k5_") == 0
        assert launches(timers[(True, wide)], "conv2d_wide_") == launches(timers[(False, wide)], "conv2d_wide_") == (7 if wide else 0)


def test_dispnet_captures_into_a_graph_and_replays_the_chain_bit_for_bit(cv, dispnet_gpu):
    from dsmnet_amd.graphs import GraphedForward
    m = dispnet_gpu
    imL, imR = (t.cuda() for t in DC.images(*DC.CASES[0][1:]))
    seen = {}
    handle = m.conv6b.register_forward_hook(lambda mod, inp, out: seen.__setitem__("y", out))
    timer = cv.LaunchTimer()
    try:
        eager = forward(cv, m, imL, imR, True, wide=True, timer=timer)
        chain_eager = seen["y"].clone()
        with options(cv, conv_precision="f16x2", wide_conv2d=True, conv2d_k5=True):
            g = GraphedForward(m, imL, imR, warmup=1)
            static = seen["y"]                   # the captured forward's conv6b output: rewritten by every replay
            static.zero_()
            outs = g(imL, imR)[1]
        torch.cuda.synchronize()
    finally:
        handle.remove()
    assert launches(timer, "conv2d_k5_") == 2 and launches(timer, "conv2d_wide_") == 7      # conv2 .. conv6b: one chain
    assert chain_eager.is_contiguous(memory_format=torch.channels_last)
    assert len(outs) == len(eager)
    assert torch.equal(static, chain_eager)      # (the final disparities pass through stock layers: not asserted)


def test_training_and_autograd_take_the_stock_layers(cv):
    m = DC.build_model().cuda()
    imL, imR = (t.cuda() for t in DC.images(*DC.CASES[0][1:]))
    timer = cv.LaunchTimer()
    with options(cv, conv_precision="f16x2", conv2d_k5=True):
        cv.set_timer(timer)
        try:
            with torch.enable_grad():            # eval mode, autograd on
                outs = m(imL, imR)[1]
                sum(o.sum() for o in outs).backward()
            assert m.conv2[0].weight.grad is not None and m.conv2[0].weight.grad.abs().sum().item() > 0
            m.zero_grad()
            m.train()
            with torch.no_grad():                # train mode, autograd off
                m(imL, imR)
        finally:
            cv.set_timer(None)
    torch.cuda.synchronize()
    assert not [k for k in timer.summary() if k.startswith("conv2d_k5_")]


def test_one_supervised_train_step(cv):
    from dsmnet_amd import train
    g = torch.Generator().manual_seed(3)
    left = torch.rand(1, 3, 64, 128, generator=g)
    disp = torch.full((1, 1, 64, 128), 6.0)
    disp[:, :, :, :6] = 0
    batch = torch.cat([left, torch.roll(left, -6, dims=3), disp], 1).cuda()
    model = DC.build_model().cuda()
    lf = train.losses("supervised", 7)
    opt = train.make_optimizer(model, lr=1e-4)
    before = model.conv2[0].weight.detach().clone()
    with options(cv, conv2d_k5=True):            # training keeps the stock layers whatever the option says
        out = train.train_step(model, opt, lf, batch)
    loss = out[0] if isinstance(out, (tuple, list)) else out
    assert np.isfinite(float(loss))
    assert not torch.equal(model.conv2[0].weight.detach(), before)


def test_deploy_loads_a_dispnet_state_dict_and_predicts(cv, tmp_path):
    from dsmnet_amd import deploy
    from dsmnet_amd.models import model_create_by_name
    path = str(tmp_path / "weight_best.pkl")
    torch.save({"state_dict": DC.build_model().state_dict()}, path)
    model = deploy.load_weights(model_create_by_name("dispnet", 192), path).eval().cuda()
    rng = np.random.default_rng(1)
    left = rng.integers(0, 256, (64, 128, 3), dtype=np.uint8)
    with options(cv, conv_precision="f16x2", conv2d_k5=True, wide_conv2d=True):
        d = deploy.disp_predict(model, left, np.roll(left, -5, axis=1))
    assert d.shape == (64, 128) and d.dtype == np.float32 and np.isfinite(d).all()
