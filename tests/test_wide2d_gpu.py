"""GPU: the wide 3x3 2-D layers (Cout 256 / 512 / 1024; dsmnet_amd/csrc/conv_wide2d.hpp) against float64
``F.conv2d`` + bias (+ ReLU) on the CPU, their determinism, ``y_amax``, and DispNetC / iResNet with the
``wide_conv2d`` option on against off.

Bands (tests/test_f16_gpu.py): f16x2 -- max <= 1.5e-6 of the largest output, rms <= 6e-7 of the output rms;
f16 -- max <= 3e-3, rms <= 6e-4.  Every shape leaves tiles, K-ranges and borders partial."""
import ctypes
import functools
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import maxerr, seeded

pytestmark = pytest.mark.gpu

F16X2_MAX, F16X2_RMS = 1.5e-6, 6e-7
F16_MAX, F16_RMS = 3e-3, 6e-4
DISP_TOL = 1e-3           # the north-star bound of tests/test_models_gpu.py

# (B, Cin, H, W), Cout, stride, input scale
CASES = [
    ((1, 1024, 6, 20), 1024, 1, 1.0),      # the real conv6b: the smallest M, the largest K
    ((2, 48, 7, 11), 256, 1, 1e-6),        # Cin % 32 != 0, M = 154, batch 2; tiny inputs
    ((1, 256, 7, 11), 512, 2, 1e4),        # odd H and W: a 4 x 6 output; large inputs
    ((2, 512, 5, 33), 512, 1, 1.0),        # a 33-wide row crosses a 32-pixel tile
    ((1, 16, 1, 1), 256, 1, 1.0),          # only the centre tap sees data
    ((1, 512, 12, 40), 1024, 2, 1.0),
]


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@contextmanager
def options(cv, **kw):
    old = {k: cv.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            cv.set_option(k, v)


@functools.lru_cache(maxsize=None)
def case_data(i):
    """(x, w, bias, float64 conv + bias before the activation) of CASES[i]: computed once, never modified.
    The bias has the spread of the convolution's output, so that ReLU clips about half the outputs with a
    different share in every channel."""
    shape, cout, stride, xs = CASES[i]
    cin = shape[1]
    x = seeded(500 + i, *shape, scale=xs)
    w = seeded(600 + i, cout, cin, 3, 3, scale=(2.0 / (9 * cin)) ** 0.5)
    pre = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    b = (seeded(700 + i, cout).double() * pre.std()).float()
    return x, w, b, pre + b.double().view(1, -1, 1, 1)


def errors(y, ref):
    err = (y.double().cpu() - ref).abs()
    return err.max().item() / ref.abs().max().item(), (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def run_case(cv, i, relu, mode="f16x2", flags=0):
    x, w, b, _ = case_data(i)
    _, cout, stride, _ = CASES[i]
    with options(cv, conv_precision=mode, conv_flags=flags):
        xg = x.cuda().contiguous(memory_format=torch.channels_last)
        return cv.conv2d_block(xg, cv.pack_conv2d_weight(w.cuda()), cout, torch.ones(cout, device="cuda"), b.cuda(),
                               stride=stride, relu=relu)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", ["f16x2", "f16"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_parity_against_float64(cv, i, mode, relu):
    ref = case_data(i)[3]
    ref = ref.relu() if relu else ref
    if relu:
        clipped = (ref == 0).double().mean().item()
        assert 0.3 <= clipped <= 0.7, clipped
    y = run_case(cv, i, relu, mode)
    assert tuple(y.shape) == tuple(ref.shape) and y.is_contiguous(memory_format=torch.channels_last)
    emax, erms = errors(y, ref)
    print("case %d %s relu=%d: max %.2e rms %.2e" % (i, mode, relu, emax, erms))
    lim = (F16X2_MAX, F16X2_RMS) if mode == "f16x2" else (F16_MAX, F16_RMS)
    assert emax <= lim[0] and erms <= lim[1], (emax, erms)


@pytest.mark.parametrize("i", [0, 2, 3])
def test_the_same_call_twice_gives_identical_bits(cv, i):
    a, b = run_case(cv, i, 1), run_case(cv, i, 1)
    assert torch.equal(a, b)


# case 2 (16 chunks: 2 .. 16 ranges; 1 is raised to 2) and case 0 (64 chunks: 8 .. 63)
@pytest.mark.parametrize("i,ks,grid", [(2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 5, 0), (2, 8, 0), (2, 16, 0), (2, 63, 0),
                                       (2, 0, 7), (2, 3, 5), (0, 8, 0), (0, 32, 0), (0, 63, 0), (0, 0, 50),
                                       (3, 0, 3), (4, 1, 1)])
def test_forced_splits_and_grids_stay_inside_the_band(cv, i, ks, grid):
    from dsmnet_amd import _lib
    flags = (ks << _lib.DSM_CONV_KSPLIT_SHIFT) | (grid << _lib.DSM_CONV_BLOCKS_SHIFT)
    ref = case_data(i)[3].relu()
    y = run_case(cv, i, 1, flags=flags)
    emax, erms = errors(y, ref)
    print("case %d ks=%d grid=%d: max %.2e rms %.2e" % (i, ks, grid, emax, erms))
    assert emax <= F16X2_MAX and erms <= F16X2_RMS, (emax, erms)
    assert torch.equal(y, run_case(cv, i, 1, flags=flags))


def raw_launch(cv, i, y_amax):
    """``dsm_conv3d_fwd`` with a caller-owned ``y_amax`` slot."""
    from dsmnet_amd import _lib
    x, w, b, _ = case_data(i)
    (B, cin, H, W), cout, stride, _ = CASES[i]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xg = x.cuda().contiguous(memory_format=torch.channels_last)
    packed, bias = cv.pack_conv2d_weight(w.cuda()), b.cuda()
    y = torch.empty((B, cout, Ho, Wo), device="cuda").contiguous(memory_format=torch.channels_last)
    xa = cv.absmax(xg)
    a = _lib.Conv3dArgs()
    a.x, a.w_packed, a.y, a.shift = xg.data_ptr(), packed.data_ptr(), y.data_ptr(), bias.data_ptr()
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi, a.Do, a.Ho, a.Wo = 1, H, W, 1, Ho, Wo
    a.stride, a.relu, a.kd, a.k, a.dil = stride, 1, 1, 3, 1
    a.precision, a.x_amax, a.y_amax = _lib.DSM_PREC_F16X2, xa.data_ptr(), y_amax.data_ptr()
    nws = _lib.load().dsm_conv3d_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(max(nws // 4, 4), device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    _lib.check(_lib.load().dsm_conv3d_fwd(ctypes.byref(a), cv._stream()), "dsm_conv3d_fwd")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("i", [0, 1, 4])       # K-split (the reduce pass folds the maximum) and single-range layers
def test_y_amax(cv, i):
    slot = torch.zeros(1, device="cuda")
    y = raw_launch(cv, i, slot)
    assert slot.item() == y.abs().max().item()
    big = torch.full((1,), 2.0 * y.abs().max().item(), device="cuda")
    want = big.item()
    raw_launch(cv, i, big)
    assert big.item() == want                    # a slot that already holds more is left alone
    y2 = run_case(cv, i, 1)                      # and the host wrapper hands the maximum to the next layer
    assert y2._dsm_amax.item() == y2.abs().max().item()


# ---------------------------------------------------------------------------------------- models --
CHAIN_LAYERS = {"dispnetcorr": ["conv3b", "conv4a", "conv4b", "conv5a", "conv5b", "conv6a", "conv6b"],
                "iresnet": ["conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1"]}


def make_model(name):
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(11)
    return model_create_by_name(name, 192).cuda().eval()


def images64():
    return seeded(21, 1, 3, 64, 128).cuda(), seeded(22, 1, 3, 64, 128).cuda()


def forward(cv, m, imL, imR, wide, timer=None):
    with options(cv, conv_precision="f16x2", wide_conv2d=wide), torch.no_grad():
        torch.manual_seed(5)                     # iResNet's warp draws an epsilon
        cv.set_timer(timer)
        try:
            return m(imL, imR)[1]
        finally:
            cv.set_timer(None)


@pytest.mark.parametrize("name", ["dispnetcorr", "iresnet"])
def test_models_option_on_equals_off_and_runs_the_chain_on_the_wide_kernel(cv, name):
    m = make_model(name)
    imL, imR = images64()
    off_timer, on_timer = cv.LaunchTimer(), cv.LaunchTimer()
    off = forward(cv, m, imL, imR, False, off_timer)
    on = forward(cv, m, imL, imR, True, on_timer)
    torch.cuda.synchronize()
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and maxerr(a, b) <= DISP_TOL, (k, maxerr(a, b))

    def wide_launches(t):
        return sum(v["launches"] for k, v in t.summary().items() if k.startswith("conv2d_wide_"))
    assert wide_launches(on_timer) == len(CHAIN_LAYERS[name]) == 7
    assert wide_launches(off_timer) == 0


@pytest.mark.parametrize("name", ["dispnetcorr", "iresnet"])
def test_models_capture_into_a_graph_and_replay_the_chain_bit_for_bit(cv, name):
    from dsmnet_amd.graphs import GraphedForward
    m = make_model(name)
    imL, imR = images64()
    seen = {}
    last = getattr(m, CHAIN_LAYERS[name][-1])
    handle = last.register_forward_hook(lambda mod, inp, out: seen.__setitem__("y", out))
    try:
        eager = forward(cv, m, imL, imR, True)
        chain_eager = seen["y"].clone()
        with options(cv, conv_precision="f16x2", wide_conv2d=True):
            g = GraphedForward(m, imL, imR, warmup=1)
            static = seen["y"]                   # the captured forward's conv6b output: rewritten by every replay
            static.zero_()
            outs = g(imL, imR)[1]
        torch.cuda.synchronize()
    finally:
        handle.remove()
    assert len(outs) == len(eager)
    assert torch.equal(static, chain_eager)      # (the final disparities pass through stock layers: not asserted)


def test_training_and_autograd_take_the_stock_path(cv):
    m = make_model("dispnetcorr")
    imL, imR = images64()
    timer = cv.LaunchTimer()
    with options(cv, conv_precision="f16x2", wide_conv2d=True):
        cv.set_timer(timer)
        try:
            with torch.enable_grad():            # eval mode, autograd on
                outs = m(imL, imR)[1]
                sum(o.sum() for o in outs).backward()
            assert m.conv6b[0].weight.grad is not None and m.conv6b[0].weight.grad.abs().sum().item() > 0
            m.zero_grad()
            m.train()
            with torch.no_grad():                # train mode, autograd off
                m(imL, imR)
        finally:
            cv.set_timer(None)
    torch.cuda.synchronize()
    assert not [k for k in timer.summary() if k.startswith("conv2d_wide_")]
