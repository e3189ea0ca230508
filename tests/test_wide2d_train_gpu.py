"""GPU: training through the wide 3x3 layers -- the transposed mode of the wide kernel (backward-data of the
stride-2 layers), ``dsm_bias_relu_bwd``, ``costvolume.wide_conv2d_relu`` and the option ``wide_conv2d_train``
in DispNetC / iResNet.

References are float64 CPU autograd (tests/wide2d_train_cases.py; tests/test_wide2d_train_reference.py
shows that they are accurate enough for the bounds).  Forward bands are the wide kernel's own
(tests/test_wide2d_gpu.py): f16x2 max <= 1.5e-6 of the largest output / rms <= 6e-7 of the output rms, f16
3e-3 / 6e-4.  Gradient bounds are those of tests/test_bwd_ranges_gpu.py: 1e-4 (f16x2) / 4e-3 (f16) of the
largest entry of the reference gradient, with the kernel's OWN ReLU mask applied to the cotangent of the
reference (a flipped mask entry is an O(1e-2) outlier that says nothing about the gradient kernels); the
mask itself is held to the forward band separately."""
import copy
import functools
import random
from contextlib import contextmanager

import pytest
import torch

from tests import wide2d_train_cases as T
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "f16"]


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


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def count(timer, prefix):
    return sum(v["launches"] for k, v in timer.summary().items() if k.startswith(prefix))


# ------------------------------------------------------------- 1. the transposed launch against float64 --
@functools.lru_cache(maxsize=None)
def transposed_case(key):
    """(g, w, float64 dX) of the backward-data launch of CASES[key] for the float64 mask."""
    x, w, b, pre, cot = T.case_data(key)
    mask = pre > 0
    return (cot * mask.float()), w, T.grads64(key, mask)[0]


def run_transposed(cv, key, mode="f16x2", flags=0):
    g, w, _ = transposed_case(key)
    (B, cin, H, W), cout, _ = T.CASES[key]
    with options(cv, conv_precision=mode, conv_flags=flags):
        packed = cv.pack_conv2d_weight(w.cuda().flip(2, 3).transpose(0, 1).contiguous())
        return cv.conv2d_transposed_block(cl(g), packed, cin, (H, W))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", T.STRIDE2)
def test_transposed_launch_against_float64(cv, key, mode):
    ref = transposed_case(key)[2]
    y = run_transposed(cv, key, mode)
    assert tuple(y.shape) == tuple(ref.shape) and y.is_contiguous(memory_format=torch.channels_last)
    emax, erms = T.band_errors(y, ref)
    print("transposed %s %s: max %.2e rms %.2e" % (key, mode, emax, erms))
    assert emax <= T.BANDS[mode][0] and erms <= T.BANDS[mode][1], (emax, erms)
    assert torch.equal(y, run_transposed(cv, key, mode))                 # the same call twice: identical bits
    assert y._dsm_amax.item() == y.abs().max().item()


def test_the_transposed_shapes_start_blocks_at_odd_rows_and_columns(cv, hip_lib):
    """E: two M-blocks of 11 rows; F: seven column blocks of 11 -- read back from the plan's unit count."""
    from dsmnet_amd import _lib
    from tests.test_wide2d_train_reference import dx_args
    from tests.test_wide2d_plans import plan
    for key, want in (("E", (11, 36, 2, 1)), ("F", (21, 11, 1, 7))):
        (B, cin, H, W), cout, _ = T.CASES[key]
        R, CW, nby, nbx = T.geometry_s1(H, W)
        assert (R, CW, nby, nbx) == want
        rc, name = plan(hip_lib, dx_args(key, "f16x2"))
        n, ks, units = (int(name.split(k)[1].split(",")[0].rstrip(">")) for k in ("N=", "KS=", "units="))
        assert rc == 0 and units == B * nby * nbx * (cin // n) * ks, (name, nby, nbx)


# B: Cin = 512 (32 chunks: 4 .. 32 ranges); D: Cin = 1024 (64 chunks: 8 .. 63) -- the values of
# tests/test_wide2d_gpu.py::test_forced_splits_and_grids_stay_inside_the_band
@pytest.mark.parametrize("key,ks,grid", [("B", 1, 0), ("B", 2, 0), ("B", 3, 0), ("B", 5, 0), ("B", 8, 0), ("B", 16, 0),
                                         ("B", 63, 0), ("B", 0, 7), ("B", 3, 5), ("D", 8, 0), ("D", 32, 0),
                                         ("D", 63, 0), ("D", 0, 50), ("E", 0, 3), ("F", 1, 1)])
def test_transposed_forced_splits_and_grids_stay_inside_the_band(cv, key, ks, grid):
    from dsmnet_amd import _lib
    flags = (ks << _lib.DSM_CONV_KSPLIT_SHIFT) | (grid << _lib.DSM_CONV_BLOCKS_SHIFT)
    ref = transposed_case(key)[2]
    y = run_transposed(cv, key, flags=flags)
    emax, erms = T.band_errors(y, ref)
    print("transposed %s ks=%d grid=%d: max %.2e rms %.2e" % (key, ks, grid, emax, erms))
    assert emax <= T.F16X2_MAX and erms <= T.F16X2_RMS, (emax, erms)
    assert torch.equal(y, run_transposed(cv, key, flags=flags))
    assert y._dsm_amax.item() == y.abs().max().item()


# ------------------------------------------------------------------------------- 2. dsm_bias_relu_bwd --
def relu_bwd(cv, gy, y, want_db=True, want_amax=True):
    from dsmnet_amd import _lib
    M, C = y.shape
    g = torch.full_like(y, float("nan"))
    db = torch.full((C,), float("nan"), device="cuda") if want_db else None
    ws = torch.empty(512 * C, device="cuda") if want_db else None
    am = torch.zeros(1, device="cuda") if want_amax else None
    p = cv._p
    rc = _lib.load().dsm_bias_relu_bwd(p(gy), p(y), p(g), p(db), p(ws), p(am), M, C, cv._stream())
    _lib.check(rc, "dsm_bias_relu_bwd")
    torch.cuda.synchronize()
    return g, db, am


@pytest.mark.parametrize("M,C", [(120, 1024), (154, 256), (1, 256), (1260, 256)])
def test_bias_relu_bwd(cv, M, C):
    y = seeded(31, M, C)
    y.view(-1)[::7] = 0.0
    y.view(-1)[3::11] = -0.0
    gy = seeded(32, M, C)
    yg, gyg = y.cuda(), gy.cuda()
    keep = gyg.clone()
    g, db, am = relu_bwd(cv, gyg, yg)
    want = torch.where(y > 0, gy, torch.zeros_like(gy))
    assert torch.equal(g.cpu().view(torch.int32), want.view(torch.int32))            # bit-equal, +0.0 where clipped
    assert torch.equal(gyg, keep)                                                    # gy is never written
    assert am.item() == want.abs().max().item()
    db64 = want.double().sum(0)
    bound = M * 2.0 ** -24 * want.double().abs().sum(0)
    err = (db.double().cpu() - db64).abs()
    print("bias_relu_bwd %dx%d: worst db error / bound %.3f" % (M, C, (err / bound.clamp_min(1e-300)).max().item()))
    assert bool((err <= bound).all())
    g2, db2, am2 = relu_bwd(cv, gyg, yg)
    assert torch.equal(db2.view(torch.int32), db.view(torch.int32)) and torch.equal(g2, g)   # two runs, the same bits
    g3, db3, am3 = relu_bwd(cv, gyg, yg, want_db=False, want_amax=False)
    assert db3 is None and am3 is None and torch.equal(g3, g)
    big = torch.full((1,), 2.0 * want.abs().max().item() + 1.0, device="cuda")       # a slot that holds more is left alone
    held = big.item()
    from dsmnet_amd import _lib
    _lib.check(_lib.load().dsm_bias_relu_bwd(cv._p(gyg), cv._p(yg), cv._p(g3), None, None, cv._p(big), M, C,
                                             cv._stream()), "dsm_bias_relu_bwd")
    assert big.item() == held


# -------------------------------------------------------------------------------------- 3. the function --
def run_function(cv, key, need_dx=True, timer=None):
    """(y, dX, dW, db) of CASES[key] through ``wide_conv2d_relu``, one scope around forward and backward."""
    x, w, b, pre, cot = T.case_data(key)
    stride = T.CASES[key][2]
    xg = cl(x).requires_grad_(need_dx)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with cv.amax_scope(dev()):
        y = cv.wide_conv2d_relu(xg, wg, bg, stride)
        cv.set_timer(timer)
        try:
            y.backward(cl(cot))
        finally:
            cv.set_timer(None)
    torch.cuda.synchronize()
    return y.detach(), xg.grad, wg.grad, bg.grad


def check_gradients(key, mode, y, grads, tag=""):
    """The mask against the forward band, then dX, dW, db against float64 autograd with the kernel's mask."""
    pre = T.case_data(key)[3]
    mask = y.cpu() > 0
    wrong = mask != (pre > 0)
    band = T.BANDS[mode][0] * pre.abs().max().item()
    assert wrong.sum().item() == 0 or pre[wrong].abs().max().item() <= band, (key, mode, wrong.sum().item())
    errs = []
    for what, got, ref in zip(("dX", "dW", "db"), grads, T.grads64(key, mask)):
        assert got is not None and tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all()), what
        errs.append(T.rel(got, ref))
    print("%s %s%s: mask flips %d, dX %.2e dW %.2e db %.2e (bound %.0e)"
          % (key, mode, tag, wrong.sum().item(), errs[0], errs[1], errs[2], T.TOL[mode]))
    assert max(errs) <= T.TOL[mode], (key, mode, errs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", T.IDS)
def test_function_forward_and_gradients_against_float64(cv, key, mode):
    pre = T.case_data(key)[3]
    ref = pre.relu()
    clipped = (ref == 0).double().mean().item()
    assert 0.3 <= clipped <= 0.7, clipped
    with options(cv, conv_precision=mode):
        y, dx, dw, db = run_function(cv, key)
        again = run_function(cv, key)
    assert y.is_contiguous(memory_format=torch.channels_last)
    emax, erms = T.band_errors(y, ref)
    print("%s %s forward: max %.2e rms %.2e" % (key, mode, emax, erms))
    assert emax <= T.BANDS[mode][0] and erms <= T.BANDS[mode][1], (emax, erms)
    check_gradients(key, mode, y, (dx, dw, db))
    assert torch.equal(again[0], y) and torch.equal(again[1], dx) and torch.equal(again[3], db)   # (dW: the bound only)
    assert T.rel(again[2], dw.double().cpu()) <= 2 * T.TOL[mode]


@pytest.mark.parametrize("key", ["B", "C"])
def test_no_backward_data_launch_when_the_input_needs_no_gradient(cv, key):
    with options(cv, conv_precision="f16x2"):
        t0, t1 = cv.LaunchTimer(), cv.LaunchTimer()
        y, dx, dw, db = run_function(cv, key, need_dx=False, timer=t0)
        full = run_function(cv, key, need_dx=True, timer=t1)
    assert dx is None and dw is not None and db is not None
    assert count(t0, "conv2d_wide_") + count(t0, "deconv2d_wide_") == 0
    assert count(t1, "conv2d_wide_") + count(t1, "deconv2d_wide_") == 1          # the timer sees the launch when there is one
    assert count(t0, "dsm_bias_relu_bwd") == 1 and count(t0, "conv2d_wgrad_kernel<") == 1
    assert torch.equal(db, full[3])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["B", "C"])
def test_backward_after_the_arena_began_again(cv, key, mode):
    """forward(x) in a scope, then a forward of x * 2^-12 in a scope of its own, then the first forward's
    backward: the saved maxima are stale and ``amax_of`` replaces them (tests/test_amax_lifetime_gpu.py)."""
    x, w, b, pre, cot = T.case_data(key)
    stride = T.CASES[key][2]
    with options(cv, conv_precision=mode):
        xg = cl(x).requires_grad_(True)
        wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        with cv.amax_scope(dev()):
            y = cv.wide_conv2d_relu(xg, wg, bg, stride)
        with cv.amax_scope(dev()), torch.no_grad():
            cv.wide_conv2d_relu(cl(x * 2.0 ** -12), wg, bg, stride)
        y.backward(cl(cot))
        torch.cuda.synchronize()
    check_gradients(key, mode, y.detach(), (xg.grad, wg.grad, bg.grad), tag=" (stale slots)")


@pytest.mark.parametrize("switched", ["bf16x3", "fp32"])
def test_backward_runs_in_the_mode_of_its_forward(cv, switched):
    """``conv_precision`` switched between forward and backward: the backward keeps the forward's mode, which it
    hands to its launches (under "fp32" a launch that read the option would ask for the fp32-input MFMA)."""
    key = "B"
    x, w, b, pre, cot = T.case_data(key)
    with options(cv, conv_precision="f16x2"):
        xg = cl(x).requires_grad_(True)
        wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        with cv.amax_scope(dev()):
            y = cv.wide_conv2d_relu(xg, wg, bg, T.CASES[key][2])
            with options(cv, conv_precision=switched):
                y.backward(cl(cot))
                assert cv.get_option("conv_precision") == switched
        torch.cuda.synchronize()
    check_gradients(key, "f16x2", y.detach(), (xg.grad, wg.grad, bg.grad), tag=" (mode switched to %s)" % switched)


# ------------------------------------------------------------------------------------------- 4. chain --
CHAIN_LAYERS = {"dispnetcorr": ["conv3b", "conv4a", "conv4b", "conv5a", "conv5b", "conv6a", "conv6b"],
                "iresnet": ["conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1"]}
CHAIN_SEED = 43


def make_model(name, seed=11):
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(seed)
    return model_create_by_name(name, 192)


def test_the_seven_layers_as_a_chain_against_float64(cv):
    m = make_model("dispnetcorr")
    layers = [getattr(m, n) for n in CHAIN_LAYERS["dispnetcorr"]]
    x = seeded(CHAIN_SEED, 1, 256, 16, 24)
    # float64 CPU autograd of the same chain, with its own masks
    ref_layers = copy.deepcopy(layers)
    x64 = x.double().requires_grad_(True)
    h, near = x64, 0
    for lay in ref_layers:
        lay.double()
        pre = lay[0](h)
        near += int((pre.detach().abs() <= T.F16X2_MAX * pre.detach().abs().max()).sum())
        h = pre.relu()
    # no pre-activation so close to zero that the forward band could flip its mask entry: the comparison below
    # is then one of gradients, not of masks
    assert near == 0, near
    cot = seeded(CHAIN_SEED + 1, *h.shape)
    h.backward(cot.double())
    want = [x64.grad] + [p.grad for lay in ref_layers for p in lay[0].parameters()]

    for lay in layers:
        lay.cuda().train()
    xg = cl(x).requires_grad_(True)
    timer = cv.LaunchTimer()
    with options(cv, conv_precision="f16x2", wide_conv2d_train=True), cv.amax_scope(dev()):
        cv.set_timer(timer)
        try:
            y = xg
            for lay in layers:
                y = lay(y)
                assert y.is_contiguous(memory_format=torch.channels_last)       # NHWC between the layers
            y.backward(cl(cot))
        finally:
            cv.set_timer(None)
    torch.cuda.synchronize()
    assert count(timer, "conv2d_wide_") == 7 + 4 and count(timer, "deconv2d_wide_") == 3
    assert count(timer, "absmax_kernel") == 1                                   # the input only: every other maximum rides along
    got = [xg.grad] + [p.grad for lay in layers for p in lay[0].parameters()]
    assert len(got) == len(want) == 15
    errs = [T.rel(y, h.detach())] + [T.rel(a, b) for a, b in zip(got, want)]
    print("chain: y %.2e, dX %.2e, parameter gradients worst %.2e" % (errs[0], errs[1], max(errs[2:])))
    assert max(errs) <= 1e-4, errs


# ------------------------------------------------------------------------------------------ 5. models --
def step_counts(timer):
    return {"fwd+dx s1": count(timer, "conv2d_wide_"), "dx s2": count(timer, "deconv2d_wide_"),
            "relu": count(timer, "dsm_bias_relu_bwd"),
            "wgrad": sum(v["launches"] for k, v in timer.summary().items()
                         if k.startswith("conv2d_wgrad_kernel<") and int(k.rstrip(">").split("x")[-1]) >= 256)}


WANT_ON = {"fwd+dx s1": 7 + 4, "dx s2": 3, "relu": 7, "wgrad": 7}
WANT_OFF = {"fwd+dx s1": 0, "dx s2": 0, "relu": 0, "wgrad": 0}


def test_dispnetc_train_steps_follow_the_stock_trajectory(cv):
    from dsmnet_amd import train
    from tests.test_train_gpu import _batch
    m_off = make_model("dispnetcorr", seed=0).cuda()
    m_on = copy.deepcopy(m_off)
    batch = _batch(2, 256, 512, 6, 3)
    losses, counts = {}, {}
    for tag, model in (("off", m_off), ("on", m_on)):
        lossfun = train.losses("supervised", model.count_levels, maxepoch_weight_adjust=37)
        lossfun.Weight_Adjust_levels(10)
        opt = train.make_optimizer(model, lr=1e-4)
        timer = cv.LaunchTimer()
        with options(cv, conv_precision="f16x2", wide_conv2d_train=(tag == "on")):
            cv.set_timer(timer)
            try:
                first = train.train_step(model, opt, lossfun, batch)[0]
            finally:
                cv.set_timer(None)
            torch.cuda.synchronize()
            counts[tag] = step_counts(timer)
            losses[tag] = [first] + [train.train_step(model, opt, lossfun, batch)[0] for _ in range(3)]
    print("dispnetcorr train steps: off %s on %s" % (losses["off"], losses["on"]))
    assert counts["on"] == WANT_ON and counts["off"] == WANT_OFF, counts
    for a, b in zip(losses["off"], losses["on"]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), losses
    assert losses["on"][-1] < losses["on"][0]


def test_iresnet_forward_and_backward_run_the_seven_layers_on_the_new_path(cv):
    m = make_model("iresnet").cuda().eval()
    imL, imR = seeded(21, 1, 3, 64, 128).cuda(), seeded(22, 1, 3, 64, 128).cuda()
    timer = cv.LaunchTimer()
    with options(cv, conv_precision="f16x2", wide_conv2d_train=True), cv.amax_scope(dev()), torch.enable_grad():
        torch.manual_seed(5)                         # iResNet's warp draws an epsilon
        cv.set_timer(timer)
        try:
            outs = m(imL, imR)[1]
            sum(o.sum() for o in outs).backward()
        finally:
            cv.set_timer(None)
    torch.cuda.synchronize()
    assert step_counts(timer) == WANT_ON, step_counts(timer)
    for name in CHAIN_LAYERS["iresnet"]:
        for p in getattr(m, name)[0].parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().sum().item() > 0, name


def test_selfsup_step_shares_one_pack_per_layer_between_its_two_forwards(cv):
    from dsmnet_amd import train, transforms
    from tests.test_selfsup_gpu import _selfsup_batch
    model = make_model("dispnetcorr", seed=1).cuda()
    lossfun = train.losses("depthmono-mask", 7)
    lossfun.Weight_Adjust_levels(2)
    opt = train.make_optimizer(model, lr=1e-4)
    batch = _selfsup_batch(1, 128, 256, 31)
    losses = []
    with options(cv, conv_precision="f16x2", wide_conv2d_train=True):
        for step in range(3):
            before = dict(cv._WIDE_PACK_MISSES)
            timer = cv.LaunchTimer()
            cv.set_timer(timer if step == 0 else None)
            try:
                random.seed(9)                       # Stereo_color draws from ``random`` and from torch's CPU generator
                torch.manual_seed(9)                 # (tests/test_color_gpu.py): the same augmentation and epsilon draws
                                                     # every step, so the three losses are values of ONE objective
                losses.append(train.train_step_selfsup(model, opt, lossfun, batch, augment=transforms.Stereo_color(),
                                                       nedge=0)[0])
            finally:
                cv.set_timer(None)
            made = {k: cv._WIDE_PACK_MISSES[k] - before[k] for k in before}
            assert made == {"forward": 7, "gradient": 7}, made                  # two forwards, two backwards: one pack each
            if step == 0:
                torch.cuda.synchronize()
                c = step_counts(timer)
                assert c == {k: 2 * v for k, v in WANT_ON.items()}, c
    print("selfsup steps: %s" % (losses,))
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert losses[-1] < losses[0]


# ----------------------------------------------------------------------------------------- 6. capture --
def test_forward_and_backward_capture_into_a_graph(cv):
    key = "B"
    x, w, b, pre, cot = T.case_data(key)
    stride = T.CASES[key][2]
    with options(cv, conv_precision="f16x2"):
        eager = run_function(cv, key)
        xg = cl(x).requires_grad_(True)
        wg, bg, cg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True), cl(cot)

        def step():
            with cv.amax_scope(dev()):
                y = cv.wide_conv2d_relu(xg, wg, bg, stride)
                return (y,) + torch.autograd.grad(y, [xg, wg, bg], cg)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        for _ in range(2):
            for o in outs:
                o.detach().zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[0].detach(), eager[0])
            assert torch.equal(outs[1], eager[1]) and torch.equal(outs[3], eager[3])
            assert T.rel(outs[2], eager[2].double().cpu()) <= 2 * T.TOL["f16x2"]
