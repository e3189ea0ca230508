"""GPU: the fused colour augmentation (csrc/color.hip, dsmnet_amd.transforms) against the float64
restatement with explicit parameters, the whole Stereo_color_batch against the reference's
per-image loop restated with torch ops on the device (same seeds: the planner must consume the CPU
and GPU generators exactly as the reference does), launch count, host synchronisation, and the
self-supervised train / validate steps with the transforms as ``augment``.

Bound against float64: 1e-5 absolute on the normalised output (fp32 steps, accurate powf,
division by std ~0.22 amplifies the last-bit differences ~4.5x)."""
import itertools
import random

import numpy as np
import pytest
import torch

from tests import color_oracle as CO

pytestmark = pytest.mark.gpu

PERMS = list(itertools.permutations(range(4)))


def _images(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g)
    x[:, :6, : max(1, H // 2), : max(1, W // 3)] *= 0.06        # dark: negative values before Gamma
    x[:, :6, -1, : (W + 1) // 2] = 0.0                          # exactly 0 and 1
    x[:, :6, -1, (W + 1) // 2:] = 1.0
    if C > 6:
        x[:, 6:] = torch.rand(B, C - 6, H, W, generator=g) * 40 - 20
    return x


def _records(B, groups, same, seed, perm_offset=0, flags=CO.JITTER | CO.LIGHTING | CO.NORMALIZE):
    """Explicit parameters: image b takes order PERMS[(b + perm_offset) % 24] (shifted per group
    when not ``same``), jitter values at the extremes of the reference's range."""
    rng = np.random.RandomState(seed)
    recs = []
    for b in range(B):
        for g in range(groups):
            k = (b + perm_offset + (0 if same else 7 * g)) % 24
            u = rng.uniform(-0.2, 0.2, size=4)
            u[1] = -0.2 if b % 2 == 0 else u[1]                     # Contrast pushing below 0
            jit = (1 + u[0], u[1], u[2], 1 + u[3])
            row = b * groups + (0 if same else g)
            recs.append((PERMS[k], jit, flags, row))
    alpha = torch.from_numpy(rng.normal(0, 0.1, size=(B, groups, 3))).float()
    return recs, alpha


def _check(x, recs, alpha, groups, bound=1e-5):
    from dsmnet_amd import costvolume as cv
    want = CO.restate(x, recs, alpha, groups)
    xd = x.cuda()
    out = cv.stereo_color(xd, recs, alpha.cuda(), groups)
    assert out is xd
    got = xd.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    assert err <= bound, err
    assert torch.equal(got[:, 3 * groups:], x[:, 3 * groups:].double())   # untouched channels
    return err


@pytest.mark.parametrize("same", [True, False])
def test_all_24_orders(hip_lib, same):
    x = _images(24, 6, 12, 40, 1)
    recs, alpha = _records(24, 2, same, 2)
    _check(x, recs, alpha, 2)


@pytest.mark.parametrize("C,H,W", [(6, 9, 13), (7, 5, 3), (9, 7, 1), (7, 11, 36), (6, 4, 4)])
def test_shapes_and_scalar_tail(hip_lib, C, H, W):
    x = _images(5, C, H, W, 3)
    for groups, same in ((2, True), (2, False), (1, False)):
        recs, alpha = _records(5, groups, same, 4, perm_offset=5)
        _check(x, recs, alpha, groups)


def test_batch_above_the_record_cap(hip_lib):
    """40 images x 2 groups = 80 records: two launches of 64 and 16."""
    x = _images(40, 7, 6, 24, 5)
    recs, alpha = _records(40, 2, False, 6)
    _check(x, recs, alpha, 2)
    x = _images(70, 6, 3, 8, 7)
    recs, alpha = _records(70, 1, False, 8)
    _check(x, recs, alpha, 1)


def test_unaligned_base_takes_the_scalar_path(hip_lib):
    from dsmnet_amd import costvolume as cv
    x = _images(2, 6, 8, 16, 9)
    recs, alpha = _records(2, 2, True, 10)
    want = CO.restate(x, recs, alpha, 2)
    buf = torch.zeros(x.numel() + 1, device="cuda")
    xd = buf[1:].view(x.shape)
    xd.copy_(x)
    cv.stereo_color(xd, recs, alpha.cuda(), 2)
    assert (xd.cpu().double() - want).abs().max().item() <= 1e-5
    assert buf[0].item() == 0.0


def test_step_subsets(hip_lib):
    x = _images(3, 6, 8, 20, 11)
    for flags in (CO.NORMALIZE, CO.JITTER, CO.LIGHTING, CO.JITTER | CO.LIGHTING, 0):
        recs, alpha = _records(3, 2, True, 12, flags=flags)
        _check(x, recs, alpha, 2)


def test_argument_errors(hip_lib):
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import transforms as T
    recs = [((0, 1, 2, 3), (1.0, 0.0, 0.0, 1.0), CO.NORMALIZE, 0)] * 4
    x = torch.rand(2, 6, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        cv.stereo_color(x.double(), recs, None, 2)
    with pytest.raises(ValueError):
        cv.stereo_color(torch.rand(2, 6, 8, 12, device="cuda")[..., 2:10], recs, None, 2)   # strided crop
    with pytest.raises(ValueError):
        cv.stereo_color(torch.rand(1, 6, 8, 8, device="cuda").expand(2, 6, 8, 8), recs, None, 2)
    with pytest.raises(ValueError):
        cv.stereo_color(torch.rand(2, 5, 8, 8, device="cuda"), recs, None, 2)
    with pytest.raises(ValueError):
        cv.stereo_color(x, recs[:3], None, 2)
    with pytest.raises(ValueError):
        T.Stereo_color()(torch.rand(2, 3, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        T.Stereo_color()(torch.rand(2, 6, 20, 20, device="cuda")[:, :, 2:10, 2:10])


def _batch(B, C, H, W, seed):
    return _images(B, C, H, W, seed).cuda()


@pytest.mark.parametrize("same", [True, False])
def test_stereo_color_batch_vs_device_restatement(hip_lib, same):
    from dsmnet_amd import transforms as T
    x = _batch(3, 7, 24, 40, 13)
    a, b = x.clone(), x.clone()
    random.seed(21)
    torch.manual_seed(21)
    out = T.Stereo_color_batch(a, T.Stereo_color(same_group=same))
    after = (random.random(), torch.rand(1).item(), torch.rand(1, device="cuda").item())
    random.seed(21)
    torch.manual_seed(21)
    CO.stereo_color_batch_torch(b, same_group=same)
    assert after == (random.random(), torch.rand(1).item(), torch.rand(1, device="cuda").item())
    assert out is a
    assert torch.isfinite(a).all()
    err = (a - b).abs().max().item()
    assert err <= 1e-5, err
    assert torch.equal(a[:, 6:], x[:, 6:])


def test_single_image_and_stereo_normalize(hip_lib):
    from dsmnet_amd import transforms as T
    x = _batch(2, 7, 16, 30, 17)
    a, b = x.clone(), x.clone()
    T.Stereo_normalize()(a)
    CO.stereo_color_batch_torch(b, color=False)
    assert (a - b).abs().max().item() <= 1e-6
    recs = [((0, 1, 2, 3), (1.0, 0.0, 0.0, 1.0), CO.NORMALIZE, 0)] * 4
    assert (a.cpu().double() - CO.restate(x.cpu(), recs, None, 2)).abs().max().item() <= 1e-6
    img = x[1].clone()
    random.seed(5)
    torch.manual_seed(5)
    assert T.Stereo_color()(img) is img
    c = x[1:2].clone()
    random.seed(5)
    torch.manual_seed(5)
    CO.stereo_color_batch_torch(c)
    assert (img - c[0]).abs().max().item() <= 1e-5


def test_no_host_synchronisation(hip_lib):
    from dsmnet_amd import transforms as T
    x = _batch(4, 6, 32, 64, 19)
    T.Stereo_color()(x.clone())                     # warm-up: library load, allocator
    torch.cuda.synchronize()
    a = x.clone()
    torch.cuda.set_sync_debug_mode("error")
    try:
        T.Stereo_color()(a)
        T.Stereo_normalize()(a)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()


def test_one_launch_per_batch(hip_lib):
    """B = 4: the four 3-element normal_ draws of Lighting and ONE stereo_color_kernel."""
    from torch.profiler import ProfilerActivity, profile
    from dsmnet_amd import transforms as T
    x = _batch(4, 6, 32, 64, 23)
    t = T.Stereo_color()
    t(x.clone())
    torch.cuda.synchronize()
    a = x.clone()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        t(a)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ours = [n for n in kernels if "stereo_color_kernel" in n]
    assert len(ours) == 1, kernels
    assert len(kernels) == 5, kernels


def _selfsup_batch(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 6, H // 16 + 2, W // 16 + 2, generator=g)
    x = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    x = (x + 0.05 * torch.rand(B, 6, H, W, generator=g)).clamp(0, 1)
    x[:, :, H // 4:H // 2, W // 4:W // 2] *= 0.05        # dark pixels
    return x.cuda()


def _model_and_loss(seed):
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(seed)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lossfun = train.losses("depthmono-mask", model.count_levels, 10)
    lossfun.Weight_Adjust_levels(4)
    return model, lossfun


def test_train_and_validate_steps_with_the_transforms(hip_lib):
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    from dsmnet_amd import transforms as T
    old = cv.get_option("conv_precision")
    cv.set_option("conv_precision", "bf16x3")
    try:
        model, lossfun = _model_and_loss(0)
        batch = _selfsup_batch(2, 192, 384, 31)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        random.seed(7)
        torch.manual_seed(7)
        fused = train.train_step_selfsup(model, opt, lossfun, batch, augment=T.Stereo_color())
        random.seed(7)
        torch.manual_seed(7)
        ref = train.train_step_selfsup(model, opt, lossfun, batch,
                                       augment=lambda b: CO.stereo_color_batch_torch(b, same_group=True))
        assert np.isfinite(fused[0])
        assert abs(fused[0] - ref[0]) <= 1e-4 * abs(ref[0]), (fused, ref)
        random.seed(8)
        torch.manual_seed(8)
        v_fused = train.validate_step_selfsup(model, lossfun, batch, augment=T.Stereo_normalize())
        random.seed(8)
        torch.manual_seed(8)
        v_ref = train.validate_step_selfsup(model, lossfun, batch,
                                            augment=lambda b: CO.stereo_color_batch_torch(b, color=False))
        assert np.isfinite(v_fused[0])
        assert abs(v_fused[0] - v_ref[0]) <= 1e-4 * abs(v_ref[0]), (v_fused, v_ref)
    finally:
        cv.set_option("conv_precision", old)


def test_training_with_augmentation_stays_finite(hip_lib):
    """A few Adam steps (default precision) on random batches with dark pixels: the Gamma drift
    keeps NaN out of the network, the loss and the weights."""
    from dsmnet_amd import train
    from dsmnet_amd import transforms as T
    model, lossfun = _model_and_loss(1)
    adam = train.make_optimizer(model, lr=1e-4)
    aug = T.Stereo_color()
    random.seed(3)
    for step in range(3):
        batch = _selfsup_batch(2, 192, 384, 40 + step)
        loss = train.train_step_selfsup(model, adam, lossfun, batch, augment=aug)[0]
        assert np.isfinite(loss), (step, loss)
    assert all(torch.isfinite(p).all() for p in model.parameters())
