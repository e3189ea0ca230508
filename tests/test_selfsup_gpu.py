"""Self-supervised depthmono[-mask] loss on the GPU (csrc/selfsup.hip): the fused op against the
float64 restatement (tests/selfsup_oracle.py) run on the same device with the same epsilons, the
whole pyramid against the reference fixture, and the training / validation steps.

Tolerances.  Loss: 1e-5 relative (fp32 statistics, fp64 tile reduction).  Gradients: at most
0.2 % of the elements off by more than 1e-2 x the largest reference gradient, the others within
2e-4 relative L2.  Why not tighter: the gradient is bilinear in the
sample position, with jumps where a sample crosses a pixel centre (fp32 and fp64 positions differ
by ~1e-5 px, so a few pixels per case land on the other side) and where |d - d_wrap| crosses 0
(the L1 sign); the SSIM adjoint divides by sigma1^2 + sigma2^2 + C2 ~ 1e-3 after the fp32
cancellation E[x^2] - mu^2 (~1e-4 relative); the scatter into the other view's disparity is an
fp32 atomic sum of unordered terms.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import selfsup_oracle as SO

pytestmark = pytest.mark.gpu


def _smooth(g, B, C, H, W, lo, hi, cell=8):
    """Smooth random field in [lo, hi): bilinear upsampling of a coarse uniform grid."""
    coarse = torch.rand(B, C, max(2, H // cell + 2), max(2, W // cell + 2), generator=g, dtype=torch.float64)
    f = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return (lo + (hi - lo) * f).float()


def _oracle(imL, imR_src, lt, dLs, imL1, imR1_src, lt1, dL1s, levels, weights, factors, mask, delts,
            stats=None):
    """The fused op's contract in float64 on the same device (entry by entry)."""
    d = lambda t: t.detach().double()
    imL, imR_src, imL1, imR1_src = map(d, (imL, imR_src, imL1, imR1_src))
    dLs = [d(x).requires_grad_() for x in dLs]
    dL1s = [d(x).requires_grad_() for x in dL1s]
    loss = 0
    for p, (k, wt, sf, dl) in enumerate(zip(levels, weights, factors, delts)):
        dL, dL1 = dLs[p], dL1s[p]
        im, im1 = imL[:, :, ::2 ** k, ::2 ** k], imL1[:, :, ::2 ** k, ::2 ** k]
        w0 = SO.imwrap_bchw(imR_src, dL, dl[0], False, lt, sf)
        w1 = SO.imwrap_bchw(imR1_src, dL1, dl[1], False, lt1, sf)
        dw = SO.imwrap_bchw(dL1, dL, dl[2], True, (0, 0), 1)
        dw1 = SO.imwrap_bchw(dL, dL1, dl[3], True, (0, 0), 1)
        wc = SO.weight_common(dL, dw, sf) if mask else None
        wc1 = SO.weight_common(dL1, dw1, sf) if mask else None
        if stats is not None:
            stats.append((dL - dw).abs().detach() / sf)
        loss = loss + (SO.loss_depthmono(im, w0, dL, dw, wc) + SO.loss_depthmono(im1, w1, dL1, dw1, wc1)) * wt
    loss.backward()
    return loss.detach(), [x.grad for x in dLs], [x.grad for x in dL1s]


def _grad_close(got, want, what):
    """Outliers (off by > 1e-2 x the largest reference gradient) at most 0.2 % of the elements;
    the rest within 2e-4 relative L2 (measured ~3e-6).  The outliers are the pixels on the
    discontinuities named above -- e.g. a disparity sample within ~1e-5 px of the map border,
    where disp_wrap == 0 exactly in one precision and not in the other, flips weight_lr."""
    g = torch.cat([x.flatten().double() for x in got])
    r = torch.cat([x.flatten() for x in want])
    out = (g - r).abs() > 1e-2 * r.abs().max()
    big = out.double().mean().item()
    keep = ~out
    rel = ((g - r)[keep].norm() / r[keep].norm().clamp_min(1e-30)).item()
    print("%s: grad rel L2 (inliers) %.2e, outliers %.4f %%" % (what, rel, 100 * big))
    assert big <= 2e-3, (what, big)
    assert rel <= 2e-4, (what, rel)


def _case(B, h, w, nedge, levels, mask, seed, dlo, dhi, weights=None, off=0.0):
    from dsmnet_amd import costvolume as cv
    g = torch.Generator().manual_seed(seed)
    H0, W0 = h + 2 * nedge, w + 2 * nedge
    full = _smooth(g, B, 6, H0, W0, 0.0, 1.0, 6) + 0.05 * torch.rand(B, 6, H0, W0, generator=g)
    full = full.cuda()
    full1 = torch.flip(full, dims=[-1])
    imL, imR_src = full[:, :3, nedge:nedge + h, nedge:nedge + w], full[:, 3:6]
    imL1, imR1_src = full1[:, 3:6, nedge:nedge + h, nedge:nedge + w], full1[:, :3]
    dLs, dL1s = [], []
    for k in levels:
        hk, wk = -(-h // 2 ** k), -(-w // 2 ** k)
        dLs.append((_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k + off).cuda().requires_grad_())
        dL1s.append((_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k + off).cuda().requires_grad_())
    weights = weights or [1.0 / (p + 1) for p in range(len(levels))]
    factors = [2 ** k for k in levels]
    torch.manual_seed(seed)
    delts = [tuple(SO.draw_delt() for _ in range(4)) for _ in levels]
    loss, aux = cv.selfsup_pyramid_loss(imL, imR_src, (nedge, nedge), dLs, imL1, imR1_src, (nedge, nedge),
                                        dL1s, levels, weights, factors, mask, delts, return_aux=True)
    loss.backward()
    bands = []
    want, gL, gL1 = _oracle(imL, imR_src, (nedge, nedge), dLs, imL1, imR1_src, (nedge, nedge), dL1s,
                            levels, weights, factors, mask, delts, bands)
    torch.cuda.synchronize()
    rel = abs(float(loss.detach()) - float(want)) / abs(float(want))
    print("B%d %dx%d nedge %d levels %s mask %s: loss %.6f vs %.6f rel %.2e" % (
        B, h, w, nedge, levels, mask, float(loss), float(want), rel))
    assert rel <= 1e-5
    _grad_close([d.grad for d in dLs] + [d.grad for d in dL1s], gL + gL1, "case seed %d" % seed)
    return aux.cpu(), bands


def test_nedge0_one_level(hip_lib):
    _case(1, 48, 80, 0, [0], False, 1, 1.0, 9.0)


def test_nedge64_scale_factors_1_2_4(hip_lib):
    _case(1, 64, 96, 64, [0, 1, 2], False, 2, 2.0, 14.0)


def test_nedge64_mask_batch3(hip_lib):
    _case(3, 64, 96, 64, [0, 1, 2], True, 3, 2.0, 14.0)


def test_ragged_sizes_mask(hip_lib):
    _case(3, 37, 101, 0, [0, 1, 2], True, 4, 1.0, 12.0)


def test_samples_off_the_left_edge(hip_lib):
    # disparities of 20-45 px on a 96-wide map: a third of the left view samples outside
    aux, _ = _case(2, 40, 96, 0, [0], True, 5, 20.0, 45.0)


def test_fewer_than_1024_valid_pixels_fallback(hip_lib):
    # 24 x 40 = 960 pixels per view: mask_ap falls back to every pixel
    aux, _ = _case(1, 24, 40, 0, [0], True, 6, 0.5, 30.0)
    assert aux[:, 1].tolist() == [1.0, 1.0]
    aux, _ = _case(1, 40, 64, 0, [0], False, 7, 1.0, 6.0)
    assert aux[:, 1].tolist() == [0.0, 0.0]


def test_mask_weights_in_all_three_bands(hip_lib):
    aux, bands = _case(2, 48, 96, 0, [0, 1], True, 8, 0.0, 12.0)
    delta = torch.cat([b.flatten() for b in bands])
    for lo, hi in ((0, 1), (1, 3), (3, 1e9)):
        frac = ((delta >= lo) & (delta < hi)).double().mean().item()
        assert frac >= 0.05, (lo, hi, frac)


def test_shape_and_device_errors(hip_lib):
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24, device="cuda")
    d = torch.rand(1, 1, 16, 24, device="cuda")
    with pytest.raises(ValueError):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d[:, :, :8]], im, im, (0, 0), [d], [0], [1.0], [1], False,
                                [(1e-5,) * 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.selfsup_pyramid_loss(im.cpu(), im.cpu(), (0, 0), [d.cpu()], im.cpu(), im.cpu(), (0, 0), [d.cpu()],
                                [0], [1.0], [1], False, [(1e-5,) * 4])


def test_no_host_synchronisation(hip_lib):
    """Forward and backward under sync-debug "error": any device->host synchronisation raises."""
    from dsmnet_amd import costvolume as cv
    g = torch.Generator().manual_seed(11)
    im = _smooth(g, 2, 6, 48, 80, 0, 1).cuda()
    dL = (_smooth(g, 2, 1, 48, 80, 1, 8)).cuda().requires_grad_()
    dL1 = (_smooth(g, 2, 1, 48, 80, 1, 8)).cuda().requires_grad_()
    args = (im[:, :3], im[:, 3:], (0, 0), [dL], im[:, 3:], im[:, :3], (0, 0), [dL1], [0], [1.0], [1], True,
            [(1e-5, 2e-5, 3e-5, 4e-5)])
    cv.selfsup_pyramid_loss(*args).backward()            # warm-up: library load, allocator
    torch.cuda.synchronize()
    want = dL.grad.clone()
    dL.grad = dL1.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = cv.selfsup_pyramid_loss(*args)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert torch.allclose(dL.grad, want, rtol=1e-5, atol=1e-9)


def _golden():
    from tests.conftest import Golden
    return Golden("selfsup")


@pytest.mark.parametrize("case", ["pyr7", "ragged"])
def test_full_pyramid_vs_reference_fixture(hip_lib, case):
    """train.losses("depthmono-mask") end to end (upsampling, epsilon draws, fused op) against the
    reference's own losses_pyramid1 executed in fp64 (tests/golden/make_goldens_selfsup.py)."""
    from dsmnet_amd import train
    z = _golden()
    meta = z.meta["cases"][case]
    for name in meta["names"]:
        lossfun = train.losses("depthmono-mask", meta["count_levels"], meta["maxepoch"])
        lossfun.flag_mask = "mask" in name        # plain depthmono: the same op without the weights
        lossfun.Weight_Adjust_levels(meta["epoch"])
        batch = torch.from_numpy(z[case + ".batch"].astype(np.float32) / 255.0).cuda()
        nedge = meta["nedge"]
        h, w = batch.shape[2:]
        batch1 = torch.flip(batch, dims=[-1])
        n = meta["levels"]
        dLs = [torch.from_numpy(z["%s.dispL.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
        dL1s = [torch.from_numpy(z["%s.dispL1.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
        args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:h - nedge, nedge:w - nedge],
                "dispLs": dLs, "scale_dispLs": list(range(n)), "LeftTop": [nedge, nedge],
                "imR1_src": batch1[:, :3], "imL1": batch1[:, 3:6, nedge:h - nedge, nedge:w - nedge],
                "dispL1s": dL1s, "scale_dispL1s": list(range(n)), "LeftTop1": [nedge, nedge]}
        torch.manual_seed(meta["seed"])
        loss = lossfun(args)
        loss.backward()
        tag = "%s.%s" % (case, name)
        want = float(z[tag + ".loss"])
        assert abs(float(loss) - want) <= 1e-5 * abs(want), (tag, float(loss), want)
        _grad_close([d.grad for d in dLs] + [d.grad for d in dL1s],
                    [torch.from_numpy(z["%s.gL.%d" % (tag, i)]).cuda().double() for i in range(n)] +
                    [torch.from_numpy(z["%s.gL1.%d" % (tag, i)]).cuda().double() for i in range(n)], tag)


def _selfsup_batch(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    left = _smooth(g, B, 3, H, W, 0, 1, 6) + 0.05 * torch.rand(B, 3, H, W, generator=g)
    right = torch.roll(left, -5, dims=3)
    return torch.cat([left, right], 1).cuda()


class _OracleLoss(object):
    """The same argument dict, the loss computed by the float32 GPU restatement."""
    flag_mask = True

    def __init__(self, weight_levels):
        self.weight_levels = weight_levels

    def __call__(self, a):
        loss, _ = SO.losses_pyramid1(self.weight_levels, True, a["imR_src"], a["imL"], a["dispLs"],
                                     a["scale_dispLs"], a["LeftTop"], a["imR1_src"], a["imL1"], a["dispL1s"],
                                     a["LeftTop1"], dtype=torch.float32)
        return loss


def test_train_step_selfsup_dispnetcorr_vs_restatement(hip_lib):
    """B=2, 192x384 source, -mask (nedge 64): loss and parameter gradients of one step against the
    same step with the loss from the restatement (bf16x3 convolutions: the model is identical in
    both, so the comparison isolates the loss)."""
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    old = cv.get_option("conv_precision")
    cv.set_option("conv_precision", "bf16x3")
    try:
        torch.manual_seed(0)
        model = model_create_by_name("dispnetcorr", 192).cuda()
        lossfun = train.losses("depthmono-mask", model.count_levels, 10)
        lossfun.Weight_Adjust_levels(4)
        batch = _selfsup_batch(2, 192, 384, 21)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        torch.manual_seed(5)
        l_fused = train.train_step_selfsup(model, opt, lossfun, batch)
        g_fused = [p.grad.detach().clone() for p in model.parameters()]
        torch.manual_seed(5)
        l_ref = train.train_step_selfsup(model, opt, _OracleLoss(lossfun.weight_levels), batch)
        g_ref = [p.grad.detach().clone() for p in model.parameters()]
    finally:
        cv.set_option("conv_precision", old)
    assert l_fused[1:] == (-1.0, -1.0)
    assert abs(l_fused[0] - l_ref[0]) <= 1e-4 * abs(l_ref[0]), (l_fused, l_ref)
    num = sum(((a - b).double() ** 2).sum() for a, b in zip(g_fused, g_ref)) ** 0.5
    den = sum((b.double() ** 2).sum() for b in g_ref) ** 0.5
    print("train step: loss %.6f vs %.6f, parameter-gradient rel L2 %.2e" % (l_fused[0], l_ref[0], num / den))
    assert float(num / den) <= 5e-3
    adam = train.make_optimizer(model, lr=1e-4)
    out = train.train_step_selfsup(model, adam, lossfun, batch)
    assert np.isfinite(out[0])


def test_validate_step_equals_training_loss(hip_lib):
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(1)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lossfun = train.losses("depthmono-mask", model.count_levels, 10)
    lossfun.Weight_Adjust_levels(2)
    batch = _selfsup_batch(1, 128, 256, 31)
    torch.manual_seed(9)
    v = train.validate_step_selfsup(model, lossfun, batch)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    torch.manual_seed(9)
    t = train.train_step_selfsup(model, opt, lossfun, batch, nedge=0)
    assert v[1:] == (-1.0, -1.0)
    assert abs(v[0] - t[0]) <= 1e-6 * abs(t[0]), (v, t)
    with pytest.raises(NotImplementedError):
        train.train_step_selfsup(model, opt, lossfun, batch, world=2)
