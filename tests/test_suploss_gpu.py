"""Fused supervised pyramid loss (csrc/suploss.hip) on the GPU against a float64 restatement:
``oracle.train.losses_pyramid0`` on ``.double()`` copies, CPU autograd for the gradients.

Bounds.  Loss: 1e-5 relative (the project's bound for fp32 fused ops; the kernel's sums are fp64).
Gradients, per item: E_fused = max|g_fused - g64| <= max(2 * E_stock, 1e-6 * max|g64|), where
E_stock is the same figure for the stock fp32 path on the GPU (option off); nothing is excluded.

``sign`` and ``clamp`` are discontinuous, so the inputs are constructed: every coarse prediction
is separable f(x) + g(y) whose neighbour increments have random sign and a magnitude from
s * [0.1, 0.4] or s * [1.2, 2.0]; gt = one level's fine prediction + e, |e| in [0.05, 5].  Between
two coarse centres the fine differences are then one increment / s; the one fine pair that
straddles a centre sees the mean of two increments, which can fall anywhere -- such pixels (and
any pixel of any level within 2e-3 of a discontinuity) are taken out of the MASK (gt = -1), so
that the precondition "no masked pixel within 1e-3 of a discontinuity" holds by construction;
every test asserts it in float64 before comparing anything."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import train as OT

pytestmark = pytest.mark.gpu

MARGIN = 1e-3


def _axis(n, s, g):
    k = max(n - 1, 0)
    big = torch.rand(k, generator=g, dtype=torch.float64) < 0.5
    u = torch.rand(k, generator=g, dtype=torch.float64)
    mag = torch.where(big, 1.2 + 0.8 * u, 0.1 + 0.3 * u) * s
    sign = torch.where(torch.rand(k, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(mag * sign, 0)])


def _pred(B, hc, wc, level, g, offset=60.0):
    s = 2 ** level
    maps = [_axis(wc, s, g)[None, :] + _axis(hc, s, g)[:, None] + offset for _ in range(B)]
    return torch.stack(maps)[:, None].float()                     # (B,1,hc,wc)


def _fine(pred, level, H, W):
    p = pred.double()
    if p.dim() == 3:
        p = p.unsqueeze(1)
    if level > 0:
        p = F.interpolate(p, scale_factor=2 ** level, mode="bilinear", align_corners=False)
    return p[:, :, :H, :W]


def _near(gt, p):
    """Pixels within ``margin`` of a discontinuity of the loss or of the D1 test (float64)."""
    dx, dy = torch.zeros_like(p), torch.zeros_like(p)
    dx[..., :, :-1] = p[..., :, 1:] - p[..., :, :-1]
    dy[..., :-1, :] = p[..., 1:, :] - p[..., :-1, :]
    e = (gt - p).abs()

    def near(margin):
        return ((e < margin) | ((dx != 0) & (dx.abs() < margin)) | ((dy != 0) & (dy.abs() < margin)) |
                ((dx.abs() + dy.abs() - 1).abs() < margin) | ((e - 3).abs() < margin) |
                ((e - 0.05 * gt).abs() < margin))
    return near


def _build(B, H, W, shapes, levels, k0, seed, squeeze=False):
    """preds (fp32, CPU), gt (fp32, CPU) meeting the precondition for every item."""
    g = torch.Generator().manual_seed(seed)
    preds = [_pred(B, hc, wc, level, g) for (hc, wc), level in zip(shapes, levels)]
    fines = [_fine(p, level, H, W) for p, level in zip(preds, levels)]
    u = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(B, 1, H, W, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    gt = fines[k0] + sign * (0.05 + 4.95 * u)
    r = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    gt = torch.where(r < 0.15, torch.zeros_like(gt), gt)                  # about 30 % without
    gt = torch.where((r >= 0.15) & (r < 0.30), -5.0 * u - 0.5, gt)        # ground truth, half negative
    gt = gt.float()
    for p in fines:
        gt[_near(gt.double(), p)(2 * MARGIN)] = -1.0
    if squeeze:
        preds = [p[:, 0] for p in preds]
    _precondition(gt, preds, levels)
    return preds, gt


def _precondition(gt, preds, levels):
    H, W = gt.shape[-2:]
    g64 = gt.double().cpu()
    mask = g64 > 0
    assert 0.3 < mask.double().mean() < 0.9                 # about 30 % of gt <= 0
    assert (g64 < 0).any() and (g64 == 0).any()
    for p, level in zip(preds, levels):
        bad = _near(g64, _fine(p.detach().cpu(), level, H, W))(MARGIN) & mask
        assert int(bad.sum()) == 0, (level, int(bad.sum()))


def _oracle(weight_levels, gt, preds, levels, flag_smooth):
    leaves = [p.detach().cpu().double().requires_grad_() for p in preds]
    ds = [d.unsqueeze(1) if d.dim() == 3 else d for d in leaves]
    loss = OT.losses_pyramid0(weight_levels, gt.cpu().double(), ds, levels, flag_smooth)
    loss.backward()
    return float(loss), [d.grad for d in leaves]


def _fused(weight_levels, gt, preds, levels, flag_smooth):
    from dsmnet_amd import costvolume as cv
    leaves = [p.detach().cuda().requires_grad_() for p in preds]
    loss, aux = cv.supervised_pyramid_loss(gt.cuda(), leaves, levels, [weight_levels[k] for k in levels],
                                           flag_smooth)
    loss.backward()
    return loss.detach(), aux, [d.grad for d in leaves]


def _stock(weight_levels, gt, preds, levels, flag_smooth):
    """Today's fp32 torch path on the GPU (the option off)."""
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    lf = train.losses("supervised", len(weight_levels), 1)
    lf.weight_levels = list(weight_levels)
    leaves = [p.detach().cuda().requires_grad_() for p in preds]
    old = cv.set_option("fused_supervised_loss", False)
    try:
        loss = lf({"disp_gt": gt.cuda(), "disps": leaves, "scale_disps": levels, "flag_smooth": flag_smooth})
        loss.backward()
    finally:
        cv.set_option("fused_supervised_loss", old)
    return loss.detach(), [d.grad for d in leaves]


def _check(tag, weight_levels, gt, preds, levels, flag_smooth):
    want, g64 = _oracle(weight_levels, gt, preds, levels, flag_smooth)
    loss, aux, gf = _fused(weight_levels, gt, preds, levels, flag_smooth)
    _, gs = _stock(weight_levels, gt, preds, levels, flag_smooth)
    rel = abs(float(loss) - want) / abs(want)
    print("%s: loss %.9g vs %.9g (rel %.2e)" % (tag, float(loss), want, rel))
    figures = []
    for i, level in enumerate(levels):
        e_f = (gf[i].cpu().double() - g64[i]).abs().max().item()
        e_s = (gs[i].cpu().double() - g64[i]).abs().max().item()
        top = g64[i].abs().max().item()
        figures.append((e_f, e_s, top))
        print("%s: item %d level %d  E_stock %.3e  E_fused %.3e  max|g64| %.3e" % (tag, i, level, e_s, e_f, top))
    assert rel <= 1e-5
    assert float(aux[0]) == float((gt > 0).sum())
    for e_f, e_s, top in figures:
        assert e_f <= max(2 * e_s, 1e-6 * top), figures
    return loss, aux, gf


@pytest.mark.parametrize("flag_smooth", [True, False])
def test_level0_below_one_tile(hip_lib, flag_smooth):
    """(1,1,5,7): one partial tile, odd W (scalar accesses), the zero last row / column."""
    preds, gt = _build(1, 5, 7, [(5, 7)], [0], 0, 11)
    _check("5x7 smooth=%d" % flag_smooth, [1.0], gt, preds, [0], flag_smooth)


def test_level0_across_tile_borders(hip_lib):
    """(2,1,33,70) with three (B,H,W) predictions as PSMNet returns them: 3 x 2 tiles per image,
    the left / upper neighbour's terms cross tile borders."""
    preds, gt = _build(2, 33, 70, [(33, 70)] * 3, [0, 0, 0], 1, 12, squeeze=True)
    assert preds[0].dim() == 3
    _check("33x70", [1.0], gt, preds, [0, 0, 0], True)


H3, W3 = 72, 136
LEVELS3 = list(range(7))


def _weights3():
    from dsmnet_amd import train
    lf = train.losses("supervised", 7, 37)
    lf.Weight_Adjust_levels(10)
    w = lf.weight_levels
    assert sorted(w)[:5] == [0.01] * 5 and 0 < sorted(w)[5] < sorted(w)[6] < 1       # two fractional
    return list(w)


@functools.lru_cache(maxsize=None)
def _case3():
    shapes = [(128 >> k, 192 >> k) for k in LEVELS3]
    shapes[0] = (H3, W3)              # level 0 is used as it is: the caller crops it
    preds, gt = _build(2, H3, W3, shapes, LEVELS3, 2, 13)
    return preds, gt


@functools.lru_cache(maxsize=None)
def _singles3():
    """Each level in a call of its own against the float64 yardstick (loss and gradient)."""
    preds, gt = _case3()
    w = _weights3()
    out = []
    for k in LEVELS3:
        loss, _, gf = _check("72x136 level %d" % k, w, gt, [preds[k]], [k], True)
        out.append((float(loss), gf[0]))
    return out


def test_seven_level_pyramid_with_a_crop_each_level(hip_lib):
    """Predictions (128, 192) / 2^L against gt (2,1,72,136): footprints cut by the crop, coarse
    elements wholly outside it (gradient exactly 0), clamped first taps."""
    preds, gt = _case3()
    singles = _singles3()
    for k in range(1, 7):
        s = 2 ** k
        g = singles[k][1]
        # a coarse element whose footprint [s*c - s/2, s*c + 3s/2) starts beyond the crop
        rows = [c for c in range(g.shape[2]) if s * c - s // 2 >= H3]
        cols = [c for c in range(g.shape[3]) if s * c - s // 2 >= W3]
        assert (rows and cols) or k == 6          # at level 6 (2 x 3 elements) every footprint reaches in
        if rows:
            assert (g[:, :, rows] == 0).all()
        if cols:
            assert (g[:, :, :, cols] == 0).all()
        assert (g != 0).any()


def test_seven_level_pyramid_all_levels_in_one_call(hip_lib):
    """The all-levels call is the sum of the single-item calls: loss to 1e-6 relative, every
    gradient to 1e-6 of its largest entry."""
    preds, gt = _case3()
    singles = _singles3()
    loss, aux, gf = _fused(_weights3(), gt, preds, LEVELS3, True)
    total = sum(s[0] for s in singles)
    assert abs(float(loss) - total) <= 1e-6 * abs(total)
    for k in LEVELS3:
        err = (gf[k] - singles[k][1]).abs().max().item()
        assert err <= 1e-6 * singles[k][1].abs().max().item(), (k, err)
    assert aux.shape == (1 + 4 * 7,)


def test_seven_level_pyramid_zero_weight_is_skipped(hip_lib):
    """One level's weight set to 0: that output is left out of the call and gets no gradient."""
    from dsmnet_amd import train
    preds, gt = _case3()
    singles = _singles3()
    lf = train.losses("supervised", 7, 37)
    lf.weight_levels = _weights3()
    lf.weight_levels[3] = 0
    leaves = [p.cuda().requires_grad_() for p in preds]
    loss = lf({"disp_gt": gt.cuda(), "disps": leaves, "scale_disps": LEVELS3, "flag_smooth": True})
    loss.backward()
    total = sum(s[0] for k, s in enumerate(singles) if k != 3)
    assert abs(float(loss) - total) <= 1e-6 * abs(total)
    assert leaves[3].grad is None
    for k in LEVELS3:
        if k != 3:
            assert (leaves[k].grad - singles[k][1]).abs().max().item() <= 1e-6 * singles[k][1].abs().max().item()
    assert lf.last_metrics is not None and lf.last_metrics[0]() is leaves[0]


def test_random_inputs_loss_only(hip_lib):
    """Plain randn maps on the 7-level shape: the loss is continuous in them (1e-5 relative)."""
    g = torch.Generator().manual_seed(14)
    gt = torch.randn(2, 1, H3, W3, generator=g) * 20 + 10
    preds = [torch.randn(2, 1, 128 >> k, 192 >> k, generator=g) * 20 + 10 for k in LEVELS3]
    preds[0] = preds[0][:, :, :H3, :W3].contiguous()
    w = _weights3()
    want = float(OT.losses_pyramid0(w, gt.double(), [p.double() for p in preds], LEVELS3, True))
    loss, _, _ = _fused(w, gt, preds, LEVELS3, True)
    print("randn: loss %.9g vs %.9g" % (float(loss), want))
    assert abs(float(loss) - want) <= 1e-5 * abs(want)


def test_no_valid_pixel(hip_lib):
    from dsmnet_amd import train
    preds, gt = _case3()
    gt = -gt.abs()
    leaves = [p.cuda().requires_grad_() for p in preds]
    lf = train.losses("supervised", 7, 37)
    lf.weight_levels = _weights3()
    args = {"disp_gt": gt.cuda(), "disps": leaves, "scale_disps": LEVELS3, "flag_smooth": True}
    lf.capturable = True
    loss = lf(args)
    assert torch.is_tensor(loss) and loss.is_cuda and float(loss) == 0.0
    loss.backward()
    assert all(d.grad is not None and (d.grad == 0).all() for d in leaves)
    lf.capturable = False
    eager = lf(args)
    assert isinstance(eager, int) and eager == 0


def test_metrics_match_accuracy(hip_lib):
    """EPE to 1e-5 relative; D1 exactly, as a count of good pixels (the inputs keep |gt - p| at
    least 1e-3 away from 3 and from 0.05 * gt: part of the precondition _build asserts)."""
    preds, gt = _case3()
    _, aux, _ = _fused(_weights3(), gt, preds, LEVELS3, True)
    aux = aux.cpu().double()
    n = float(aux[0])
    g64 = gt.double()
    mask = g64 > 0
    assert n == float(mask.sum())
    for i, k in enumerate(LEVELS3):
        p = _fine(preds[k], k, H3, W3)
        e = (g64 - p).abs()
        assert (((e - 3).abs() >= MARGIN) & ((e - 0.05 * g64).abs() >= MARGIN))[mask].all()
        d1, epe = OT.accuracy(p.numpy(), g64.numpy())
        good_want = int((((e <= 3) | (e / g64 <= 0.05)) & mask).sum())
        good = (100.0 - float(aux[1 + 4 * i + 3])) / 100.0 * n
        print("level %d: EPE %.7g vs %.7g, good %.3f vs %d of %d" % (k, float(aux[1 + 4 * i + 2]), epe, good,
                                                                   good_want, int(n)))
        assert abs(float(aux[1 + 4 * i + 2]) - epe) <= 1e-5 * epe
        assert abs(float(aux[1 + 4 * i + 0]) - epe) <= 1e-5 * epe            # the L1 mean is the EPE
        assert abs(good - round(good)) < 0.05 and round(good) == good_want
        assert abs((100.0 - 100.0 * good_want / n) - d1) <= 1e-9


def test_two_runs_are_bit_identical(hip_lib):
    preds, gt = _case3()
    w = _weights3()
    a = _fused(w, gt, preds, LEVELS3, True)
    b = _fused(w, gt, preds, LEVELS3, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_launch_count(hip_lib):
    """One losses("supervised") forward + backward on a 7-level pyramid: this library is entered
    twice, for the two forward kernels (tiles, reduce) and for the one backward gather."""
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    preds, gt = _case3()
    lf = train.losses("supervised", 7, 37)
    lf.weight_levels = _weights3()
    leaves = [p.cuda().requires_grad_() for p in preds]
    names = []

    class Timer(cv.LaunchTimer):
        def stop(self, name, start, work):
            names.append(name)
    cv.set_timer(Timer())
    try:
        lf({"disp_gt": gt.cuda(), "disps": leaves, "scale_disps": LEVELS3, "flag_smooth": True}).backward()
        torch.cuda.synchronize()
    finally:
        cv.set_timer(None)
    assert names == ["suploss_fwd_tiles+reduce", "suploss_bwd_gather"]
    assert sum(len(n.split("+")) for n in names) == 2 + 1


def test_train_step_with_the_option_on_and_off(hip_lib):
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    g = torch.Generator().manual_seed(3)
    left = torch.rand(2, 3, 128, 256, generator=g)
    disp = torch.full((2, 1, 128, 256), 6.0)
    disp[:, :, :, :6] = 0
    batch = torch.cat([left, torch.roll(left, -6, dims=3), disp], 1).cuda()
    out = {}
    for on in (True, False):
        torch.manual_seed(0)
        model = model_create_by_name("dispnetcorr", 192).cuda()
        lf = train.losses("supervised", model.count_levels, 37)
        lf.Weight_Adjust_levels(10)
        opt = train.make_optimizer(model, lr=1e-4)
        old = cv.set_option("fused_supervised_loss", on)
        try:
            out[on] = train.train_step(model, opt, lf, batch)
            assert (lf.last_metrics is not None) == on
            val = train.validate_step(model, lf, batch)
            assert all(v == v for v in val)
        finally:
            cv.set_option("fused_supervised_loss", old)
    print("train_step on %r off %r" % (out[True], out[False]))
    for a, b in zip(out[True], out[False]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (out[True], out[False])
    assert abs(out[True][0] - out[False][0]) <= 1e-5 * abs(out[False][0])
