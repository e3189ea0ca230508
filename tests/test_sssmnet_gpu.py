"""SsSMnet[-mask] and common[-mask] objectives on the GPU (csrc/selfsup.hip: the sss_* kernels with
their warp buffer and two-stage backward; the C_ds3 instantiation and its image-gradient
pre-pass): the fused op against the float64 restatement (tests/sssmnet_oracle.py)
run on the same device with the same epsilons, the whole pyramid against the reference fixture,
bit-reproducibility of loss and aux, launch counts, and the training / validation steps through
``train.selfsup_losses``.

Tolerances are those of tests/test_selfsup_gpu.py, for the reasons at the top of that file: loss
1e-5 relative; gradients by its ``_grad_close`` (at most 0.2 % of the elements off by more than
1e-2 x the largest reference gradient -- a cap, not a measurement -- and 2e-4 relative L2 on the
rest).

Inputs are that file's recipe with ONE change: ``0.3 * rand / 2**k`` per pixel is added to every
disparity.  The smooth field alone is piecewise bilinear: its second-order terms
(d[i]/d[i+1] + d[i]/d[i-1] - 2 of C_ds3, d[i+1] + d[i-1] - 2 d[i] of C_ds2) are of rounding size
and their sign -- which is the whole gradient of an absolute value -- is noise in ANY precision.  With the noise, the float32 stock
restatement itself, on the CPU, against the float64 one, on the inputs of the four shape cases
below (``_inputs`` is device-free, so this is repeatable without a GPU), gives (SsSMnet | common):

    1x48x80   nedge 0  [0]      no mask   loss 1.1e-07 | 3.4e-08  no outlier  rel L2 2.8e-06 | 2.9e-06
    1x64x96   nedge 64 [0,1,2]  no mask   loss 2.1e-07 | 8.6e-08  no outlier  rel L2 2.8e-06 | 2.9e-06
    3x64x96   nedge 64 [0,1,2]  -mask     loss 1.6e-07 | 1.2e-07  no outlier  rel L2 2.7e-06 | 2.8e-06
    3x37x101  nedge 0  [0,1,2]  -mask     loss 6.9e-08 | 3.8e-08  no outlier  rel L2 2.0e-06 | 2.1e-06

far inside both caps, so a miss of the fused op is the fused op's.  The further cases give at most
4.0e-07 on the loss, no outlier and 1.9e-05 relative L2 in the same check, but for the low-contrast
one: 6.1e-06 | 5.2e-06, no outlier, 3.9e-05 | 4.4e-05 -- float32 SSIM of images whose variance is
below C2, inside both caps with less room.  Two inputs were CHANGED because the restatement alone
came too near a cap or passed it: the 3x64x96 case had seed 3, where one SsSMnet pixel whose
im_wrap1 is zero in one precision only (weight_lr flips) gave 1.2e-04 relative L2; the low-contrast
case had contrast 0.02, where float32 SsSMnet missed the loss by 1.6e-05.
"""
import numpy as np
import pytest
import torch

from tests import selfsup_oracle as SO
from tests import sssmnet_oracle as XO
from tests.test_selfsup_gpu import _grad_close, _selfsup_batch, _smooth

pytestmark = pytest.mark.gpu


OBJECTIVES = ["sssmnet", "common"]


def _inputs(B, h, w, nedge, levels, seed, dlo, dhi, contrasts=None, step_at=None, n_delts=4):
    """CPU tensors: the image pair, one disparity pair per level, the epsilons of each level.
    ``contrasts``: one factor per batch sample that shrinks its images towards 0.5.  ``step_at``: the
    left disparity of level 0 is 0 left of that column and 40 from it on."""
    g = torch.Generator().manual_seed(seed)
    H0, W0 = h + 2 * nedge, w + 2 * nedge
    full = _smooth(g, B, 6, H0, W0, 0.0, 1.0, 6) + 0.05 * torch.rand(B, 6, H0, W0, generator=g)
    if contrasts is not None:
        full = 0.5 + torch.tensor(contrasts).view(B, 1, 1, 1) * (full - 0.5)
    dLs, dL1s = [], []
    for k in levels:
        hk, wk = -(-h // 2 ** k), -(-w // 2 ** k)
        for out in (dLs, dL1s):
            out.append((_smooth(g, B, 1, hk, wk, dlo, dhi, 4) + 0.3 * torch.rand(B, 1, hk, wk, generator=g)) / 2 ** k)
    if step_at is not None:
        dLs[0] = torch.zeros_like(dLs[0])
        dLs[0][..., step_at:] = 40.0
    torch.manual_seed(seed)
    delts = [tuple(SO.draw_delt() for _ in range(n_delts)) for _ in levels]
    return full, dLs, dL1s, delts


def _views(full, h, w, nedge):
    full1 = torch.flip(full, dims=[-1])
    return (full[:, :3, nedge:nedge + h, nedge:nedge + w], full[:, 3:6],
            full1[:, 3:6, nedge:nedge + h, nedge:nedge + w], full1[:, :3])


def _oracle(objective, views, lt, dLs, dL1s, levels, weights, factors, mask, delts, stats=None,
            dtype=torch.float64, ds3=None, divisors=None):
    """The fused op's contract in ``dtype`` on the tensors' device (entry by entry)."""
    d = lambda t: t.detach().to(dtype)
    imL, imR_src, imL1, imR1_src = map(d, views)
    dLs = [d(x).requires_grad_() for x in dLs]
    dL1s = [d(x).requires_grad_() for x in dL1s]
    loss = 0
    for p, (k, wt, sf, dl) in enumerate(zip(levels, weights, factors, delts)):
        dL, dL1 = dLs[p], dL1s[p]
        im, im1 = imL[:, :, ::2 ** k, ::2 ** k], imL1[:, :, ::2 ** k, ::2 ** k]
        w0 = SO.imwrap_bchw(imR_src, dL, dl[0], False, lt, sf)
        w1 = SO.imwrap_bchw(imR1_src, dL1, dl[1], False, lt, sf)
        if ds3 is not None:
            ds3.append(XO.diff_z_dx(dL.detach().abs() + 1).abs())
        if objective == "sssmnet":
            w01 = SO.imwrap_bchw(w1, dL, dl[2], True, (0, 0), 1)
            w11 = SO.imwrap_bchw(w0, dL1, dl[3], True, (0, 0), 1)
            wc = SO.weight_common(dL, SO.imwrap_bchw(dL1, dL, dl[4], True, (0, 0), 1), sf) if mask else None
            wc1 = SO.weight_common(dL1, SO.imwrap_bchw(dL, dL1, dl[5], True, (0, 0), 1), sf) if mask else None
            dv = divisors[p] if divisors else 1
            loss = loss + (XO.loss_sssmnet(im, w0, w01, dL, dv, wc, stats) +
                           XO.loss_sssmnet(im1, w1, w11, dL1, dv, wc1, stats)) * wt
            continue
        dw = SO.imwrap_bchw(dL1, dL, dl[2], True, (0, 0), 1)
        dw1 = SO.imwrap_bchw(dL, dL1, dl[3], True, (0, 0), 1)
        wc = SO.weight_common(dL, dw, sf) if mask else None
        wc1 = SO.weight_common(dL1, dw1, sf) if mask else None
        loss = loss + (XO.loss_common(im, w0, dL, dw, wc, stats) + XO.loss_common(im1, w1, dL1, dw1, wc1, stats)) * wt
    loss.backward()
    return loss.detach(), [x.grad for x in dLs], [x.grad for x in dL1s]


def _case(objective, B, h, w, nedge, levels, mask, seed, dlo, dhi, **kw):
    from dsmnet_amd import costvolume as cv
    sss = objective == "sssmnet"
    full, dLs, dL1s, delts = _inputs(B, h, w, nedge, levels, seed, dlo, dhi, n_delts=6 if sss and mask else 4, **kw)
    views = _views(full.cuda(), h, w, nedge)
    dLs = [x.cuda().requires_grad_() for x in dLs]
    dL1s = [x.cuda().requires_grad_() for x in dL1s]
    weights = [1.0 / (p + 1) for p in range(len(levels))]
    factors = [2 ** k for k in levels]
    lt = (nedge, nedge)
    args = (views[0], views[1], lt, dLs, views[2], views[3], lt, dL1s, levels, weights, factors, mask, delts)
    # SsSMnet: a smoothness divisor that is NOT the scale factor, as for levels above 2
    okw = {"objective": objective, "ds_divisors": [2 * f for f in factors]} if sss else {"objective": objective}
    loss, aux = cv.selfsup_pyramid_loss(*args, return_aux=True, **okw)
    loss.backward()
    stats, ds3 = [], []
    want, gL, gL1 = _oracle(objective, views, lt, dLs, dL1s, levels, weights, factors, mask, delts, stats, ds3=ds3,
                            divisors=okw.get("ds_divisors"))
    torch.cuda.synchronize()
    grads = [x.grad for x in dLs] + [x.grad for x in dL1s]
    rel = abs(float(loss.detach()) - float(want)) / abs(float(want))
    print("%s B%d %dx%d nedge %d levels %s mask %s: loss %.6f vs %.6f rel %.2e, %s %s" % (
        objective, B, h, w, nedge, levels, mask, float(loss.detach()), float(want), rel,
        "valid" if sss else "fallback", [int(s[1]) for s in stats]))
    assert all(bool(torch.isfinite(x).all()) for x in grads) and bool(torch.isfinite(loss))
    assert rel <= 1e-5
    _grad_close(grads, gL + gL1, "%s case seed %d" % (objective, seed))
    return {"loss": loss.detach(), "aux": aux.cpu(), "grads": grads, "stats": stats, "ds3": ds3, "args": args,
            "okw": okw}


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_one_level_no_mask(hip_lib, objective):
    _case(objective, 1, 48, 80, 0, [0], False, 1, 1.0, 9.0)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_nedge64_scale_factors_1_2_4(hip_lib, objective):
    _case(objective, 1, 64, 96, 64, [0, 1, 2], False, 2, 2.0, 14.0)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_nedge64_mask_batch3(hip_lib, objective):
    _case(objective, 3, 64, 96, 64, [0, 1, 2], True, 13, 2.0, 14.0)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ragged_sizes_mask(hip_lib, objective):
    """37 x 101: no multiple of the tile; at level 2 (10 x 26) the map is smaller than a tile plus
    halo, and has fewer rows than the pre-pass has row chunks (some chunks are empty)."""
    _case(objective, 3, 37, 101, 0, [0, 1, 2], True, 4, 1.0, 12.0)


def test_every_sample_off_the_map_falls_back_to_every_pixel(hip_lib):
    a = _case("common", 1, 40, 64, 0, [0], True, 5, 70.0, 90.0)
    assert a["aux"][:, 1].tolist() == [1.0, 1.0]
    assert all(bool(s[1]) for s in a["stats"])


def test_sssmnet_every_sample_off_the_map_gives_w_0001_and_a_finite_loss(hip_lib):
    a = _case("sssmnet", 1, 40, 64, 0, [0], True, 5, 70.0, 90.0)
    assert [int(s[1]) for s in a["stats"]] == [0, 0]
    assert a["aux"][:, 0].tolist() == [float(np.float32(0.001))] * 2
    assert a["aux"][:, 1].tolist() == [0.0, 0.0]
    assert bool(torch.isfinite(a["aux"][:, [0, 1, 2]]).all())


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_fewer_than_1024_pixels(hip_lib, objective):
    a = _case(objective, 1, 20, 40, 0, [0], True, 6, 0.5, 8.0)
    assert a["aux"][:, 1].tolist() == ([0.0, 0.0] if objective == "sssmnet" else [1.0, 1.0])


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_low_contrast_w_above_its_floor(hip_lib, objective):
    """Images of contrast 0.04, a fifth of the samples outside, 2560 pixels: the masked mean SSIM is
    above 0.75 and w ~ 0.03 instead of its floor of 0.001, so the smoothness term (and SsSMnet's
    C_lr) carries percents of the gradient, not tenths of a percent as in the cases above -- an
    order above what ``_grad_close`` lets pass."""
    a = _case(objective, 1, 40, 64, 0, [0], True, 9, 4.0, 12.0, contrasts=[0.04])
    assert a["aux"][:, 1].tolist() == [0.0, 0.0]
    assert all(float(w) > 0.02 for w in a["aux"][:, 0])
    for v, (w, _, simlary) in enumerate(a["stats"]):
        assert abs(float(a["aux"][v, 3]) - float(simlary)) <= 1e-5 * float(simlary)
        assert abs(float(a["aux"][v, 0]) - float(w)) <= 0.5e-5 * float(simlary) + 1e-7


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("step_at", [9, 16])
def test_a_disparity_step_clamps_the_ratio_term_at_10(hip_lib, step_at, objective):
    """0 -> 40 inside a tile (x = 9) and on a tile border (x = 16): on d = |disp| + 1 the ratio
    term is 41/1 + 41/41 - 2 = 40 right of the step, clamped to 10 with no gradient, and
    1/41 + 1/1 - 2 = -0.98 left of it, unclamped."""
    a = _case(objective, 1, 40, 64, 0, [0], True, 7, 1.0, 6.0, step_at=step_at)
    r = a["ds3"][0]
    assert float(r[0, 0, 3, step_at]) == 40.0 and abs(float(r[0, 0, 3, step_at - 1]) - 40.0 / 41.0) < 1e-12
    assert float(r[..., :step_at - 1].max()) == 0.0 and float(r[..., step_at + 1:].max()) == 0.0


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_the_image_gradient_mean_is_per_batch_sample(hip_lib, objective):
    """Three samples of contrast 1, 0.3 and 0.1: one mean over the batch instead of one per sample
    would weight the low-contrast samples' smoothness by exp(-max/(0.5 m)) with an m several
    times too large."""
    a = _case(objective, 3, 40, 72, 0, [0, 1], True, 8, 1.0, 10.0, contrasts=[1.0, 0.3, 0.1])
    views = a["args"][0:2]
    m = XO.diff1_dx(views[0].double()).abs().mean((1, 2, 3))
    assert float(m[0] / m[2]) > 8.0


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_loss_and_aux_are_bit_identical_from_run_to_run(hip_lib, objective):
    from dsmnet_amd import costvolume as cv
    a = _case(objective, 3, 37, 101, 0, [0, 1, 2], True, 4, 1.0, 12.0)
    for _ in range(2):
        loss, aux = cv.selfsup_pyramid_loss(*a["args"], return_aux=True, **a["okw"])
        assert torch.equal(loss.detach(), a["loss"]) and torch.equal(aux.cpu(), a["aux"])


def _launches(fn, monkeypatch):
    """Launch names (one "+"-joined name per entry into the library, one kernel per part) and how
    often torch.zeros was called meanwhile (the fill launch), as tests/test_cap_gpu.py counts them."""
    from dsmnet_amd import costvolume as cv
    names, fills = [], []

    class Timer(cv.LaunchTimer):
        def stop(self, name, start, work):
            names.append(name)
    real = torch.zeros

    def zeros(*a, **k):
        fills.append(a)
        return real(*a, **k)
    cv.set_timer(Timer())
    try:
        with monkeypatch.context() as m:
            m.setattr(torch, "zeros", zeros)
            fn()
            torch.cuda.synchronize()
    finally:
        cv.set_timer(None)
    return names, len(fills)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_launch_count_does_not_depend_on_the_number_of_entries(hip_lib, monkeypatch, objective):
    """Entries into the library (one ``_timed`` label each, naming its kernels "+"-joined) and
    torch.zeros calls; the kernels inside an entry are listed in profiles/sssmnet.md from a trace."""
    from dsmnet_amd import costvolume as cv
    out = []
    for levels in ([0], [0, 1, 2]):
        full, dLs, dL1s, delts = _inputs(2, 40, 96, 0, levels, 12, 1.0, 10.0, n_delts=6 if objective == "sssmnet" else 4)
        views = _views(full.cuda(), 40, 96, 0)
        dLs = [x.cuda().requires_grad_() for x in dLs]
        dL1s = [x.cuda().requires_grad_() for x in dL1s]
        args = (views[0], views[1], (0, 0), dLs, views[2], views[3], (0, 0), dL1s, levels, [1.0] * len(levels),
                [2 ** k for k in levels], True, delts)
        out.append(_launches(lambda: cv.selfsup_pyramid_loss(*args, objective=objective).backward(), monkeypatch))
    want = {"common": ["selfsup_common_fwd_gradmean+tiles+reduce", "selfsup_common_bwd"],
            "sssmnet": ["selfsup_sssmnet_fwd_warp+tiles+reduce", "selfsup_sssmnet_bwd_tiles+chain"]}[objective]
    assert out[0] == out[1] == (want, 1)


@pytest.mark.parametrize("name", ["SsSMnet-mask", "SsSMnet", "common-mask", "common"])
def test_full_pyramid_vs_reference_fixture(hip_lib, name):
    """train.selfsup_losses(name, 7) end to end (upsampling of levels 3..6, epsilon draws, fused op)
    against the reference's own losses_pyramid1 + loss_common / losses_pyramid2 + loss_SsSMnet executed in fp64
    (tests/golden/make_goldens_sssmnet.py)."""
    from dsmnet_amd import train
    from tests.conftest import Golden
    z, case = Golden("sssmnet"), "pyr7"
    meta = z.meta["cases"][case]
    lossfun = train.selfsup_losses(name, meta["count_levels"], meta["maxepoch"])
    lossfun.Weight_Adjust_levels(meta["epoch"])
    batch = torch.from_numpy(z[case + ".batch"].astype(np.float32) / 255.0).cuda()
    nedge, n = meta["nedge"], meta["levels"]
    h, w = batch.shape[2:]
    batch1 = torch.flip(batch, dims=[-1])
    dLs = [torch.from_numpy(z["%s.dispL.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
    dL1s = [torch.from_numpy(z["%s.dispL1.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
    args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:h - nedge, nedge:w - nedge],
            "dispLs": dLs, "scale_dispLs": list(range(n)), "LeftTop": [nedge, nedge],
            "imR1_src": batch1[:, :3], "imL1": batch1[:, 3:6, nedge:h - nedge, nedge:w - nedge],
            "dispL1s": dL1s, "scale_dispL1s": list(range(n)), "LeftTop1": [nedge, nedge]}
    torch.manual_seed(meta["seed"])
    loss = lossfun(args)
    assert float(torch.rand(1)[0]) == float(z["%s.%s.next" % (case, name)])      # the CPU generator: as the reference leaves it
    loss.backward()
    tag = "%s.%s" % (case, name)
    want, got = float(z[tag + ".loss"]), float(loss.detach())
    print("%s: loss %.8f vs %.8f rel %.2e" % (tag, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-5 * abs(want), (tag, got, want)
    _grad_close([d.grad for d in dLs] + [d.grad for d in dL1s],
                [torch.from_numpy(z["%s.gL.%d" % (tag, i)]).cuda() for i in range(n)] +
                [torch.from_numpy(z["%s.gL1.%d" % (tag, i)]).cuda() for i in range(n)], tag)


@pytest.mark.parametrize("name", ["depthmono-mask", "Cap_ds-mask"])
def test_built_names_give_the_bits_of_train_losses(hip_lib, name):
    from dsmnet_amd import train
    full, dLs, dL1s, _ = _inputs(2, 40, 96, 0, [0, 1], 13, 1.0, 10.0)
    views = _views(full.cuda(), 40, 96, 0)
    args = {"imR_src": views[1], "imL": views[0], "dispLs": [x.cuda() for x in dLs], "scale_dispLs": [0, 1],
            "LeftTop": [0, 0], "imR1_src": views[3], "imL1": views[2], "dispL1s": [x.cuda() for x in dL1s],
            "scale_dispL1s": [0, 1], "LeftTop1": [0, 0]}
    out = []
    for cls in (train.losses, train.selfsup_losses):
        lossfun = cls(name, 2, 4)
        lossfun.Weight_Adjust_levels(1)
        torch.manual_seed(3)
        out.append(lossfun(args))
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("name", ["SsSMnet-mask", "common-mask"])
def test_train_and_validate_step_dispnetcorr(hip_lib, name):
    """B=2, 192x384 source: one training step with -mask's nedge of 64 (finite loss, a finite
    gradient on every parameter); then, as tests/test_selfsup_gpu.py demands of depthmono-mask, the
    validation step equals a zero-learning-rate training step without the crop under the same seed."""
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    batch = _selfsup_batch(2, 192, 384, 21)
    torch.manual_seed(0)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lossfun = train.selfsup_losses(name, model.count_levels, 10)
    lossfun.Weight_Adjust_levels(4)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    torch.manual_seed(5)
    out = train.train_step_selfsup(model, opt, lossfun, batch)
    assert np.isfinite(out[0]) and out[1:] == (-1.0, -1.0)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    torch.manual_seed(9)
    v = train.validate_step_selfsup(model, lossfun, batch)
    torch.manual_seed(9)
    t = train.train_step_selfsup(model, opt, lossfun, batch, nedge=0)
    assert v[1:] == (-1.0, -1.0)
    assert abs(v[0] - t[0]) <= 1e-6 * abs(t[0]), (v, t)
